"""The image backbone's one-pass fp16 kernels (csrc/vov.hip cmt_img_*_f16, csrc/fpn.hip cmt_rows_to_nchw_f16) and
VoVNet under native_img.set_img_precision('fp16') on the device.  B = 2 throughout.

Kernel oracle: float64 on operands already rounded to fp16 (the packed fp16 weights, fp16 input rows), so they are
exact; the kernel's only errors are the fp32 accumulation and the one rounding of the output.  Bound per element,
derived, not measured:

    |got - ref| <= 2^-11 |ref| + 2^-24 + (K + 8) 2^-24 sum |x w|

(half an fp16 ulp of the result; half an ulp of an fp16 subnormal for results that round below 2^-14, so an output
with sum |x w| = 0 still has a bound; K + 8 fp32 roundings, each at most 2^-24 of the running sum of magnitudes).

Tile geometry the sizes are picked from: 128 output rows per workgroup, 32 per wave; W staged in chunks of 64 k, so
Cin = 32 is a single half chunk per tap, 64 one full chunk, 96 / 160 / 224 full chunks and a trailing half chunk;
the concat's tiles lie within one image, the stem's and the conv's run over the batch."""
import functools
from collections import OrderedDict

import pytest
import torch
import torch.nn.functional as F

import _vov_ref as R

pytestmark = pytest.mark.gpu

B = 2
SENT = 0x7BCD                 # fp16 64 928: never a result here
NAN16 = 0x7E00

# whole backbone under 'fp16' against the quantised restatement (b) below: max abs error over (b)'s max abs value.
# It cannot be derived (a rounding flip in one map moves everything after it), so the bound is 4 x the largest value
# measured on an MI355X with the committed seeds (profiles/img_backbone_f16.txt, "module parity": stage3 of V-39-eSE at
# 37x53; the other outputs of the three specs 2.7e-4 ... 1.08e-3, the chain through CPFPN 5.2e-4 and 4.4e-4).
QUANT_MEASURED = 1.10e-3
QUANT_BOUND = 4 * QUANT_MEASURED


def _NI():
    from projects.mmdet3d_plugin import native_img
    return native_img


def _NF():
    from projects.mmdet3d_plugin import native_fpn
    return native_fpn


def _flag(dev):
    return torch.zeros(1, dtype=torch.int32, device=dev)


def _bits(t):
    return t.detach().cpu().contiguous().view(torch.int16)


def _out16(dev, M, C, extra=5, ld=None):
    """(buffer [M + extra, ld] full of the sentinel, its [M, C] view the kernel writes)"""
    ld = C if ld is None else ld
    buf = torch.full((M + extra, ld), SENT, dtype=torch.int16, device=dev).view(torch.float16)
    return buf, buf[:M, :C]


def _only_rows_written(buf, M, C):
    b = _bits(buf)
    return bool((b[M:] == SENT).all() and (b[:, C:] == SENT).all())


def _nan16(n, C):
    return torch.full((n, C), NAN16, dtype=torch.int16).view(torch.float16)


def _rows16(g, n, C, scale=1.0, extra=3):
    """seeded fp16 rows with ``extra`` NaN rows the kernel must not read"""
    x = (torch.randn(n, C, generator=g) * scale).half()
    return torch.cat([x, _nan16(extra, C)]), x


def _bound(ref, mag, K):
    return 2.0 ** -11 * ref.abs() + 2.0 ** -24 + (K + 8) * 2.0 ** -24 * mag


def _w_nchw(w16, cin):
    """packed [Cout, 9 Cin] tap-major -> float64 (Cout, Cin, 3, 3)"""
    return w16.double().reshape(w16.shape[0], 3, 3, cin).permute(0, 3, 1, 2).contiguous()


def _conv_ref(x16_nchw, w16, shift, cin, stride, relu):
    """(float64 rows of act(conv + shift), rows of sum |x w|) on the fp16 operands"""
    w = _w_nchw(w16, cin)
    y = F.conv2d(x16_nchw.double(), w, None, stride, 1) + shift.double()[None, :, None, None]
    mag = F.conv2d(x16_nchw.double().abs(), w.abs(), None, stride, 1)
    return R.rows_of(torch.relu(y) if relu else y), R.rows_of(mag)


# ---- 1. the stem -----------------------------------------------------------------------------------------------

# 5x7 -> 3x4 = 12 rows per image: below one wave; 9x13 -> 5x7 = 35 per image, 70 in all: three waves, the image
# boundary inside the second
@pytest.mark.parametrize("hw", [(5, 7), (9, 13)], ids=lambda hw: f"{hw[0]}x{hw[1]}")
@pytest.mark.parametrize("cin", [3, 1])
def test_stem(dev, parity_log, cin, hw):
    NI = _NI()
    H, W = hw
    g = torch.Generator().manual_seed(111000 + 10 * cin + 7 * H + W)
    w = torch.randn(64, cin, 3, 3, generator=g) / (9 * cin) ** 0.5
    w16, shift = NI.pack_stem_f16(w, list(R.random_bn(64, g)) + [R.BN_EPS])
    Ho, Wo = (H - 1) // 2 + 1, (W - 1) // 2 + 1
    M = B * Ho * Wo
    # contiguous, and the batch as every other image of a longer one (x_bstride = 2 Cin H W), NaN between
    for strided in (False, True):
        x = torch.randn(B, cin, H, W, generator=g) * 2
        want, mag = _conv_ref(x.half(), w16[:, :9 * cin], shift, cin, 2, True)
        xd = x.to(dev)
        if strided:
            hold = torch.full((2 * B, cin, H, W), float("nan"), device=dev)
            hold[::2] = xd
            xd = hold[::2]
            assert xd.stride(0) == 2 * cin * H * W
        buf, out = _out16(dev, M, 64)
        flag = _flag(dev)
        got = NI.stem_f16(xd, w16.to(dev), shift.to(dev), Cout=64, out=out, range_flag=flag)
        assert got is out and _only_rows_written(buf, M, 64), "the stem wrote beyond its rows"
        err = (out.cpu().double() - want).abs()
        bound = _bound(want, mag, 9 * cin)
        parity_log.append(f"img16 stem {cin}->64 {H}x{W}{' strided' if strided else ''}: {err.max().item():.2e} "
                          f"(bound, largest {bound.max().item():.2e}; worst ratio {(err / bound).max().item():.2f})")
        assert (err <= bound).all()
        assert int(flag.item()) == 0 and (want == 0).any() and want.max().item() > 0.5


# ---- 2. the 3 x 3 conv -----------------------------------------------------------------------------------------

# one half chunk per tap (32), a full chunk and a half (96), the V-99 stage widths with a trailing half chunk (160:
# 2 + half, 224: 3 + half), full chunks only (64), and the two ends of the accumulator count (NB 1 ... 8)
CONV_CH = [(32, 64), (96, 32), (160, 160), (224, 224), (64, 128), (32, 256)]
# from tests/test_gpu_vov.py's CONV_MAPS.  1x5: below one wave, and the taps above and below the only map row are
# padding for every row of the wave (the ballot skip); 5x7 (70 rows in all): three waves, the image boundary inside
# the second; 8x16 (256): two full tiles, one per image; 11x25 (550): five tiles straddling row ends and the image
# boundary, a tail of 38; 2x200: a tile is less than a map row, so whole waves lie in one map row and skip three taps
CONV_MAPS = [(1, 5), (5, 7), (8, 16), (11, 25), (2, 200)]


def _conv_operands(cin, cout, H, W, seed=121, wscale=1.0, xscale=1.0):
    NI = _NI()
    g = torch.Generator().manual_seed(seed * 1000 + cin + 3 * cout + 7 * H + W)
    rows, x16 = _rows16(g, B * H * W, cin, xscale)
    w = torch.randn(cout, cin, 3, 3, generator=g) / (9 * cin) ** 0.5 * wscale
    w16, shift = NI.pack_conv3x3_f16(w, list(R.random_bn(cout, g)) + [R.BN_EPS])
    return rows, R.nchw_of(x16, B, H, W), w16, shift


def _run_conv(dev, rows, w16, shift, H, W, stride, relu, flag=None, nb=0, ldx=None, ldy=None):
    NI = _NI()
    cout, cin = w16.shape[0], w16.shape[1] // 9
    Ho, Wo = (H - 1) // stride + 1, (W - 1) // stride + 1
    M = B * Ho * Wo
    X = rows.to(dev)
    if ldx is not None:                                   # the rows as a column slice of a wider buffer, NaN in the slack
        wide = torch.full((rows.shape[0], ldx), NAN16, dtype=torch.int16, device=dev).view(torch.float16)
        wide[:, :cin] = X
        X = wide[:, :cin]
    buf, out = _out16(dev, M, cout, ld=ldy)
    got = NI.conv3x3_f16(X, w16.to(dev), shift.to(dev), B=B, H=H, W=W, Cin=cin, Cout=cout, stride=stride, relu=relu,
                         out=out, range_flag=flag, nb=nb)
    assert got is out and _only_rows_written(buf, M, cout), "the conv wrote beyond its rows or into the slack"
    return out.cpu()


@pytest.mark.parametrize("stride", [1, 2])
@pytest.mark.parametrize("cin,cout", CONV_CH, ids=[f"{a}-{b}" for a, b in CONV_CH])
def test_conv3x3(dev, parity_log, cin, cout, stride):
    worst = 0.0
    for i, (H, W) in enumerate(CONV_MAPS):
        relu = (i + stride) % 2 == 0          # every map runs with and without ReLU over the two strides
        rows, x16, w16, shift = _conv_operands(cin, cout, H, W)
        want, mag = _conv_ref(x16, w16, shift, cin, stride, relu)
        flag = _flag(dev)
        got = _run_conv(dev, rows, w16, shift, H, W, stride, relu, flag)
        err, bound = (got.double() - want).abs(), _bound(want, mag, 9 * cin)
        worst = max(worst, (err / bound).max().item())
        assert (err <= bound).all(), (H, W, (err / bound).max().item())
        assert int(flag.item()) == 0
        assert ((got >= 0).all() and (want == 0).any()) if relu else (want < 0).any()
        # every divisor nb gives the bits of nb = 0 (the small maps here make the library split the columns; the
        # full-size layers run with nb = Cout / 32)
        blocks = cout // 32
        for nb in [d for d in range(1, blocks + 1) if blocks % d == 0]:
            other = _run_conv(dev, rows, w16, shift, H, W, stride, relu, nb=nb)
            assert torch.equal(_bits(other), _bits(got)), (H, W, nb)
    parity_log.append(f"img16 conv3x3 {cin}->{cout} /{stride}: worst error / bound over {len(CONV_MAPS)} maps {worst:.2f}")


@pytest.mark.parametrize("cin,cout,stride,hw", [(160, 160, 1, (5, 7)), (32, 64, 2, (11, 25)), (64, 128, 1, (8, 16))],
                         ids=["160-160", "32-64-s2", "64-128"])
def test_conv3x3_wide_rows(dev, cin, cout, stride, hw):
    """ldx and ldy wider than the row: the slack of X is NaN and never read, the slack of Y and the rows after the
    last keep their sentinel, and the result is the bits of the dense call"""
    H, W = hw
    rows, x16, w16, shift = _conv_operands(cin, cout, H, W)
    dense = _run_conv(dev, rows, w16, shift, H, W, stride, True)
    wide = _run_conv(dev, rows, w16, shift, H, W, stride, True, ldx=cin + 8, ldy=cout + 24)
    assert torch.equal(_bits(wide), _bits(dense)) and not torch.isnan(wide).any()


def test_conv3x3_all_padding_and_zero_products(dev, parity_log):
    """a map of one row: six of the nine taps are padding for every output row, so whole waves skip them (ballot);
    and one image of zeros, where sum |x w| = 0 and the output is the fp16 of the shift: the bound still holds"""
    cin, cout, H, W = 96, 64, 1, 45
    rows, x16, w16, shift = _conv_operands(cin, cout, H, W)
    rows[H * W:B * H * W] = 0
    x16[1] = 0
    for stride in (1, 2):
        want, mag = _conv_ref(x16, w16, shift, cin, stride, False)
        got = _run_conv(dev, rows, w16, shift, H, W, stride, False)
        err, bound = (got.double() - want).abs(), _bound(want, mag, 9 * cin)
        assert (err <= bound).all()
        Mo = want.shape[0] // B
        assert (mag[Mo:] == 0).all() and torch.equal(_bits(got[Mo:]), _bits(shift.half()[None, :].expand(Mo, cout)))
        parity_log.append(f"img16 conv3x3 96->64 /{stride} 1x45, one image zero: worst error / bound "
                          f"{(err / bound).max().item():.2f}")


def test_conv3x3_subnormal_weights(dev, parity_log):
    """every weight in fp16's subnormal range (|w| < 6.1e-5): the products are kept (the MFMA does not flush fp16
    subnormal operands), so the bound is the one of every other case"""
    cin, cout, H, W = 64, 128, 5, 7
    rows, x16, w16, shift = _conv_operands(cin, cout, H, W, wscale=1e-4, xscale=256.0)
    assert 0 < w16.abs().max().item() < 6.1e-5 and (w16 != 0).float().mean().item() > 0.9
    shift = torch.zeros_like(shift)                       # the result is the products' alone
    want, mag = _conv_ref(x16, w16, shift, cin, 1, False)
    got = _run_conv(dev, rows, w16, shift, H, W, 1, False)
    err, bound = (got.double() - want).abs(), _bound(want, mag, 9 * cin)
    parity_log.append(f"img16 conv3x3 64->128 subnormal weights: {err.max().item():.2e}, |ref| max "
                      f"{want.abs().max().item():.2e} (worst error / bound {(err / bound).max().item():.2f})")
    assert want.abs().max().item() > 0.05 and (got != 0).float().mean().item() > 0.9
    assert (err <= bound).all()


def test_conv3x3_range_flag(dev):
    H, W = 5, 7
    rows, _, w16, shift = _conv_operands(64, 160, H, W)
    flag = _flag(dev)
    _run_conv(dev, rows, w16, shift, H, W, 1, True, flag)
    assert int(flag.item()) == 0
    # inputs inside the range whose pre-activation value is not: 576 products of 6e4 * |w|
    big = torch.cat([torch.full((B * H * W, 64), 6e4).half(), _nan16(3, 64)])
    got = _run_conv(dev, big, w16.abs(), torch.zeros_like(shift), H, W, 2, True, flag)
    assert int(flag.item()) == 1 and torch.isinf(got).any()
    flag.zero_()
    bad = rows.clone()
    bad.view(torch.int16)[B * H * W - 1, 63] = 0x7C00       # +inf in the last pixel's last channel
    _run_conv(dev, bad, w16, shift, H, W, 1, True, flag)
    assert int(flag.item()) == 1


# ---- 3. the aggregation ----------------------------------------------------------------------------------------

CONCAT_SRC = [(64,), (128, 128, 128, 128), (256, 160, 160, 160, 160, 160), (32,) * 8]
# pixels per image: 63 (a partial tile, the last wave with 31 rows) and 129 (one tile plus one pixel)
CONCAT_HW = [63, 129]


@pytest.mark.parametrize("cout", [128, 256])
@pytest.mark.parametrize("widths", CONCAT_SRC, ids=lambda w: "+".join(str(c) for c in w))
def test_concat1x1(dev, parity_log, widths, cout):
    NI = _NI()
    K = sum(widths)
    for HW in CONCAT_HW:
        g = torch.Generator().manual_seed(131000 + K + cout + HW)
        M = B * HW
        pairs = [_rows16(g, M, c) for c in widths]
        x64 = torch.cat([x for _, x in pairs], 1).double()
        # the last source as the C-word column slice of a wider row buffer, NaN outside the slice
        c = widths[-1]
        wide = torch.full((M + 3, c + 24), NAN16, dtype=torch.int16).view(torch.float16)
        wide[:M, 8:8 + c] = pairs[-1][1]
        w = torch.randn(cout, K, 1, 1, generator=g) / K ** 0.5
        w16, shift = NI.pack_concat_f16(w, list(R.random_bn(cout, g)) + [R.BN_EPS])
        want = torch.relu(x64 @ w16.double().T + shift.double())
        mag = x64.abs() @ w16.double().abs().T
        buf, out = _out16(dev, M, cout)
        part = torch.full((B, NI.concat_tiles(HW), cout), float("nan"), device=dev)
        flag = _flag(dev)
        dsrcs = [r.to(dev) for r, _ in pairs[:-1]] + [wide.to(dev)[:M, 8:8 + c]]
        assert dsrcs[-1].stride(0) == c + 24
        got, p = NI.concat1x1_f16(dsrcs, w16.to(dev), shift.to(dev), B=B, HW=HW, Cout=cout, out=out, part=part,
                                  range_flag=flag)
        assert got is out and p is part and _only_rows_written(buf, M, cout), "the concat wrote beyond its rows"
        y = out.cpu().double()
        err, bound = (y - want).abs(), _bound(want, mag, K)
        parity_log.append(f"img16 concat1x1 {'+'.join(str(c) for c in widths)}->{cout} HW {HW}: worst error / bound "
                          f"{(err / bound).max().item():.2f}")
        assert (err <= bound).all(), HW
        assert int(flag.item()) == 0 and (want == 0).any()
        # the partial sums of the stored fp16 values: the fp32 worst case of a sum of n_rows terms
        psum = part.cpu().double()
        assert torch.isfinite(psum).all() and tuple(psum.shape) == (B, (HW + 127) // 128, cout)
        stored = y.view(B, HW, cout)
        for t in range(psum.shape[1]):
            tile = stored[:, 128 * t:128 * (t + 1)]
            assert ((psum[:, t] - tile.sum(1)).abs() <= tile.shape[1] * 2.0 ** -24 * tile.abs().sum(1)).all(), (HW, t)
        # part=None writes none and changes nothing else; two runs are bit-equal
        _, out2 = _out16(dev, M, cout)
        _, none = NI.concat1x1_f16(dsrcs, w16.to(dev), shift.to(dev), B=B, HW=HW, Cout=cout, out=out2)
        assert none is None and torch.equal(_bits(out2), _bits(out))


def test_concat1x1_range_flag(dev):
    NI = _NI()
    HW, M = 63, B * 63
    x = torch.full((M, 64), 6e4).half()
    w16 = torch.full((128, 64), 0.5).half()
    flag = _flag(dev)
    y, _ = NI.concat1x1_f16([x.to(dev)], w16.to(dev), torch.zeros(128, device=dev), B=B, HW=HW, Cout=128, range_flag=flag)
    assert int(flag.item()) == 1 and torch.isinf(y).all()
    flag.zero_()
    NI.concat1x1_f16([(x / 64).to(dev)], w16.to(dev), torch.zeros(128, device=dev), B=B, HW=HW, Cout=128, range_flag=flag)
    assert int(flag.item()) == 0


# ---- 4. the apply ----------------------------------------------------------------------------------------------

@pytest.mark.parametrize("HW", [1, 63])
@pytest.mark.parametrize("identity", [False, True], ids=["plain", "identity"])
@pytest.mark.parametrize("inplace", [False, True], ids=["out", "inplace"])
def test_ese_apply(dev, parity_log, inplace, identity, HW):
    NI = _NI()
    C, M = 256, B * HW
    g = torch.Generator().manual_seed(151000 + HW)
    xr, x = _rows16(g, M, C, 3.0, extra=2)
    rr, r = _rows16(g, M, C, 3.0, extra=2)
    gate = torch.rand(B, C, generator=g)
    gate[0, :4] = torch.tensor([0.0, 1.0, 0.0, 1.0])
    xg = x.double().view(B, HW, C) * gate.double()[:, None, :]
    res = r.double().view(B, HW, C) if identity else torch.zeros_like(xg)
    want = (xg + res).view(M, C)
    buf, out = _out16(dev, M, C)
    if inplace:
        out[:M] = x.to(dev)
    flag = _flag(dev)
    got = NI.ese_apply_f16(out if inplace else xr.to(dev), gate.to(dev), B=B, HW=HW, C=C,
                           identity=rr.to(dev) if identity else None, out=out, range_flag=flag)
    assert got is out and _only_rows_written(buf, M, C)
    err = (out.cpu().double() - want).abs()
    bound = 2.0 ** -11 * want.abs() + 2.0 ** -24 + 2.0 ** -22 * (xg.abs() + res.abs()).view(M, C)
    parity_log.append(f"img16 ese_apply{' +id' if identity else ''}{' in place' if inplace else ''} HW {HW}: "
                      f"{err.max().item():.2e} (worst error / bound {(err / bound).max().item():.2f})")
    assert (err <= bound).all() and int(flag.item()) == 0


def test_ese_apply_range_flag(dev):
    NI = _NI()
    C, HW = 256, 63
    x = torch.full((B * HW, C), 1.0).half()
    x[B * HW - 1, C - 1] = 4e4
    r = torch.full((B * HW, C), 4e4).half()
    gate = torch.ones(B, C)
    flag = _flag(dev)
    NI.ese_apply_f16(x.to(dev), gate.to(dev), B=B, HW=HW, C=C, range_flag=flag)
    assert int(flag.item()) == 0                       # neither term leaves the range
    NI.ese_apply_f16(x.to(dev), (0.5 * gate).to(dev), B=B, HW=HW, C=C, identity=r.to(dev), range_flag=flag)
    assert int(flag.item()) == 0                       # 2e4 + 4e4
    y = NI.ese_apply_f16(x.to(dev), gate.to(dev), B=B, HW=HW, C=C, identity=r.to(dev), range_flag=flag)
    assert int(flag.item()) == 1                       # 4e4 + 4e4, in the last row's last channel
    assert torch.isinf(y[B * HW - 1, C - 1]).item() and torch.isfinite(y[:B * HW - 1]).all()


# ---- 5. the pool -----------------------------------------------------------------------------------------------

# even and odd extents; Ho = (H - 2) / 2 + 1, so both have a clipped last window: 10x14 (windows of 2 at the far
# edges), 5x7 and 3x3 (exact), 4x5 (clipped rows, exact columns), 2x2 (one clipped window)
@pytest.mark.parametrize("hw", [(2, 2), (3, 3), (4, 5), (10, 14), (5, 7)], ids=lambda hw: f"{hw[0]}x{hw[1]}")
@pytest.mark.parametrize("C", [128, 160])
def test_maxpool(dev, C, hw):
    NI = _NI()
    H, W = hw
    Ho, Wo = NI.pool_hw(H, W)
    M = B * Ho * Wo
    g = torch.Generator().manual_seed(161000 + C + 7 * H + W)
    for case in ("random", "negative", "ties", "nan"):
        x = torch.randn(B, C, H, W, generator=g).half()
        if case == "negative":
            x = -x.abs() - 0.5                       # a zero-initialised maximum would win everywhere
        if case == "ties":
            # every maximum is a zero, of either sign: equal values with different bits, the first in window order wins
            x = -x.abs() - 0.5
            zero = torch.rand(B, C, H, W, generator=g) < 0.4
            sign = torch.rand(B, C, H, W, generator=g) < 0.5
            x[zero & sign] = 0.0
            x[zero & ~sign] = -0.0
        if case == "nan":
            x[torch.rand(B, C, H, W, generator=g) < 0.1] = float("nan")
        rows = R.rows_of(x)
        want, idx = F.max_pool2d(x.double(), 3, 2, ceil_mode=True, return_indices=True)
        assert tuple(want.shape) == (B, C, Ho, Wo)
        # the oracle's winning element, bit for bit
        src = _bits(rows).view(B, H * W, C).permute(0, 2, 1)                       # [B, C, H*W]
        expect = torch.gather(src, 2, idx.view(B, C, Ho * Wo)).permute(0, 2, 1).reshape(M, C)
        buf, out = _out16(dev, M, C)
        got = NI.maxpool_f16(torch.cat([rows, _nan16(3, C)]).to(dev), B=B, H=H, W=W, C=C, out=out)
        assert got is out and _only_rows_written(buf, M, C)
        assert torch.equal(_bits(out), expect), f"{case}: not the oracle's winning element"
        if case == "ties":
            assert (expect == 0).any() and (expect == -32768).any()       # +0 and -0 both win somewhere
        if case == "nan":
            assert torch.isnan(out).any() and not torch.isnan(out).all()


# ---- 6. to NCHW ------------------------------------------------------------------------------------------------

# HW 1 and 63: the scalar stores, a partial 64-pixel tile; 64: the 16-byte stores (HW % 4 == 0); C 72: a partial
# 64-channel tile of 8
@pytest.mark.parametrize("HW", [1, 63, 64])
@pytest.mark.parametrize("C", [72, 128])
def test_rows_to_nchw_f16(dev, C, HW):
    NF = _NF()
    g = torch.Generator().manual_seed(171000 + C + HW)
    rows, x = _rows16(g, B * HW, C, 100.0)
    x.view(torch.int16)[0, :4] = torch.tensor([1, -32767, 0x7BFF, 0x0400], dtype=torch.int16)   # subnormals, max, min normal
    rows[:B * HW] = x
    out = torch.full((B, C, HW, 1), float("nan"), device=dev)
    got = NF.rows_to_nchw_f16(rows.to(dev), (B, C, HW, 1), out=out)
    want = x.float().view(B, HW, C).permute(0, 2, 1).reshape(B, C, HW, 1).contiguous()
    assert got is out and torch.equal(got.cpu().view(torch.int32), want.view(torch.int32))


# ---- 7. the stem's flag ----------------------------------------------------------------------------------------

def test_stem_range_flag(dev):
    NI = _NI()
    g = torch.Generator().manual_seed(181)
    x = torch.randn(B, 3, 9, 13, generator=g)
    w16, shift = NI.pack_stem_f16(torch.randn(64, 3, 3, 3, generator=g) / 27 ** 0.5, list(R.random_bn(64, g)) + [R.BN_EPS])
    flag = _flag(dev)
    run = lambda img, w: NI.stem_f16(img.to(dev), w.to(dev), shift.to(dev), Cout=64, range_flag=flag)   # noqa: E731
    run(x, w16)
    assert int(flag.item()) == 0
    bad = x.clone()
    bad[1, 2, 8, 12] = 7e4                              # a pixel outside the range: the last pixel of the last image
    run(bad, w16)
    assert int(flag.item()) == 1
    flag.zero_()
    bad = x.clone()
    bad[0, 1, 0, 0] = float("nan")
    run(bad, w16)
    assert int(flag.item()) == 1
    flag.zero_()
    run(torch.full_like(x, 6e4), torch.full_like(w16, 0.5))      # pixels inside the range, 27 products of 3e4
    assert int(flag.item()) == 1


# ---- 8. the module ---------------------------------------------------------------------------------------------

def _fold16(sd, prefix):
    """(float64 of the fp16-rounded folded weight (Cout, Cin, k, k), float64 of the fp32 shift): the pack, restated"""
    w = sd[prefix + "/conv.weight"]
    gamma, beta, mean, var = (sd[f"{prefix}/norm.{n}"] for n in R.BN_NAMES)
    scale = gamma / torch.sqrt(var + R.BN_EPS)
    return (w * scale[:, None, None, None]).half().double(), (beta - mean * scale).float().double()


def vovnet_quant(sd, spec_name, x, out_features=R.NAMES):
    """The chain of _vov_ref.vovnet_ref with the one-pass policy's storage: weights folded in float64 and rounded once
    to fp16, the image and every stored map rounded to fp16, the shift, the fc and the gate fp32; exact (float64)
    arithmetic between the roundings.  An ordered dict name -> float64 NCHW map of fp16 values."""
    sd = {k: v.detach().cpu().double() for k, v in sd.items() if v.is_floating_point()}
    lpb, blocks = R.SHAPE[spec_name]
    q = lambda t: t.half().double()   # noqa: E731

    def cbr(x, prefix, stride):
        w, shift = _fold16(sd, prefix)
        return q(torch.relu(F.conv2d(x, w, None, stride, w.shape[-1] // 2) + shift[None, :, None, None]))

    outs = OrderedDict()
    x = q(x.cpu().float())
    for i, stride in enumerate((2, 1, 2)):
        x = cbr(x, f"stem.stem_{i + 1}", stride)
    if "stem" in out_features:
        outs["stem"] = x
    for i, name in enumerate(R.NAMES[1:]):
        if i > 0:
            x = F.max_pool2d(x, 3, 2, ceil_mode=True)
        for k in range(blocks[i]):
            blk = f"OSA{i + 2}_{k + 1}"
            p = f"{name}.{blk}"
            feats, cur = [x], x
            for j in range(lpb):
                cur = cbr(cur, f"{p}.layers.{j}.{blk}_{j}", 1)
                feats.append(cur)
            y = cbr(torch.cat(feats, 1), f"{p}.concat.{blk}_concat", 1)
            gate = R.ese_gate_ref(y, sd[f"{p}.ese.fc.weight"].float(), sd[f"{p}.ese.fc.bias"].float()).float().double()
            x = q(y * gate + x) if k > 0 else q(y * gate)
        if name in out_features:
            outs[name] = x
    return outs


MODULE_CASES = [("V-19-eSE", (2, 3, 37, 53), R.NAMES), ("V-39-eSE", (2, 3, 37, 53), R.NAMES),
                ("V-99-eSE", (2, 3, 64, 96), ("stage4", "stage5"))]


def _module(spec, feats, seed=39, **kw):
    from projects.mmdet3d_plugin import build_backbone
    m = build_backbone(dict(type="VoVNet", spec_name=spec, out_features=feats, **kw))
    return R.seed_by_key(m, seed).eval()


@functools.lru_cache(maxsize=None)
def _yardsticks(spec, shape, feats):
    """(the image, (a) the float64 oracle, (b) the quantised restatement), computed once on the CPU and shared"""
    m = _module(spec, feats)
    x = R.seeded_image(3953, shape)
    return x, R.vovnet_ref(m.state_dict(), spec, x, feats), vovnet_quant(m.state_dict(), spec, x, feats)


def _rel(got, ref):
    return ((got.double() - ref).abs().max() / ref.abs().max()).item()


class _Precision:
    def __init__(self, mode):
        self.mode = mode

    def __enter__(self):
        self.old = _NI().set_img_precision(self.mode)

    def __exit__(self, *exc):
        _NI().set_img_precision(self.old)


@pytest.mark.parametrize("spec,shape,feats", MODULE_CASES, ids=[s for s, _, _ in MODULE_CASES])
def test_module(dev, parity_log, spec, shape, feats):
    x, ref_a, ref_b = _yardsticks(spec, shape, feats)
    m = _module(spec, feats).to(dev)
    with _Precision("fp16"):
        outs = m(x.to(dev))
        m.check_input_range()                                 # a clean run does not raise
        again = m(x.to(dev))
    assert list(outs) == [n for n in R.NAMES if n in feats] == list(ref_a)
    lines = []
    for k in outs:
        got = outs[k]
        assert got.dtype == torch.float32 and got.is_cuda and got.is_contiguous() and got.shape == ref_a[k].shape, k
        assert torch.equal(again[k], got), "two runs differ"
        assert torch.equal(got.cpu().half().float(), got.cpu()), "an output that is no fp16 value"
        nat_a, quant_a, nat_b = _rel(got.cpu(), ref_a[k]), _rel(ref_b[k], ref_a[k]), _rel(got.cpu(), ref_b[k])
        lines.append((k, nat_a, quant_a, nat_b))
    parity_log.append(f"img16 backbone {spec} {shape[2]}x{shape[3]} (native-oracle / quantised-oracle / native-quantised): "
                      + " ".join(f"{k} {a:.2e}/{q:.2e}/{b:.2e}" for k, a, q, b in lines))
    for k, nat_a, quant_a, nat_b in lines:
        assert nat_a <= 2 * quant_a, (k, nat_a, quant_a)      # the policy costs what its arithmetic costs, no more
        assert nat_b <= QUANT_BOUND, (k, nat_b)


def test_chain_into_the_neck(dev, parity_log):
    """VoVNet under 'fp16' -> CPFPN (untouched: three-pass on fp32 NCHW) against both yardsticks chained into the
    neck's oracle"""
    import _fpn_ref as RF
    from projects.mmdet3d_plugin import build_neck
    spec, shape, feats = MODULE_CASES[2]
    x, ref_a, ref_b = _yardsticks(spec, shape, feats)
    neck = RF.seed_neck(build_neck(dict(type="CPFPN", in_channels=[768, 1024], out_channels=256, num_outs=2)), 12).eval()
    na, nb = RF.cpfpn_ref(neck, list(ref_a.values())), RF.cpfpn_ref(neck, list(ref_b.values()))
    m = _module(spec, feats).to(dev)
    neck.to(dev)
    with _Precision("fp16"):
        outs = neck(list(m(x.to(dev)).values()))
    assert len(outs) == len(na) == 2
    lines = [(_rel(o.cpu(), a), _rel(b, a), _rel(o.cpu(), b)) for o, a, b in zip(outs, na, nb)]
    parity_log.append("img16 backbone -> neck V-99-eSE 64x96 (native-oracle / quantised-oracle / native-quantised): "
                      + " ".join(f"{a:.2e}/{q:.2e}/{b:.2e}" for a, q, b in lines))
    for nat_a, quant_a, nat_b in lines:
        assert nat_a <= 2 * quant_a and nat_b <= QUANT_BOUND
    m.check_input_range()
    neck.check_input_range()


# ---- 9. the switch ---------------------------------------------------------------------------------------------

def test_switching_back_and_forth(dev):
    feats = ("stage4", "stage5")
    m = _module("V-19-eSE", feats).to(dev)
    x = R.seeded_image(3953, (2, 3, 37, 53)).to(dev)
    with _Precision("ref"):
        first = m(x)
        with _Precision("fp16"):
            middle = m(x)
            fresh = _module("V-19-eSE", feats).to(dev)(x)
        last = m(x)
    for k in first:
        assert torch.equal(first[k], last[k]), "the 'ref' result moved across a toggle"
        assert torch.equal(middle[k], fresh[k]), "'fp16' on a module that ran 'ref' first is not a fresh module's"
        assert not torch.equal(middle[k], first[k])
    # after an in-place update both paths follow it
    with torch.no_grad():
        m.stage3.OSA3_1.layers[1][0].weight.mul_(1.5)
        m.stem[1].running_mean.add_(0.25)
    sd = m.state_dict()
    ref = R.vovnet_ref(sd, "V-19-eSE", x, feats)
    quant = vovnet_quant(sd, "V-19-eSE", x, feats)
    with _Precision("ref"):
        after_ref = m(x)
    with _Precision("fp16"):
        after16 = m(x)
    for k in feats:
        assert not torch.equal(after_ref[k], first[k]) and not torch.equal(after16[k], middle[k])
        assert _rel(after_ref[k].cpu(), ref[k]) <= 1e-5
        assert _rel(after16[k].cpu(), ref[k]) <= 2 * _rel(quant[k], ref[k]) and _rel(after16[k].cpu(), quant[k]) <= QUANT_BOUND


def test_module_range_flag(dev):
    m = _module("V-19-eSE", ("stage5",)).to(dev)
    x = R.seeded_image(3953, (2, 3, 37, 53))
    with _Precision("fp16"):
        m(x.to(dev))
        m.check_input_range()
        bad = x.clone()
        bad[1, 0, 20, 20] = 7e4
        m(bad.to(dev))
        with pytest.raises(ValueError, match="f16 operand range"):
            m.check_input_range()
        m.check_input_range()                                 # cleared by the raise


# ---- 10. the detector ------------------------------------------------------------------------------------------

def test_fusion_detector(dev):
    """CmtDetector fusion at tests/test_gpu_detector.py's small shapes under 'fp16': extract_feat and simple_test are
    the modules called by hand under the same setting, bit for bit, and the 'ref' result does not move"""
    import test_gpu_detector as D
    from projects.mmdet3d_plugin import synthetic as S
    Bd, V = 2, 2
    det, cfg = D._build(dev, "cmt_fusion_nus")
    pts, img4 = D._points(dev, cfg, Bd, 10), D._images(dev, Bd * V, 20)
    with torch.no_grad(), _Precision("ref"):
        ref_img = D._img_by_hand(det, img4)
        ref_res = det.simple_test(pts, D._metas(Bd, S.NUS_YAWS[:V], seed=30), img=img4)
        with _Precision("fp16"):
            metas = D._metas(Bd, S.NUS_YAWS[:V], seed=30)
            want_pts, want_img = D._pts_by_hand(det, pts), D._img_by_hand(det, img4)
            img_feats, pts_feats = det.extract_feat(pts, img4, metas)
            D._same_maps(pts_feats, want_pts)
            D._same_maps(img_feats, want_img)
            assert not torch.equal(want_img[0], ref_img[0])          # the setting reaches the detector's backbone
            assert _rel(want_img[0].cpu(), ref_img[0].cpu().double()) < 0.05
            want = det.pts_bbox_head.get_bboxes(det.pts_bbox_head(want_pts, want_img, metas), metas)
            D._same_results(det.simple_test(pts, metas, img=img4), want, Bd)
            det.check_input_range()
        D._same_maps(D._img_by_hand(det, img4), ref_img)
        again = det.simple_test(pts, D._metas(Bd, S.NUS_YAWS[:V], seed=30), img=img4)
    for a, b in zip(again, ref_res):
        for k in ("boxes_3d", "scores_3d", "labels_3d"):
            assert torch.equal(a["pts_bbox"][k], b["pts_bbox"][k]), "the 'ref' result moved across a toggle"


def test_cli_img_precision(dev, tmp_path):
    """tools/test.py --detector --img-precision fp16 in this process: the backbone runs the one-pass kernels, and the
    process setting is what it was afterwards"""
    import importlib.util
    import json
    import os

    from conftest import PKG
    NI = _NI()
    spec = importlib.util.spec_from_file_location("cmt_test_cli_img16", os.path.join(PKG, "tools", "test.py"))
    cli = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(cli)
    argv = ["cmt_fusion_nus", "--synthetic", "--detector", "--num-query", "32", "--num-layers", "1", "--grid", "32", "32",
            "--frame-size", "188", "320", "--points", "1000"]
    calls = []
    real = NI.conv3x3_f16
    NI.conv3x3_f16 = lambda *a, **kw: (calls.append(kw["Cin"]), real(*a, **kw))[1]
    try:
        with _Precision("ref"):
            assert cli.main(argv + ["--out", str(tmp_path / "ref.json")]) == 0 and not calls
            assert cli.main(argv + ["--img-precision", "fp16", "--out", str(tmp_path / "f16.json")]) == 0 and calls
            assert NI.img_precision() == "ref"
    finally:
        NI.conv3x3_f16 = real
    with pytest.raises(SystemExit):
        cli.parse_args(argv + ["--img-precision", "bf16"])
    for name in ("ref.json", "f16.json"):
        fr = json.loads((tmp_path / name).read_text())["frames"][0]
        assert len(fr["scores_3d"]) > 0 and len(fr["boxes_3d"][0]) == 9
