"""The image backbone kernels (csrc/vov.hip) and VoVNet on the device against the float64 oracle on torch's
CPU ops (tests/_vov_ref.py).  B = 2 throughout, so batch strides and image boundaries show.

Tile geometry the sizes are picked from: cmt_img_stem, cmt_img_conv3x3 and cmt_img_concat1x1 work on 128
output rows per workgroup, 32 per wave; the conv's workgroup holds all Cout (Cout / 32 accumulators per wave),
the concat's 128 output channels, and the concat's tiles lie within one image while the stem's and the conv's
run over the batch (a tile may straddle a map-row end and an image boundary).  W is staged in chunks of 32 k,
so Cin = 32 is one chunk per tap and 64 ... 256 are 2 ... 8.  cmt_img_ese_gate takes 16 outputs per
workgroup, four per wave, 64 channels per lane step; cmt_img_ese_apply and cmt_img_maxpool 8 channels per
thread, 256 threads."""
import pytest
import torch
import torch.nn.functional as F

import _vov_ref as R

pytestmark = pytest.mark.gpu

B = 2
SENTINEL = 0x7BCD
# whole backbone: max abs error over the oracle's max abs value, per output.  The hard condition is the
# project's 1e-3 (north_star); the bound is 4 x the largest value measured on an MI355X with the committed
# seeds (profiles/img_backbone.txt, "module parity", the line "img backbone V-99-eSE 64x96": 1.77e-6 for stage5,
# the end of a chain of 87 convolutions; the other outputs of the three specs 3.9e-7 ... 9.7e-7, the chain
# through CPFPN 1.48e-6 and 1.23e-6), which covers box-to-box differences in fp32 summation order only.
BACKBONE_MEASURED = 1.77e-6
BACKBONE_BOUND = min(4 * BACKBONE_MEASURED, 1e-3)


def _NI():
    from projects.mmdet3d_plugin import native_img
    return native_img


def _NB():
    from projects.mmdet3d_plugin import native_bev
    return native_bev


def _bound(ref):
    """the project's pair bound (tests/test_gpu_bev.py): three f16 passes, <= ~2^-21 per product, plus the
    split of the output"""
    top = ref.abs().max().item()
    return 3e-6 * top + 1e-6 + 2.0 ** -21 * top


def _out_rows(dev, M, C, extra=5):
    return torch.full((M + extra, 2, C), SENTINEL, dtype=torch.int16, device=dev).view(torch.uint16)


def _untouched(out, M):
    return bool((out[M:].cpu().view(torch.int16) == SENTINEL).all())


def _nan_rows(n, C):
    return torch.full((n, 2, C), 0x7E00, dtype=torch.int16).view(torch.uint16)


def _pair_input(g, B_, C, H, W, extra=3):
    """seeded fp32 NCHW -> (pair rows with ``extra`` NaN rows the kernel must not read, the float64 NCHW
    the pair format carries)"""
    x = torch.randn(B_, C, H, W, generator=g)
    rows = R.pair(R.rows_of(x))
    return torch.cat([rows, _nan_rows(extra, C)]), R.nchw_of(R.unpair(rows), B_, H, W)


def _flag(dev):
    return torch.zeros(1, dtype=torch.int32, device=dev)


# ---- 1. the stem -----------------------------------------------------------------------------------------------

# 2x2: smaller than a window; 5x7 / 6x8: odd and even extents (an odd one pads both ends of the strided
# output, an even one the low end only); 23x31 -> 12x16 = 192 rows per image, 384 in all: three workgroup tiles,
# the second across the image boundary; 37x53 -> 19x27 = 513 per image, 1026 in all: eight tiles and a tail of 2
STEM_MAPS = [(2, 2), (5, 7), (6, 8), (23, 31), (37, 53)]


def _stem_operands(cin, H, W, seed=11):
    g = torch.Generator().manual_seed(seed * 1000 + 10 * cin + 7 * H + W)
    x = torch.randn(B, cin, H, W, generator=g)
    w = torch.randn(64, cin, 3, 3, generator=g) / (9 * cin) ** 0.5
    return x, w, R.random_bn(64, g)


def _run_stem(dev, x, w, bn, flag=None):
    NI = _NI()
    wp, shift = NI.pack_stem(w, list(bn) + [R.BN_EPS])
    Ho, Wo = _NB().out_hw(x.shape[2], x.shape[3], 2)
    M = B * Ho * Wo
    out = _out_rows(dev, M, 64)
    got = NI.stem(x.to(dev), wp.to(dev), shift.to(dev), Cout=64, out=out, range_flag=flag)
    assert got is out and _untouched(out, M), "the stem wrote beyond its rows"
    return out[:M]


@pytest.mark.parametrize("hw", STEM_MAPS, ids=lambda hw: f"{hw[0]}x{hw[1]}")
@pytest.mark.parametrize("cin", [3, 1])
def test_stem(dev, parity_log, cin, hw):
    x, w, bn = _stem_operands(cin, *hw)
    want = R.rows_of(R.conv_bn_relu(x, w, bn, R.BN_EPS, stride=2))    # the oracle gets the fp32 image
    flag = _flag(dev)
    got = _run_stem(dev, x, w, bn, flag)
    err = (R.unpair(got) - want).abs().max().item()
    parity_log.append(f"img stem {cin}->64 {hw[0]}x{hw[1]}: {err:.2e} (bound {_bound(want):.2e})")
    assert err <= _bound(want)
    assert int(flag.item()) == 0 and (want == 0).any() and want.max().item() > 0.5


def test_stem_range_flag(dev):
    x, w, bn = _stem_operands(3, 37, 53)
    flag = _flag(dev)
    bad = x.clone()
    bad[0, 1, 0, 0] = float("nan")
    _run_stem(dev, bad, w, bn, flag)
    assert int(flag.item()) == 1
    flag.zero_()
    bad = x.clone()
    bad[1, 2, 36, 52] = 7e4                    # the last pixel of the last image: the last tile's tail of 2 rows
    _run_stem(dev, bad, w, bn, flag)
    assert int(flag.item()) == 1


# ---- 2. the 3 x 3 conv -----------------------------------------------------------------------------------------

# every accumulator count the backbone uses and the two ends: NB = 2, 4, 5, 6, 7, 8; one chunk per tap (32) to 8
CONV_CH = [(32, 64), (64, 128), (256, 160), (160, 160), (192, 192), (224, 224), (32, 256)]
# 1x5: below one wave; 5x7 (70 rows in all): three waves, the image boundary inside the second; 9x13 (234):
# two tiles, the boundary inside the first; 8x16 (256): two full tiles, one per image; 11x25 (550): five tiles,
# a tail of 38; 2x200: wider than the 180 of the NCHW halo conv (a tile is less than a map row)
CONV_MAPS = [(1, 5), (5, 7), (9, 13), (8, 16), (11, 25), (2, 200)]


def _conv_operands(cin, cout, H, W, seed=21):
    g = torch.Generator().manual_seed(seed * 1000 + cin + 3 * cout + 7 * H + W)
    rows, x64 = _pair_input(g, B, cin, H, W)
    w = torch.randn(cout, cin, 3, 3, generator=g) / (9 * cin) ** 0.5
    return rows, x64, w, R.random_bn(cout, g)


def _run_conv(dev, rows, w, bn, H, W, stride, relu, flag=None, nb=0):
    NI, NB = _NI(), _NB()
    cout, cin = w.shape[:2]
    wp, shift = NB.pack_conv3x3(w, list(bn) + [R.BN_EPS])
    Ho, Wo = NB.out_hw(H, W, stride)
    M = B * Ho * Wo
    out = _out_rows(dev, M, cout)
    got = NI.conv3x3(rows.to(dev), wp.to(dev), shift.to(dev), B=B, H=H, W=W, Cin=cin, Cout=cout, stride=stride,
                     relu=relu, out=out, range_flag=flag, nb=nb)
    assert got is out and _untouched(out, M), "the conv wrote beyond its rows"
    return out[:M]


@pytest.mark.parametrize("stride", [1, 2])
@pytest.mark.parametrize("cin,cout", CONV_CH, ids=[f"{a}-{b}" for a, b in CONV_CH])
def test_conv3x3(dev, parity_log, cin, cout, stride):
    for i, (H, W) in enumerate(CONV_MAPS):
        relu = (i + stride) % 2 == 0          # every map runs with and without ReLU over the two strides
        rows, x64, w, bn = _conv_operands(cin, cout, H, W)
        want = R.rows_of(R.conv_bn_relu(x64, w, bn, R.BN_EPS, stride=stride, relu=relu))
        flag = _flag(dev)
        got = _run_conv(dev, rows, w, bn, H, W, stride, relu, flag)
        err = (R.unpair(got) - want).abs().max().item()
        parity_log.append(f"img conv3x3 {cin}->{cout} /{stride}{' relu' if relu else ''} {H}x{W}: {err:.2e} "
                          f"(bound {_bound(want):.2e})")
        assert err <= _bound(want), (H, W)
        assert int(flag.item()) == 0
        assert ((R.unpair(got) >= 0).all() and (want == 0).any()) if relu else (want < 0).any()
        # the maps here are small, so the library splits the columns over workgroups on its own (nb = 0); the
        # full-size layers run with all columns in one workgroup (nb = Cout / 32): that form, and every divisor
        # between, must give the same bits
        blocks = cout // 32
        for nb in [d for d in range(1, blocks + 1) if blocks % d == 0]:
            if nb == blocks or (H, W) in ((5, 7), (11, 25)):
                other = _run_conv(dev, rows, w, bn, H, W, stride, relu, nb=nb)
                assert torch.equal(other.cpu().view(torch.int16), got.cpu().view(torch.int16)), (H, W, nb)
        if (H, W) == (11, 25):
            again = _run_conv(dev, rows, w, bn, H, W, stride, relu)
            assert torch.equal(again.cpu().view(torch.int16), got.cpu().view(torch.int16)), "two runs differ"


def test_conv3x3_routed_shapes(dev, parity_log):
    """the shapes the module routes to cmt_gemm's CMT_A_CONV3X3 path, through the module's routing helper: the
    same maps, ReLU on and off, against the oracle and bit-equal to cmt_img_conv3x3 (same K order)"""
    from projects.mmdet3d_plugin import native_img as NI
    from projects.mmdet3d_plugin.models.backbones import vovnet as V
    NB = _NB()
    assert V.GEMM_ROUTED == {(128, 128)}
    taken = []
    real = NI.conv3x3_gemm
    NI.conv3x3_gemm = lambda *a, **kw: (taken.append(kw["Cin"]), real(*a, **kw))[1]
    try:
        for cin, cout in sorted(V.GEMM_ROUTED):
            for i, (H, W) in enumerate(CONV_MAPS):
                for relu in (True, False):
                    rows, x64, w, bn = _conv_operands(cin, cout, H, W)
                    want = R.rows_of(R.conv_bn_relu(x64, w, bn, R.BN_EPS, stride=1, relu=relu))
                    wp, shift = NB.pack_conv3x3(w, list(bn) + [R.BN_EPS])
                    M = B * H * W
                    out, flag = _out_rows(dev, M, cout), _flag(dev)
                    got = V.route_conv3x3(rows.to(dev), wp.to(dev), shift.to(dev), B=B, H=H, W=W, Cin=cin, Cout=cout,
                                          stride=1, relu=relu, out=out, range_flag=flag)
                    assert got is out and _untouched(out, M), "the routed conv wrote beyond its rows"
                    err = (R.unpair(out[:M]) - want).abs().max().item()
                    parity_log.append(f"img conv3x3 routed {cin}->{cout}{' relu' if relu else ''} {H}x{W}: {err:.2e} "
                                      f"(bound {_bound(want):.2e})")
                    assert err <= _bound(want) and int(flag.item()) == 0, (H, W)
                    own = _run_conv(dev, rows, w, bn, H, W, 1, relu)
                    assert torch.equal(own.cpu().view(torch.int16), out[:M].cpu().view(torch.int16)), (H, W)
        assert len(taken) == 2 * len(CONV_MAPS) * len(V.GEMM_ROUTED)
        # a shape that is not routed, and a routed one at stride 2, stay on cmt_img_conv3x3
        rows, _, w, bn = _conv_operands(64, 128, 5, 7)
        wp, shift = NB.pack_conv3x3(w, list(bn) + [R.BN_EPS])
        V.route_conv3x3(rows.to(dev), wp.to(dev), shift.to(dev), B=B, H=5, W=7, Cin=64, Cout=128, stride=1)
        rows, _, w, bn = _conv_operands(128, 128, 5, 7)
        wp, shift = NB.pack_conv3x3(w, list(bn) + [R.BN_EPS])
        V.route_conv3x3(rows.to(dev), wp.to(dev), shift.to(dev), B=B, H=5, W=7, Cin=128, Cout=128, stride=2)
        assert len(taken) == 2 * len(CONV_MAPS) * len(V.GEMM_ROUTED)
    finally:
        NI.conv3x3_gemm = real
    # a pre-activation value outside the range raises the flag on this path too
    big = torch.cat([R.pair(torch.full((B * 35, 128), 6e4)), _nan_rows(3, 128)])
    one = (torch.ones(128), torch.zeros(128), torch.zeros(128), torch.ones(128))
    wp, shift = NB.pack_conv3x3(w.abs(), list(one) + [0.0])
    flag = _flag(dev)
    V.route_conv3x3(big.to(dev), wp.to(dev), shift.to(dev), B=B, H=5, W=7, Cin=128, Cout=128, stride=1, range_flag=flag)
    assert int(flag.item()) == 1


def test_conv3x3_range_flag(dev):
    H, W = 9, 13
    rows, _, w, bn = _conv_operands(64, 160, H, W)
    flag = _flag(dev)
    _run_conv(dev, rows, w, bn, H, W, 1, True, flag)
    assert int(flag.item()) == 0
    bad = rows.clone()
    bad.view(torch.int16)[B * H * W - 1, 0, 63] = 0x7C00      # +inf in the last pixel's hi half
    _run_conv(dev, bad, w, bn, H, W, 1, True, flag)
    assert int(flag.item()) == 1
    flag.zero_()
    # inputs inside the range whose pre-activation value is not
    big = torch.cat([R.pair(torch.full((B * H * W, 64), 6e4)), _nan_rows(3, 64)])
    one = (torch.ones(160), torch.zeros(160), torch.zeros(160), torch.ones(160))
    _run_conv(dev, big, w.abs(), one, H, W, 2, True, flag)
    assert int(flag.item()) == 1


# ---- 3. the aggregation ----------------------------------------------------------------------------------------

CONCAT_SRC = [(64,), (128, 128, 128, 128), (256, 160, 160, 160, 160, 160), (32,) * 8]
# pixels per image: 1; 35 and 117 (tails no 32-pixel wave tile divides); 128 (one full tile); 275 (three tiles,
# the last with 19 pixels and three waves without any)
CONCAT_HW = [1, 35, 117, 128, 275]


@pytest.mark.parametrize("cout", [128, 256])
@pytest.mark.parametrize("widths", CONCAT_SRC, ids=lambda w: "+".join(str(c) for c in w))
def test_concat1x1(dev, parity_log, widths, cout):
    NI = _NI()
    K = sum(widths)
    for HW in CONCAT_HW:
        g = torch.Generator().manual_seed(31000 + K + cout + HW)
        M = B * HW
        xs = [torch.randn(M, c, generator=g) for c in widths]
        srcs = [torch.cat([R.pair(x), _nan_rows(3, c)]) for x, c in zip(xs, widths)]
        x64 = torch.cat([R.unpair(s[:M]) for s in srcs], 1)
        # the last source as the 2 C-word column slice of a wider row buffer, NaN outside the slice
        c = widths[-1]
        wide = torch.full((M + 3, 2 * c + 24), 0x7E00, dtype=torch.int16).view(torch.uint16)
        wide[:M, 8:8 + 2 * c] = srcs[-1][:M].reshape(M, 2 * c)
        w = torch.randn(cout, K, 1, 1, generator=g) / K ** 0.5
        bn = R.random_bn(cout, g)
        want = R.bn_relu((x64 @ w.double().view(cout, K).T).T.reshape(1, cout, M, 1), bn, R.BN_EPS)[0, :, :, 0].T
        wp, shift = NI.pack_concat(w, list(bn) + [R.BN_EPS])
        out = _out_rows(dev, M, cout)
        part = torch.full((B, NI.concat_tiles(HW), cout), float("nan"), device=dev)
        flag = _flag(dev)
        dsrcs = [s.to(dev) for s in srcs[:-1]] + [wide.to(dev)[:M, 8:8 + 2 * c].view(M, 2, c)]
        assert dsrcs[-1].stride(0) == 2 * c + 24
        got, p = NI.concat1x1(dsrcs, wp.to(dev), shift.to(dev), B=B, HW=HW, Cout=cout, out=out, part=part,
                              range_flag=flag)
        assert got is out and p is part and _untouched(out, M), "the concat wrote beyond its rows"
        y = R.unpair(out[:M])
        err = (y - want).abs().max().item()
        parity_log.append(f"img concat1x1 {'+'.join(str(c) for c in widths)}->{cout} HW {HW}: {err:.2e} "
                          f"(bound {_bound(want):.2e})")
        assert err <= _bound(want), HW
        assert int(flag.item()) == 0 and (want == 0).any()
        # the partial sums: one per (image, tile, column), adding up to the image's column sums.  Against the
        # stored map (what the gate's mean is the mean of) the bound is the fp32 worst case of a sum of n_rows
        # terms alone; against the oracle every term also carries its own pair bound.
        psum = part.cpu().double()
        assert torch.isfinite(psum).all() and tuple(psum.shape) == (B, (HW + 127) // 128, cout)
        stored, oracle = y.view(B, HW, cout), want.view(B, HW, cout)
        fp32 = HW * 2.0 ** -24 * stored.abs().sum(1)
        assert ((psum.sum(1) - stored.sum(1)).abs() <= fp32).all(), HW
        assert ((psum.sum(1) - oracle.sum(1)).abs() <= fp32 + HW * _bound(want)).all(), HW
        for t in range(psum.shape[1]):
            tile = stored[:, 128 * t:128 * (t + 1)]
            assert ((psum[:, t] - tile.sum(1)).abs() <= tile.shape[1] * 2.0 ** -24 * tile.abs().sum(1)).all()
        # part=None writes none and changes nothing else; two runs are bit-equal
        out2 = _out_rows(dev, M, cout)
        _, none = NI.concat1x1(dsrcs, wp.to(dev), shift.to(dev), B=B, HW=HW, Cout=cout, out=out2)
        assert none is None and torch.equal(out2.cpu().view(torch.int16), out.cpu().view(torch.int16))


# ---- 4. the gate -----------------------------------------------------------------------------------------------

@pytest.mark.parametrize("tiles", [1, 3, 37])
@pytest.mark.parametrize("C", [256, 1024])
def test_ese_gate(dev, parity_log, C, tiles):
    NI = _NI()
    g = torch.Generator().manual_seed(41000 + C + tiles)
    HW = 128 * tiles - 5
    part = torch.rand(B, tiles, C, generator=g) * 100.0
    w = torch.randn(C, C, generator=g) / C ** 0.5
    bias = torch.randn(C, generator=g)
    mean = part.double().sum(1) / HW
    # rows 0 .. 5 of fc, scaled (bias 0) so that image 0's pre-activation lands below -3, above +3 and within
    # 1e-3 of both knees, on either side
    targets = [-5.0, 5.0, -3.0 - 5e-4, -3.0 + 5e-4, 3.0 - 5e-4, 3.0 + 5e-4]
    for o, t in enumerate(targets):
        bias[o] = 0.0
        w[o] *= t / (w[o].double() @ mean[0]).item()
    t64 = mean @ w.double().T + bias.double()
    want = R.hsigmoid(t64)
    got = NI.ese_gate(part.to(dev), w.view(C, C, 1, 1).to(dev), bias.to(dev), HW=HW).cpu()
    assert got.dtype == torch.float32 and tuple(got.shape) == (B, C)
    bound = 2.0 ** -24 * (C + tiles + 8) * (mean.abs() @ w.double().abs().T + bias.double().abs()) / 6
    err = (got.double() - want).abs()
    parity_log.append(f"img ese_gate C {C} tiles {tiles}: {err.max().item():.2e} (bound, smallest {bound.min().item():.2e})")
    assert (err <= bound).all()
    assert got[0, 0].item() == 0.0 and got[0, 2].item() == 0.0 and got[0, 1].item() == 1.0 and got[0, 5].item() == 1.0
    assert 0.0 < got[0, 3].item() < 2e-4 and 1.0 - 2e-4 < got[0, 4].item() < 1.0
    assert ((want == 0).sum() >= 2) and ((want == 1).sum() >= 2) and ((want > 0) & (want < 1)).sum() > C


# ---- 5. the apply ----------------------------------------------------------------------------------------------

@pytest.mark.parametrize("HW", [1, 63, 275])
@pytest.mark.parametrize("identity", [False, True], ids=["plain", "identity"])
@pytest.mark.parametrize("inplace", [False, True], ids=["out", "inplace"])
def test_ese_apply(dev, parity_log, inplace, identity, HW):
    NI = _NI()
    C, M = 256, B * HW
    g = torch.Generator().manual_seed(51000 + HW)
    x = R.pair(torch.randn(M, C, generator=g) * 3)
    r = R.pair(torch.randn(M, C, generator=g) * 3)
    gate = torch.rand(B, C, generator=g)
    gate[0, :4] = torch.tensor([0.0, 1.0, 0.0, 1.0])
    xg = R.unpair(x).view(B, HW, C) * gate.double()[:, None, :]
    rr = R.unpair(r).view(B, HW, C) if identity else torch.zeros_like(xg)
    want = (xg + rr).view(M, C)
    buf = _out_rows(dev, M, C)
    if inplace:
        buf.view(torch.int16)[:M] = x.view(torch.int16).to(dev)
    flag = _flag(dev)
    got = NI.ese_apply(buf if inplace else torch.cat([x, _nan_rows(2, C)]).to(dev), gate.to(dev), B=B, HW=HW, C=C,
                       identity=torch.cat([r, _nan_rows(2, C)]).to(dev) if identity else None, out=buf, range_flag=flag)
    assert got is buf and _untouched(buf, M)
    err = (R.unpair(buf[:M]) - want).abs()
    bound = 2.0 ** -21 * (xg.abs() + rr.abs()).view(M, C) + 2.0 ** -25
    parity_log.append(f"img ese_apply{' +id' if identity else ''}{' in place' if inplace else ''} HW {HW}: "
                      f"{err.max().item():.2e} (bound, largest {bound.max().item():.2e})")
    assert (err <= bound).all() and int(flag.item()) == 0


def test_ese_apply_range_flag(dev):
    NI = _NI()
    C, HW = 256, 63
    x = R.pair(torch.full((B * HW, C), 1.0))
    x[B * HW - 1, :, C - 1] = R.pair(torch.tensor([4e4]))[:, 0]
    r = R.pair(torch.full((B * HW, C), 4e4))
    gate = torch.ones(B, C)
    flag = _flag(dev)
    NI.ese_apply(x.to(dev), gate.to(dev), B=B, HW=HW, C=C, range_flag=flag)
    assert int(flag.item()) == 0                       # neither term leaves the range
    NI.ese_apply(x.to(dev), (0.5 * gate).to(dev), B=B, HW=HW, C=C, identity=r.to(dev), range_flag=flag)
    assert int(flag.item()) == 0                       # 2e4 + 4e4
    NI.ese_apply(x.to(dev), gate.to(dev), B=B, HW=HW, C=C, identity=r.to(dev), range_flag=flag)
    assert int(flag.item()) == 1                       # 4e4 + 4e4, in the last row's last channel


# ---- 6. the pool -----------------------------------------------------------------------------------------------

# 2x2 and 3x3: one window (clipped, exact); 4x5: the second window clipped to 2 rows, exact columns; 10x14:
# clipped on both axes; 5x7: exact on both; 2x9: a clipped single row of windows
POOL_MAPS = [(2, 2), (3, 3), (4, 5), (10, 14), (5, 7), (2, 9)]


@pytest.mark.parametrize("hw", POOL_MAPS, ids=lambda hw: f"{hw[0]}x{hw[1]}")
@pytest.mark.parametrize("C", [128, 160])
def test_maxpool(dev, C, hw):
    NI = _NI()
    H, W = hw
    Ho, Wo = NI.pool_hw(H, W)
    g = torch.Generator().manual_seed(61000 + C + 7 * H + W)
    for negative in (False, True):
        x = torch.randn(B, C, H, W, generator=g)
        if negative:
            x = -x.abs() - 0.5                       # a zero-initialised maximum would win everywhere
        rows = R.pair(R.rows_of(x))
        x64 = R.nchw_of(R.unpair(rows), B, H, W)
        want, idx = F.max_pool2d(x64, 3, 2, ceil_mode=True, return_indices=True)
        assert tuple(want.shape) == (B, C, Ho, Wo)
        # the pair of the oracle's maximum: the input pair at the oracle's winning position
        src = rows.view(B, H * W, 2, C).permute(0, 3, 2, 1)                       # [B, C, 2, H*W]
        pick = idx.view(B, C, 1, Ho * Wo).expand(B, C, 2, Ho * Wo)
        expect = torch.gather(src.view(torch.int16), 3, pick).permute(0, 3, 2, 1).reshape(B * Ho * Wo, 2, C)
        M = B * Ho * Wo
        out = _out_rows(dev, M, C)
        got = NI.maxpool(torch.cat([rows, _nan_rows(3, C)]).to(dev), B=B, H=H, W=W, C=C, out=out)
        assert got is out and _untouched(out, M)
        assert torch.equal(out[:M].cpu().view(torch.int16), expect), "not the pair of the oracle's maximum"
        assert torch.equal(R.unpair(out[:M]), R.rows_of(want))
    # equal maxima in one window: either pair is the same pair
    flat = R.pair(torch.full((B * H * W, C), -2.5))
    out = NI.maxpool(flat.to(dev), B=B, H=H, W=W, C=C)
    assert (R.unpair(out) == -2.5).all() and tuple(out.shape) == (B * Ho * Wo, 2, C)


# ---- 7. the module ---------------------------------------------------------------------------------------------

MODULE_CASES = [("V-39-eSE", (2, 3, 37, 53), ("stage4", "stage5")), ("V-19-eSE", (2, 3, 37, 53), ("stage4", "stage5")),
                ("V-99-eSE", (2, 3, 64, 96), ("stage4", "stage5")), ("V-39-eSE", (2, 3, 37, 53), R.NAMES)]


def _module(spec, feats, seed=39, **kw):
    from projects.mmdet3d_plugin import build_backbone
    m = build_backbone(dict(type="VoVNet", spec_name=spec, out_features=feats, **kw))
    return R.seed_by_key(m, seed).eval()


def _rel_errors(outs, ref):
    assert list(outs) == list(ref)
    errs = {}
    for k in ref:
        got = outs[k]
        assert got.dtype == torch.float32 and got.is_cuda and got.is_contiguous() and got.shape == ref[k].shape, k
        errs[k] = ((got.cpu().double() - ref[k]).abs().max() / ref[k].abs().max()).item()
    return errs


@pytest.mark.parametrize("spec,shape,feats", MODULE_CASES,
                         ids=[f"{s}-{'all' if len(f) == 5 else 'out45'}" for s, _, f in MODULE_CASES])
def test_module(dev, parity_log, spec, shape, feats):
    m = _module(spec, feats)
    x = R.seeded_image(3953, shape)
    ref = R.vovnet_ref(m.state_dict(), spec, x, feats)
    m.to(dev)
    outs = m(x.to(dev))
    assert isinstance(outs, dict) and list(outs) == [n for n in R.NAMES if n in feats]
    errs = _rel_errors(outs, ref)
    parity_log.append(f"img backbone {spec} {shape[2]}x{shape[3]}: " +
                      " ".join(f"{k} {e:.2e}" for k, e in errs.items()) + f" (bound {BACKBONE_BOUND:.1e})")
    assert max(errs.values()) <= BACKBONE_BOUND
    m.check_input_range()                                 # a clean run does not raise
    again = m(x.to(dev).double())                         # a float64 image goes through .float()
    assert all(torch.equal(again[k], outs[k]) for k in outs), "two runs differ"
    assert len(list(outs.values())) == len(feats)


def test_module_follows_in_place_updates(dev, parity_log):
    m = _module("V-19-eSE", ("stage4", "stage5")).to(dev)
    x = R.seeded_image(3953, (2, 3, 37, 53))
    before = m(x.to(dev))
    with torch.no_grad():
        m.stage3.OSA3_1.layers[1][0].weight.mul_(1.5)
        m.stem[1].running_mean.add_(0.25)
        m.stage4.OSA4_1.ese.fc.bias.add_(0.5)
    ref = R.vovnet_ref(m.state_dict(), "V-19-eSE", x, ("stage4", "stage5"))
    after = m(x.to(dev))
    errs = _rel_errors(after, ref)
    parity_log.append("img backbone V-19-eSE after in-place updates: " + " ".join(f"{k} {e:.2e}" for k, e in errs.items()))
    assert max(errs.values()) <= BACKBONE_BOUND
    assert not torch.equal(after["stage4"], before["stage4"])


def test_module_range_flag(dev):
    m = _module("V-19-eSE", ("stage5",)).to(dev)
    x = R.seeded_image(3953, (2, 3, 37, 53))
    m(x.to(dev))
    m.check_input_range()
    bad = x.clone()
    bad[1, 0, 20, 20] = 7e4
    m(bad.to(dev))
    with pytest.raises(ValueError, match="f16 operand range"):
        m.check_input_range()
    m.check_input_range()                                 # cleared by the raise


def test_chain_into_the_neck(dev, parity_log):
    """VoVNet -> CPFPN from the fusion config's two dicts against both oracles chained"""
    import _fpn_ref as RF
    from projects.mmdet3d_plugin import build_neck
    m = _module("V-99-eSE", ("stage4", "stage5"), norm_eval=True, frozen_stages=-1, input_ch=3)
    neck = RF.seed_neck(build_neck(dict(type="CPFPN", in_channels=[768, 1024], out_channels=256, num_outs=2)), 12).eval()
    x = R.seeded_image(3953, (2, 3, 64, 96))
    feats = R.vovnet_ref(m.state_dict(), "V-99-eSE", x, ("stage4", "stage5"))
    assert [tuple(v.shape) for v in feats.values()] == [(2, 768, 4, 6), (2, 1024, 2, 3)]
    ref = RF.cpfpn_ref(neck, list(feats.values()))
    m.to(dev)
    neck.to(dev)
    outs = neck(list(m(x.to(dev)).values()))
    errs = [((o.cpu().double() - r).abs().max() / r.abs().max()).item() for o, r in zip(outs, ref)]
    parity_log.append("img backbone -> neck V-99-eSE 64x96: " + " ".join(f"{e:.2e}" for e in errs) +
                      f" (bound {BACKBONE_BOUND:.1e})")
    assert len(outs) == len(ref) == 2 and max(errs) <= BACKBONE_BOUND
    m.check_input_range()
    neck.check_input_range()
