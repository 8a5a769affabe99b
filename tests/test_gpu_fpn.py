"""The camera neck kernels (csrc/fpn.hip) and CPFPN on the device against the float64 oracle on torch's CPU
ops (tests/_fpn_ref.py).  B = 2 throughout, so batch strides show.

Tile geometry the map sizes are picked from: cmt_fpn_lateral works on 128 pixels of one image per workgroup,
32 per wave, and 128 output channels per workgroup; cmt_rows_to_nchw on 64 pixels x 64 channels, with
16-byte stores where H*W % 4 == 0 and 4-byte stores otherwise."""
import functools

import pytest
import torch

import _fpn_ref as R

pytestmark = pytest.mark.gpu

B, EPS = 2, 1e-3
# whole neck: max abs error over the oracle's max abs value, per output.  The hard condition is the project's
# 1e-3 (north_star); the bound is 4 x the largest value measured on an MI355X with the committed seeds
# (profiles/img_neck.txt: 9.91e-7 for the three-level neck's outs[0]; 6.2e-7 ... 9.6e-7 for the other forms'
# outs[0], 9.1e-8 ... 2.6e-7 for the laterals that leave as they are, 7.2e-7 after the reseed), which covers
# box-to-box differences in fp32 summation order only.
NECK_MEASURED = 9.91e-7
NECK_BOUND = min(4 * NECK_MEASURED, 1e-3)


def _NF():
    from projects.mmdet3d_plugin import native_fpn
    return native_fpn


def _bound(ref):
    """the project's pair bound (tests/test_gpu_bev.py): three f16 passes, <= ~2^-21 per product, plus the
    split of the output"""
    top = ref.abs().max().item()
    return 3e-6 * top + 1e-6 + 2.0 ** -21 * top


# (Cin, Cout, form, relu): both channel forms, both widths (one and two 128-channel groups), the bias and the
# BN form, ReLU on and off
VARIANTS = [(32, 128, "bias", False), (80, 256, "bn", True), (80, 128, "bn", False), (32, 256, "bias", True)]
VARIANT_IDS = [f"{ci}-{co}-{f}{'-relu' if r else ''}" for ci, co, f, r in VARIANTS]


def _lateral_operands(cin, cout, form, H, W, seed):
    g = torch.Generator().manual_seed(seed * 1000 + cin + 7 * H + W)
    x = torch.randn(B, cin, H, W, generator=g)
    w = torch.randn(cout, cin, 1, 1, generator=g) / cin ** 0.5
    bias = 0.5 * torch.randn(cout, generator=g) if form == "bias" else None
    bn = R.random_bn(cout, g) if form == "bn" else None
    return g, x, w, bias, bn


def _run_lateral(dev, x, w, bias, bn, cout, relu, top=None, top_hw=None, flag=None):
    """-> (the rows the kernel wrote, the whole buffer with its 5 sentinel rows)"""
    NF = _NF()
    wp, shift = NF.pack_conv1x1(w, list(bn) + [EPS] if bn is not None else bias)
    M = x.shape[0] * x.shape[2] * x.shape[3]
    sentinel = 0x7BCD
    out = torch.full((M + 5, 2, cout), sentinel, dtype=torch.int16, device=dev).view(torch.uint16)
    got = NF.lateral(x.to(dev), wp.to(dev), shift.to(dev), Cout=cout, top=None if top is None else top.to(dev),
                     top_hw=top_hw, relu=relu, out=out, range_flag=flag)
    assert got is out
    assert (out[M:].cpu().view(torch.int16) == sentinel).all(), "the lateral wrote beyond its rows"
    return out[:M]


# ---- 1. the lateral alone, no top-down term ------------------------------------------------------------------

# 1x5: below one wave; 5x7 (35) and 9x13 (117): tails that no 32-pixel wave tile divides (two and four waves
# at work, the last with 3 and 21 pixels); 8x16: exactly 128 pixels per image, one full workgroup tile each;
# 11x25 (275): three workgroup tiles per image, the last with 19 pixels and three waves without any
PLAIN_MAPS = [(1, 5), (5, 7), (9, 13), (8, 16), (11, 25)]


@pytest.mark.parametrize("hw", PLAIN_MAPS, ids=lambda hw: f"{hw[0]}x{hw[1]}")
@pytest.mark.parametrize("cin,cout,form,relu", VARIANTS, ids=VARIANT_IDS)
def test_lateral_plain(dev, parity_log, cin, cout, form, relu, hw):
    H, W = hw
    _, x, w, bias, bn = _lateral_operands(cin, cout, form, H, W, seed=1)
    want = R.rows_of(R.lateral_ref(x, w, bias, bn, EPS, relu))
    flag = torch.zeros(1, dtype=torch.int32, device=dev)
    got = _run_lateral(dev, x, w, bias, bn, cout, relu, flag=flag)
    err = (R.unpair(got) - want).abs().max().item()
    parity_log.append(f"fpn lateral {cin}->{cout} {form}{' relu' if relu else ''} {H}x{W}: {err:.2e} "
                      f"(bound {_bound(want):.2e})")
    assert err <= _bound(want)
    assert int(flag.item()) == 0
    assert (not relu) or (R.unpair(got) >= 0).all()
    assert relu or (want < 0).any()


# ---- 2. the lateral with the coarser level's rows --------------------------------------------------------------

# (coarse, fine): exact halves; odd sizes (3 -> 5, 7 -> 13; 4 -> 7, 5 -> 9); a 1 x 1 map broadcast; equal sizes
# (the add alone); (1, 2) -> (2, 82), where the integer index rule in * dst // out is not torch's (and a second
# workgroup tile of 36 pixels); (6, 13) -> (11, 25): several workgroup tiles per image
TOP_DOWN = [((3, 5), (6, 10)), ((3, 7), (5, 13)), ((4, 5), (7, 9)), ((1, 1), (5, 7)), ((5, 7), (5, 7)),
            ((1, 2), (2, 82)), ((6, 13), (11, 25))]


@pytest.mark.parametrize("sizes", TOP_DOWN, ids=lambda s: f"{s[0][0]}x{s[0][1]}to{s[1][0]}x{s[1][1]}")
@pytest.mark.parametrize("cin,cout,form,relu", VARIANTS, ids=VARIANT_IDS)
def test_lateral_top_down(dev, parity_log, cin, cout, form, relu, sizes):
    (Ht, Wt), (H, W) = sizes
    g, x, w, bias, bn = _lateral_operands(cin, cout, form, H, W, seed=2)
    top = R.pair(R.rows_of(torch.randn(B, cout, Ht, Wt, generator=g)))
    top64 = R.nchw_of(R.unpair(top), B, Ht, Wt)      # the oracle gets the pair-rounded T and the fp32 X
    want = R.rows_of(R.lateral_ref(x, w, bias, bn, EPS, relu, top=top64))
    got = _run_lateral(dev, x, w, bias, bn, cout, relu, top=top, top_hw=(Ht, Wt))
    err = (R.unpair(got) - want).abs().max().item()
    parity_log.append(f"fpn lateral {cin}->{cout} {form}{' relu' if relu else ''} {Ht}x{Wt} -> {H}x{W}: {err:.2e} "
                      f"(bound {_bound(want):.2e})")
    assert err <= _bound(want)
    if relu:
        # ReLU acts before the add: after it, no output could be negative
        assert (want < 0).any()
        after = torch.relu(R.rows_of(R.lateral_ref(x, w, bias, bn, EPS, False, top=top64)))
        assert (after - want).abs().max().item() > 100 * _bound(want)


def test_lateral_range_flag(dev):
    H, W = 5, 7
    _, x, w, bias, bn = _lateral_operands(32, 128, "bias", H, W, seed=3)
    flag = torch.zeros(1, dtype=torch.int32, device=dev)
    _run_lateral(dev, x, w, bias, bn, 128, False, flag=flag)
    assert int(flag.item()) == 0
    bad = x.clone()
    bad[1, 17, 4, 6] = 7e4                     # the last pixel of the last image: in a tile's tail
    _run_lateral(dev, bad, w, bias, bn, 128, False, flag=flag)
    assert int(flag.item()) == 1
    flag.zero_()
    bad = x.clone()
    bad[0, 0, 0, 0] = float("nan")
    _run_lateral(dev, bad, w, bias, bn, 128, False, flag=flag)
    assert int(flag.item()) == 1
    # an input inside the range whose output is not: |w x| >= 65520 before the split
    flag.zero_()
    big = torch.full_like(x, 6e4)
    _run_lateral(dev, big, w.abs(), bias, bn, 128, False, flag=flag)
    assert int(flag.item()) == 1
    # the top-down sum leaves the range though neither term does
    flag.zero_()
    zero_w = torch.zeros_like(w)
    shift = torch.full((128,), 4e4)
    top = R.pair(torch.full((B * 2 * 3, 128), 4e4))
    _run_lateral(dev, x, zero_w, shift, None, 128, False, top=top, top_hw=(2, 3), flag=flag)
    assert int(flag.item()) == 1


# ---- 3. rows_to_nchw alone -----------------------------------------------------------------------------------------

# 1x5, 5x7, 9x13: odd pixel counts (4-byte stores), below one tile, a tail, several tiles; 6x10 and 8x16:
# H*W % 4 == 0 (16-byte stores) with a tail (60) and with exactly two tiles (128).  C = 72: a channel tile of 8.
@pytest.mark.parametrize("hw", [(1, 5), (5, 7), (9, 13), (6, 10), (8, 16)], ids=lambda hw: f"{hw[0]}x{hw[1]}")
@pytest.mark.parametrize("C", [128, 256, 72])
def test_rows_to_nchw(dev, C, hw):
    from projects.mmdet3d_plugin import native_bev as NB
    NF = _NF()
    H, W = hw
    g = torch.Generator().manual_seed(300 + C + H)
    M = B * H * W
    rows = torch.cat([R.pair(4.0 * torch.randn(M, C, generator=g)).view(torch.int16),
                      torch.full((3, 2, C), 0x7BCD, dtype=torch.int16)]).view(torch.uint16).to(dev)   # + 3 rows beyond
    want = NB.RowMap(rows, (B, C, H, W)).nchw()
    got = NF.rows_to_nchw(rows, (B, C, H, W))
    assert got.dtype == torch.float32 and got.is_contiguous() and tuple(got.shape) == (B, C, H, W)
    assert torch.equal(got, want)
    assert torch.equal(got.cpu().double(), R.nchw_of(R.unpair(rows[:M]), B, H, W))   # hi + lo is exact in fp32 here
    out = torch.full((B, C, H, W), -1.0, device=dev)
    assert NF.rows_to_nchw(rows, (B, C, H, W), out=out) is out and torch.equal(out, want)


# ---- 4. the module ---------------------------------------------------------------------------------------------------

BN = dict(type="BN", eps=EPS, momentum=0.01)
NECKS = {
    "two-6x10": (dict(in_channels=[48, 80], out_channels=128, num_outs=2), [(6, 10), (3, 5)]),
    "two-5x13": (dict(in_channels=[48, 80], out_channels=128, num_outs=2), [(5, 13), (3, 7)]),
    "three": (dict(in_channels=[32, 48, 64], out_channels=128, num_outs=3), [(9, 13), (5, 7), (3, 4)]),
    "three-4outs": (dict(in_channels=[32, 48, 64], out_channels=128, num_outs=4), [(9, 13), (5, 7), (3, 4)]),
    "one": (dict(in_channels=[48], out_channels=128, num_outs=1), [(5, 13)]),
    "bn-relu": (dict(in_channels=[48, 80], out_channels=128, num_outs=3, norm_cfg=BN, act_cfg=dict(type="ReLU")),
                [(6, 10), (3, 5)]),
}


def _neck(form, seed=71):
    from projects.mmdet3d_plugin import build_neck
    return R.seed_neck(build_neck(dict(NECKS[form][0], type="CPFPN")), seed).eval()


@functools.lru_cache(maxsize=None)
def _neck_inputs(form):
    g = torch.Generator().manual_seed(70)
    return tuple(torch.randn(B, c, h, w, generator=g) for c, (h, w) in zip(NECKS[form][0]["in_channels"], NECKS[form][1]))


def _rel_err(got, want):
    top = want.abs().max().item()
    assert top > 0.1
    return (got.cpu().double() - want).abs().max().item() / top


def _check_outs(outs, want, dev):
    assert isinstance(outs, tuple) and len(outs) == len(want)
    errs = []
    for o, w in zip(outs, want):
        assert tuple(o.shape) == tuple(w.shape)
        assert o.dtype == torch.float32 and o.is_contiguous() and o.device == dev
        errs.append(_rel_err(o, w))
    return errs


@pytest.mark.parametrize("form", list(NECKS))
def test_neck(dev, parity_log, form):
    n = _neck(form)
    xs = _neck_inputs(form)
    want = R.cpfpn_ref(n, xs)
    cfg, sizes = NECKS[form]
    assert len(want) == cfg["num_outs"]
    assert [tuple(w.shape[2:]) for w in want[:len(sizes)]] == sizes
    n.to(dev)
    dxs = [x.to(dev) for x in xs]
    with torch.no_grad():
        outs = n(dxs)
        again = n(dxs)
    errs = _check_outs(outs, want, dev)
    assert all(torch.equal(a, b) for a, b in zip(outs, again)), "two runs differ"
    parity_log.append(f"CPFPN {form}: max abs err / max abs per output {', '.join(f'{e:.2e}' for e in errs)} "
                      f"(bound {NECK_BOUND:.1e})")
    print(f"CPFPN {form}: relative error {max(errs):.3e}")
    assert max(errs) <= NECK_BOUND
    n.check_input_range()                                # a clean run does not raise
    # other float dtypes go through .float()
    with torch.no_grad():
        from_double = n([x.double() for x in dxs])
    assert all(torch.equal(a, b) for a, b in zip(outs, from_double))


def test_neck_packs_follow_a_reseed(dev, parity_log):
    n = _neck("two-6x10")
    xs = _neck_inputs("two-6x10")
    want = R.cpfpn_ref(n, xs)
    n.to(dev)
    dxs = [x.to(dev) for x in xs]
    with torch.no_grad():
        outs = n(dxs)
        g = torch.Generator().manual_seed(73)
        w = n.lateral_convs[1].conv.weight
        w.copy_((torch.randn(w.shape, generator=g) / 80 ** 0.5).to(dev))
        b = n.fpn_convs[0].conv.bias
        b.copy_(torch.randn(b.shape, generator=g).to(dev))
        outs2 = n(dxs)
    assert not torch.equal(outs2[0], outs[0]) and not torch.equal(outs2[1], outs[1])
    want2 = R.cpfpn_ref(n, xs)
    assert min((a - b).abs().max().item() for a, b in zip(want2, want)) > 1e-2
    errs = _check_outs(outs2, want2, dev)
    parity_log.append(f"CPFPN two-6x10 after a reseed: {', '.join(f'{e:.2e}' for e in errs)}")
    print(f"CPFPN two-6x10 after a reseed: relative error {max(errs):.3e}")
    assert max(errs) <= NECK_BOUND


def test_neck_range_flag(dev):
    n = _neck("two-6x10").to(dev)
    dxs = [x.to(dev) for x in _neck_inputs("two-6x10")]
    with torch.no_grad():
        n(dxs)
    n.check_input_range()
    bad = dxs[1].clone()
    bad[1, 17, 2, 3] = 7e4
    with torch.no_grad():
        n([dxs[0], bad])
    with pytest.raises(ValueError, match="f16 operand range"):
        n.check_input_range()
    n.check_input_range()                                 # cleared by the raise
