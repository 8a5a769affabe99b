"""The dense BEV backbone / neck kernels (csrc/bev.hip) and SECOND / SECONDFPN on the device against the
float64 oracle on torch's CPU ops (tests/_bev_ref.py).  B = 2 throughout, so batch strides show.

Tile geometry the map sizes are picked from: cmt_bev_conv3x3 works on 64 output rows per workgroup, 32 per
wave; cmt_bev_deblock on 32 input pixels per workgroup."""
import functools

import pytest
import torch

import _bev_ref as R

pytestmark = pytest.mark.gpu

B, EPS = 2, 1e-3
# whole pipeline: max abs error over the oracle's max abs value.  The hard condition is the project's 1e-3
# (north_star); the bound is 4 x the largest value measured on an MI355X with the committed seeds
# (profiles/bev_backbone.txt: 7.33e-7 / 7.39e-7 for the two pipelines, 9.71e-7 / 5.80e-7 after their reseed,
# 9.13e-7 for the chain from the sparse encoder), which covers box-to-box differences in fp32 summation order
# only.
PIPELINE_MEASURED = 9.71e-7
PIPELINE_BOUND = min(4 * PIPELINE_MEASURED, 1e-3)


def _NB():
    from projects.mmdet3d_plugin import native_bev
    return native_bev


def _tol(ref):
    """the project's pair bound (tests/test_gpu_split.py _tol): three f16 passes, <= ~2^-21 per product"""
    return 3e-6 * ref.abs().max().item() + 1e-6


def _conv_operands(cin, cout, H, W, seed):
    g = torch.Generator().manual_seed(seed * 1000 + cin + 7 * H + W)
    xp = R.pair(R.rows_of(torch.randn(B, cin, H, W, generator=g)))            # N(0, 1) split to pairs
    w = torch.randn(cout, cin, 3, 3, generator=g) / (9 * cin) ** 0.5
    return xp, w, R.random_bn(cout, g)


# ---- 1. the strided conv alone -------------------------------------------------------------------------------

# 7x9 / 8x10: odd and even extents (both padding forms); 1x5, 5x1: one output row / column; 23x37: several
# tiles, rows that straddle map rows and the batch boundary; 1x5 is also below one tile (6 output rows);
# 15x16 -> 2 x 8 x 8 = 128 rows, exactly two tiles; 5x21 -> 2 x 3 x 11 = 66 rows, one tile plus 2 rows (less
# than a wave's 32)
CONV_MAPS = [(7, 9), (8, 10), (1, 5), (5, 1), (23, 37), (15, 16), (5, 21)]


@pytest.mark.parametrize("hw", CONV_MAPS, ids=lambda hw: f"{hw[0]}x{hw[1]}")
@pytest.mark.parametrize("cin,cout", [(32, 128), (64, 256)])
def test_strided_conv(dev, parity_log, cin, cout, hw):
    NB = _NB()
    H, W = hw
    xp, w, bn = _conv_operands(cin, cout, H, W, seed=1)
    wp, shift = NB.pack_conv3x3(w, list(bn) + [EPS])
    Ho, Wo = NB.out_hw(H, W, 2)
    M = B * Ho * Wo
    want = R.rows_of(R.conv_bn_relu(R.nchw_of(R.unpair(xp), B, H, W), w, bn, EPS, 2))
    assert tuple(want.shape) == (M, cout)
    sentinel = 0x7BCD
    out = torch.full((M + 5, 2, cout), sentinel, dtype=torch.int16, device=dev).view(torch.uint16)
    flag = torch.zeros(1, dtype=torch.int32, device=dev)
    got = NB.conv3x3(xp.to(dev), wp.to(dev), shift.to(dev), B=B, H=H, W=W, Cin=cin, Cout=cout, stride=2, out=out,
                     range_flag=flag)
    assert got is out
    assert (out[M:].cpu().view(torch.int16) == sentinel).all(), "the conv wrote beyond its rows"
    err = (R.unpair(out[:M]) - want).abs().max().item()
    bound = _tol(want) + 2.0 ** -21 * want.abs().max().item()
    parity_log.append(f"bev conv3x3 s2 {cin}->{cout} {H}x{W}: {err:.2e} (bound {bound:.2e})")
    assert err <= bound
    assert (R.unpair(out[:M]) >= 0).all() and int(flag.item()) == 0


# ---- 2. the deblock alone ------------------------------------------------------------------------------------

# 5x7: 70 pixels, two 32-pixel tiles and a tail of 6; 9x13: 234 pixels, runs that end inside a tile
@pytest.mark.parametrize("hw", [(5, 7), (9, 13)], ids=lambda hw: f"{hw[0]}x{hw[1]}")
@pytest.mark.parametrize("c0", [0, 128])
@pytest.mark.parametrize("cin,cout", [(32, 128), (64, 256)])
@pytest.mark.parametrize("k,transposed", [(1, True), (1, False), (2, True), (4, True)])
def test_deblock(dev, parity_log, k, transposed, cin, cout, c0, hw):
    NB = _NB()
    H, W = hw
    g = torch.Generator().manual_seed(2000 + 10 * k + cin + H)
    xp = R.pair(R.rows_of(torch.randn(B, cin, H, W, generator=g)))
    w = torch.randn((cin, cout, k, k) if transposed else (cout, cin, 1, 1), generator=g) / cin ** 0.5
    bn = R.random_bn(cout, g)
    wp, shift = NB.pack_deblock(w, list(bn) + [EPS], k, transposed=transposed)
    want = R.deblock_bn_relu(R.nchw_of(R.unpair(xp), B, H, W), w, bn, EPS, k, transposed=transposed)
    ctot = cout + 128
    sentinel = -12345.678
    out = torch.full((B, ctot, k * H, k * W), sentinel, dtype=torch.float32, device=dev)
    NB.deblock(xp.to(dev), wp.to(dev), shift.to(dev), out, B=B, H=H, W=W, Cin=cin, Cout=cout, k=k, c0=c0)
    got = out.cpu()
    outside = torch.ones(ctot, dtype=torch.bool)
    outside[c0:c0 + cout] = False
    assert torch.equal(got[:, outside], torch.full_like(got[:, outside], sentinel)), "wrote outside its slice"
    err = (got[:, c0:c0 + cout].double() - want).abs().max().item()
    parity_log.append(f"bev deblock k{k}{'' if transposed else ' conv1x1'} {cin}->{cout} c0 {c0} {H}x{W}: {err:.2e} "
                      f"(bound {_tol(want):.2e})")
    assert err <= _tol(want)


# ---- 3. stride 1: the new kernel and the cmt_gemm pair-row path, each against the oracle -----------------------

def test_stride1_both_paths(dev, parity_log):
    NB = _NB()
    cin, cout, H, W = 64, 128, 11, 13
    xp, w, bn = _conv_operands(cin, cout, H, W, seed=3)
    wp, shift = NB.pack_conv3x3(w, list(bn) + [EPS])
    want = R.rows_of(R.conv_bn_relu(R.nchw_of(R.unpair(xp), B, H, W), w, bn, EPS, 1))
    bound = _tol(want) + 2.0 ** -21 * want.abs().max().item()
    args = (xp.to(dev), wp.to(dev), shift.to(dev))
    new = NB.conv3x3(*args, B=B, H=H, W=W, Cin=cin, Cout=cout, stride=1)
    old = NB.conv3x3_gemm(*args, B=B, H=H, W=W, Cin=cin, Cout=cout)
    for name, y in (("cmt_bev_conv3x3", new), ("cmt_gemm CONV3X3", old)):
        err = (R.unpair(y) - want).abs().max().item()
        parity_log.append(f"bev conv3x3 s1 via {name} {cin}->{cout} {H}x{W}: {err:.2e} (bound {bound:.2e})")
        assert err <= bound, name


# ---- 4. the whole pipeline at the smallest faithful shape ---------------------------------------------------------

BN = dict(type="BN", eps=EPS, momentum=0.01)
PIPELINES = {
    "s1-2": (dict(layer_strides=[1, 2]), dict(upsample_strides=[1, 2], use_conv_for_no_stride=True)),
    # a strided stage 0: the nchw_to_rows entry path, deconv of k = 2 and 4
    "s2-2": (dict(layer_strides=[2, 2]), dict(upsample_strides=[2, 4], use_conv_for_no_stride=True)),
}


def _pipeline(form, seed=41):
    from projects.mmdet3d_plugin import build_backbone, build_neck
    bcfg, ncfg = PIPELINES[form]
    b = build_backbone(dict(type="SECOND", in_channels=32, out_channels=[128, 128], layer_nums=[2, 2], norm_cfg=BN,
                            conv_cfg=dict(type="Conv2d", bias=False), **bcfg))
    n = build_neck(dict(type="SECONDFPN", in_channels=[128, 128], out_channels=[128, 128], norm_cfg=BN,
                        upsample_cfg=dict(type="deconv", bias=False), **ncfg))
    return R.seed_module(b, seed).eval(), R.seed_module(n, seed + 1).eval()


@functools.lru_cache(maxsize=None)
def _pipeline_input():
    return torch.randn(B, 32, 20, 28, generator=torch.Generator().manual_seed(40))


def _oracle(b, n, x):
    return R.fpn_ref(n, R.second_ref(b, x))


def _rel_err(got, want):
    top = want.abs().max().item()
    assert top > 0.1
    return (got.cpu().double() - want).abs().max().item() / top


@pytest.mark.parametrize("form", list(PIPELINES))
def test_pipeline(dev, parity_log, form):
    b, n = _pipeline(form)
    x = _pipeline_input()
    want = _oracle(b, n, x)
    b.to(dev), n.to(dev)
    with torch.no_grad():
        feats = b(x.to(dev))
        got = n(feats)[0]
        again = n(b(x.to(dev)))[0]
    s = 1 if form == "s1-2" else 2
    assert [f.shape for f in feats] == [(B, 128, 20 // s, 28 // s), (B, 128, 10 // s, 14 // s)]
    assert tuple(got.shape) == (B, 256, 20, 28) == tuple(want.shape)
    assert got.dtype == torch.float32 and got.is_contiguous() and got.device.type == "cuda"
    assert torch.equal(got, again), "two runs differ"
    err = _rel_err(got, want)
    parity_log.append(f"SECOND + SECONDFPN {form}: max abs err / max abs {err:.2e} (bound {PIPELINE_BOUND:.1e})")
    print(f"SECOND + SECONDFPN {form}: relative error {err:.3e}")
    assert err <= PIPELINE_BOUND
    # the row maps un-pair to the stage outputs (off the hot path), and the neck takes plain NCHW tensors too
    stage = R.second_ref(b, x)
    assert _rel_err(feats[1].nchw(), stage[1]) <= PIPELINE_BOUND
    with torch.no_grad():
        from_nchw = n([f.nchw() for f in feats])[0]
    assert _rel_err(from_nchw, want) <= PIPELINE_BOUND
    b.check_input_range(), n.check_input_range()

    # an in-place reseed of one conv weight and one BN running_var: the packs follow
    with torch.no_grad():
        g = torch.Generator().manual_seed(43)
        w = b.blocks[1][3].weight
        w.copy_((torch.randn(w.shape, generator=g) / (9 * 128) ** 0.5).to(dev))
        v = n.deblocks[1][1].running_var
        v.copy_((0.5 + 1.5 * torch.rand(v.shape, generator=g)).to(dev))
        got2 = n(b(x.to(dev)))[0]
    assert not torch.equal(got2, got)
    want2 = _oracle(b, n, x)
    assert (want2 - want).abs().max().item() > 1e-2
    err2 = _rel_err(got2, want2)
    parity_log.append(f"SECOND + SECONDFPN {form} after a reseed: {err2:.2e}")
    assert err2 <= PIPELINE_BOUND


# ---- 5. voxels to the head's input ---------------------------------------------------------------------------------

def _voxels(seed=53):
    """a few hundred voxels in shuffled order, clustered like LiDAR surfaces, in both samples"""
    g = torch.Generator().manual_seed(seed)
    centres = torch.stack([torch.randint(0, B, (40,), generator=g), torch.randint(2, 39, (40,), generator=g),
                           torch.randint(2, 30, (40,), generator=g), torch.randint(2, 30, (40,), generator=g)], 1)
    near = centres.repeat_interleave(12, 0)
    near[:, 1:] += torch.randint(-2, 3, (near.shape[0], 3), generator=g)
    coors = torch.unique(near, dim=0)
    coors = coors[torch.randperm(coors.shape[0], generator=g)].to(torch.int32).contiguous()
    return torch.randn(coors.shape[0], 5, generator=g), coors


def test_chain_from_the_sparse_encoder(dev, parity_log):
    import _sparse_ref as SR
    from projects.mmdet3d_plugin import build_backbone, build_middle_encoder, build_neck
    enc = SR.seed_encoder(build_middle_encoder(dict(SR.REF_ENCODER_CFG, sparse_shape=[41, 32, 32],
                                                    capacity_factor=8.0)), 11).eval().to(dev)
    b = build_backbone(dict(type="SECOND", in_channels=256, out_channels=[128, 256], layer_nums=[5, 5],
                            layer_strides=[1, 2], norm_cfg=BN, conv_cfg=dict(type="Conv2d", bias=False)))
    n = build_neck(dict(type="SECONDFPN", in_channels=[128, 256], out_channels=[256, 256], upsample_strides=[1, 2],
                        norm_cfg=BN, upsample_cfg=dict(type="deconv", bias=False), use_conv_for_no_stride=True))
    R.seed_module(b, 51).eval(), R.seed_module(n, 52).eval()
    feats, coors = _voxels()
    with torch.no_grad():
        bev = enc(feats.to(dev), coors.to(dev), B)
    assert tuple(bev.shape) == (B, 256, 4, 4)
    want = _oracle(b, n, bev.cpu())
    b.to(dev), n.to(dev)
    with torch.no_grad():
        out = n(b(bev))
    assert isinstance(out, list) and len(out) == 1
    got = out[0]
    # the head's input contract
    assert tuple(got.shape) == (B, 512, 4, 4) and got.dtype == torch.float32 and got.is_contiguous()
    err = _rel_err(got, want)
    parity_log.append(f"SparseEncoder -> SECOND -> SECONDFPN: max abs err / max abs {err:.2e} "
                      f"(bound {PIPELINE_BOUND:.1e})")
    print(f"SparseEncoder -> SECOND -> SECONDFPN: relative error {err:.3e}")
    assert err <= PIPELINE_BOUND
    b.check_input_range(), n.check_input_range()          # a clean run does not raise
    bad = bev.clone()
    bad[1, 17, 2, 3] = 7e4
    with torch.no_grad():
        n(b(bad))
    with pytest.raises(ValueError, match="f16 operand range"):
        b.check_input_range()
    b.check_input_range()                                 # cleared by the raise
