"""The native sparse convolution (csrc/sparse.hip) and SparseEncoder on the device against the float64
restatement on dense conv3d (tests/_sparse_ref.py).

The grid is non-cubic, (9, 16, 24) with B = 2, so an axis swap shows.  Active sets (_sparse_ref.active_set)
are a seeded random set plus one dense 3x3x3 clump, all eight corners and a run along each face, in
shuffled row order as the voxelizer gives it; far-apart clumps leave whole 32-row tiles without a neighbour
at some taps, which is the skipped-tap path of the kernel."""
import math

import pytest
import torch

import _sparse_ref as R

pytestmark = pytest.mark.gpu

SHAPE, B = (9, 16, 24), 2
GRID = (B,) + SHAPE
FORMS = {"subm": None, **R.DOWN_FORMS}
# whole encoder: max abs error over the output's max abs value.  The hard condition is the project's 1e-3
# (north_star); the bound is 4 x the value measured on an MI355X with seed 11 (profiles/sparse_encoder.txt).
ENCODER_MEASURED = 1.464e-5
ENCODER_BOUND = min(4 * ENCODER_MEASURED, 1e-3)


def _S():
    from projects.mmdet3d_plugin import native_sparse
    return native_sparse


def _count(n, dev):
    return torch.full((1,), n, dtype=torch.int32, device=dev)


def _rulebook(form, coors_d, dev, cap=None):
    """-> (out_coors, out_count, nbr) on the device; for subm the outputs are the inputs"""
    S = _S()
    n = coors_d.shape[0]
    cnt = _count(n, dev)
    index = S.build_index(coors_d, cnt, GRID)
    if form == "subm":
        return coors_d, cnt, S.rulebook_subm(coors_d, cnt, index, GRID)
    k, s, p = R.DOWN_FORMS[form]
    oc, ocnt, nbr, _, og = S.rulebook_down(coors_d, cnt, index, GRID, k, s, p, cap if cap is not None else 8 * n)
    assert og == (B,) + R.out_shape(SHAPE, k, s, p)
    return oc, ocnt, nbr


def _ref_outputs(form, coors):
    """restatement: the output coordinates (ascending) of a strided form"""
    k, s, p = R.DOWN_FORMS[form]
    _, mask = R.densify(torch.zeros(coors.shape[0], 1), coors, GRID)
    return R.mask_coors(R.down_mask(mask, k, s, p))


# ---- 1. rulebooks, integer-exact ---------------------------------------------------------------------------

@pytest.mark.parametrize("n", [1, 63, 64, 65, 300])
def test_rulebook_subm_exact(dev, n):
    full = R.active_set(SHAPE, B)
    assert full.shape[0] >= 300
    coors = full[:n]
    _, _, nbr = _rulebook("subm", coors.to(dev), dev)
    ref = R.nbr_subm(coors)
    assert nbr.shape == ref.shape == (n, 27)
    assert torch.equal(nbr.cpu(), ref)
    assert torch.equal(nbr[:, 13].cpu(), torch.arange(n, dtype=torch.int32))   # the centre tap is the row itself


@pytest.mark.parametrize("form", list(R.DOWN_FORMS))
@pytest.mark.parametrize("n", [1, 63, 64, 65, 300])
def test_rulebook_down_exact(dev, form, n):
    coors = R.active_set(SHAPE, B)[:n]
    want = _ref_outputs(form, coors)
    m = want.shape[0]
    oc, ocnt, nbr = _rulebook(form, coors.to(dev), dev, cap=m)     # capacity exactly the true count
    assert int(ocnt.item()) == m
    assert torch.equal(oc.cpu(), want)                               # ascending, = the mask's nonzeros
    k, s, p = R.DOWN_FORMS[form]
    assert torch.equal(nbr.cpu(), R.nbr_down(coors, want, k, s, p))
    assert (nbr >= 0).any(dim=1).all()                               # active iff an input lies in the window
    if m > 1:
        _, short, _ = _rulebook(form, coors.to(dev), dev, cap=m - 1)
        assert int(short.item()) == -1                               # one short: gives up, as the voxelizer does


@pytest.mark.parametrize("form", list(FORMS))
def test_rulebook_with_an_empty_sample(dev, form):
    coors = R.active_set(SHAPE, B, only_sample=1)[:200]
    assert (coors[:, 0] == 1).all()
    oc, ocnt, nbr = _rulebook(form, coors.to(dev), dev)
    if form == "subm":
        assert torch.equal(nbr.cpu(), R.nbr_subm(coors))
        return
    want = _ref_outputs(form, coors)
    m = int(ocnt.item())
    assert m == want.shape[0] and torch.equal(oc[:m].cpu(), want)
    k, s, p = R.DOWN_FORMS[form]
    assert torch.equal(nbr[:m].cpu(), R.nbr_down(coors, want, k, s, p))
    assert (nbr[m:] == -1).all()


# ---- 2. one convolution against float64 ---------------------------------------------------------------------

def _conv_case(form, cin, cout, seed=1):
    """seeded unit-variance operands and the float64 pre-epilogue result at the output rows"""
    g = torch.Generator().manual_seed(seed * 1000 + cin * 7 + cout)
    coors = R.active_set(SHAPE, B)[:300]
    x = torch.randn(300, cin, generator=g)
    if form == "subm":
        w = torch.randn(cout, 3, 3, 3, cin, generator=g)
        oc = coors
    else:
        k, s, p = R.DOWN_FORMS[form]
        w = torch.randn((cout,) + R.triple(k) + (cin,), generator=g)
        oc = _ref_outputs(form, coors)
    xd, mask = R.densify(x, coors, GRID)
    k, s, p = (3, 1, 1) if form == "subm" else R.DOWN_FORMS[form]
    yd, _ = R.conv_dense(xd, mask, w, subm=form == "subm", stride=s, padding=p, relu=False)
    pre = R.rows_of(yd, oc)
    scale = 0.5 + torch.rand(cout, generator=g)
    shift = torch.randn(cout, generator=g)
    res = torch.randn(oc.shape[0], cout, generator=g)
    return coors, x, w, oc, pre, scale, shift, res


@pytest.mark.parametrize("form", list(FORMS))
@pytest.mark.parametrize("cin,cout", [(5, 16), (16, 16), (32, 64), (128, 128)])
def test_conv_against_float64(dev, parity_log, form, cin, cout):
    S = _S()
    coors, x, w, oc, pre, scale, shift, res = _conv_case(form, cin, cout)
    K = w.shape[1] * w.shape[2] * w.shape[3]
    # bf16x3: ~2^-16 relative per product, as test_gemm_ex_transposes bounds it
    bound = 2.0 ** -15 * math.sqrt(K * cin) * 4 * scale.max().item()
    ocd, ocnt, nbr = _rulebook(form, coors.to(dev), dev)
    m = int(ocnt.item())
    assert m == oc.shape[0] and torch.equal(ocd[:m].cpu(), oc)
    xd, wp = x.to(dev), S.pack_weight(w.to(dev))
    sc, sh, rs = scale.to(dev), shift.to(dev), torch.zeros(nbr.shape[0], cout, device=dev)
    rs[:m] = res.to(dev)
    worst = 0.0
    for with_res, relu in ((False, False), (True, True), (False, True), (True, False)):
        want = pre * scale.double() + shift.double()
        if with_res:
            want = want + res.double()
        if relu:
            want = torch.relu(want)
        got = S.conv(xd, nbr, ocnt, wp, sc, sh, Cin=cin, Cout=cout, relu=relu, R=rs if with_res else None)[:m]
        err = (got.cpu().double() - want).abs().max().item()
        worst = max(worst, err)
        assert err <= bound, (form, cin, cout, with_res, relu, err, bound)
    # fp32 exponent range: inputs scaled by 2^-30 keep the relative accuracy (no shift, no residual)
    zero = torch.zeros(cout, device=dev)
    got = S.conv(xd * 2.0 ** -30, nbr, ocnt, wp, sc, zero, Cin=cin, Cout=cout, relu=False)[:m]
    err = ((got.cpu().double() * 2.0 ** 30) - pre * scale.double()).abs().max().item()
    assert err <= bound, (form, cin, cout, "2^-30", err, bound)
    parity_log.append(f"sparse conv {form} {cin}->{cout}: max abs err {max(worst, err):.2e} (bound {bound:.2e})")


# ---- 3. determinism, bitwise --------------------------------------------------------------------------------

@pytest.mark.parametrize("form", ["subm", "k3s2p1"])
def test_conv_bitwise_determinism(dev, form):
    S = _S()
    coors, x, w, oc, _, scale, shift, _ = _conv_case(form, 32, 64, seed=2)
    wp, sc, sh = S.pack_weight(w.to(dev)), scale.to(dev), shift.to(dev)

    def run(c, f):
        ocd, ocnt, nbr = _rulebook(form, c.to(dev), dev)
        y = S.conv(f.to(dev), nbr, ocnt, wp, sc, sh, Cin=32, Cout=64, relu=True)
        m = int(ocnt.item())
        return ocd[:m].cpu(), y[:m].cpu()

    c1, y1 = run(coors, x)
    c2, y2 = run(coors, x)
    assert torch.equal(y1.view(torch.int32), y2.view(torch.int32))              # the same call twice
    perm = torch.randperm(300, generator=torch.Generator().manual_seed(9))
    c3, y3 = run(coors[perm].contiguous(), x[perm].contiguous())
    if form == "subm":                                                          # identically permuted output
        assert torch.equal(y3.view(torch.int32), y1[perm].view(torch.int32))
    else:                                                                       # identical output
        assert torch.equal(c3, c1) and torch.equal(y3.view(torch.int32), y1.view(torch.int32))


# ---- 4. densify ---------------------------------------------------------------------------------------------

@pytest.mark.parametrize("grid,C", [(GRID, 5), ((2, 2, 5, 7), 3)])
def test_to_dense_exact(dev, grid, C):
    S = _S()
    coors = R.active_set(tuple(grid[1:]), grid[0], n_random=40)
    g = torch.Generator().manual_seed(6)
    x = torch.randn(coors.shape[0], C, generator=g)
    got = S.to_dense(x.to(dev), coors.to(dev), _count(coors.shape[0], dev), grid, C).cpu()
    dense, _ = R.densify(x, coors, grid)
    want = dense.float().reshape(grid[0], C * grid[1], grid[2], grid[3])        # [B, C, D, H, W] viewed
    assert got.shape == want.shape and torch.equal(got, want)                   # zeros included
    b, z, y, xx = coors[0].tolist()
    assert got[b, 1 * grid[1] + z, y, xx] == x[0, 1]                            # channel-major, then depth


# ---- 5. the whole encoder -----------------------------------------------------------------------------------

ENC_SHAPE = (41, 32, 32)


def _encoder(seed=11):
    from projects.mmdet3d_plugin import build_middle_encoder
    enc = build_middle_encoder(dict(R.REF_ENCODER_CFG, sparse_shape=list(ENC_SHAPE), capacity_factor=8.0))
    return R.seed_encoder(enc, seed).eval()


def _check_encoder(enc, feats, coors, dev, parity_log, what, partly_inactive=False):
    want, mask = R.encoder_dense(enc, feats, coors, 2)
    assert tuple(want.shape) == (2, 256, 4, 4) and mask.sum() > 0
    assert not partly_inactive or mask.sum() < mask.numel()
    enc.to(dev)
    with torch.no_grad():
        got = enc(feats.to(dev), coors.to(dev), 2).cpu()
    enc.cpu()
    assert tuple(got.shape) == (2, 256, 4, 4) and got.dtype == torch.float32
    # the active pattern, per site: inactive sites are exactly 0 in every channel, active ones are not (ReLU
    # zeroes single channels, never all 128 of these seeded sites)
    site = (got.reshape(2, 128, 2, 4, 4) != 0).any(dim=1, keepdim=True)
    assert torch.equal(site, mask > 0)
    assert torch.equal((want.reshape(2, 128, 2, 4, 4) != 0).any(dim=1, keepdim=True), mask > 0)
    top = want.abs().max().item()
    assert top > 0.1
    err = (got.double() - want).abs().max().item() / top
    parity_log.append(f"SparseEncoder {what}: max abs err / max abs {err:.2e} (bound {ENCODER_BOUND:.1e}), "
                      f"output max {top:.3f}, active {int(mask.sum())} of {mask.numel()} sites")
    print(f"SparseEncoder {what}: relative error {err:.3e}, output max {top:.4f}")
    assert err <= ENCODER_BOUND


def _encoder_voxels(seed=11):
    """~400 voxels in shuffled order: clusters (LiDAR-like surfaces) in one half of the y range plus a few
    isolated sites, so part of the 4 x 4 output map stays inactive"""
    g = torch.Generator().manual_seed(seed)
    centres = torch.stack([torch.randint(0, 2, (32,), generator=g), torch.randint(2, 39, (32,), generator=g),
                           torch.randint(2, 13, (32,), generator=g), torch.randint(2, 30, (32,), generator=g)], 1)
    near = centres.repeat_interleave(14, 0)
    near[:, 1:] += torch.randint(-2, 3, (near.shape[0], 3), generator=g)
    lone = torch.stack([torch.zeros(6, dtype=torch.int64), torch.randint(0, 41, (6,), generator=g),
                        torch.randint(0, 32, (6,), generator=g), torch.randint(0, 32, (6,), generator=g)], 1)
    coors = torch.unique(torch.cat([near, lone]), dim=0)
    coors = coors[torch.randperm(coors.shape[0], generator=g)].to(torch.int32).contiguous()
    return torch.randn(coors.shape[0], 5, generator=g), coors


def test_encoder_against_float64(dev, parity_log):
    feats, coors = _encoder_voxels()
    assert 300 <= coors.shape[0] <= 500
    _check_encoder(_encoder(), feats, coors, dev, parity_log, f"{coors.shape[0]} voxels", partly_inactive=True)


def test_encoder_after_the_voxelizer(dev, parity_log):
    """voxelize_batch -> SparseEncoder: the voxelizer's real (first-appearance) row order"""
    from projects.mmdet3d_plugin.mmcv_custom.ops.voxel import SPConvVoxelization, voxelize_batch
    layer = SPConvVoxelization(voxel_size=[0.075, 0.075, 0.2], point_cloud_range=[-1.2, -1.2, -5.0, 1.2, 1.2, 3.0],
                               max_num_points=10, max_voxels=(4000, 4000), num_point_features=5).eval()
    assert layer.grid_size.tolist() == [32, 32, 40]
    g = torch.Generator().manual_seed(12)
    clouds = []
    for _ in range(2):   # ~1500 points per sample on a few slanted planes
        xy = torch.rand(1500, 2, generator=g) * 2.4 - 1.2
        plane = torch.randint(0, 3, (1500,), generator=g).float()
        z = -4.0 + 2.5 * plane + 0.4 * xy[:, 0] + 0.05 * torch.randn(1500, generator=g)
        clouds.append(torch.cat([xy, z[:, None], torch.rand(1500, 2, generator=g)], 1).contiguous())
    feats, _, coors = voxelize_batch(layer, [c.to(dev) for c in clouds])
    assert coors.shape[1] == 4 and coors.shape[0] > 500
    _check_encoder(_encoder(), feats.cpu(), coors.cpu(), dev, parity_log, f"{coors.shape[0]} voxels of 3000 points")


def test_encoder_capacity_overflow_is_reported(dev):
    from projects.mmdet3d_plugin import build_middle_encoder
    enc = build_middle_encoder(dict(R.REF_ENCODER_CFG, sparse_shape=list(ENC_SHAPE))).eval().to(dev)
    # isolated sites at odd coordinates: the padding-1 strided stage makes several outputs of each
    coors = torch.tensor([[0, 5, 5, 5], [0, 11, 21, 9], [1, 21, 7, 27], [1, 31, 25, 13]], dtype=torch.int32)
    with torch.no_grad(), pytest.raises(RuntimeError, match="capacity_factor"):
        enc(torch.ones(4, 5).to(dev), coors.to(dev), 2)


# ---- 6. the full-size grid -----------------------------------------------------------------------------------

def test_full_grid_index(dev):
    """(41, 1440, 1440): 85 M sites, the far corner included -- 32-bit site numbers and the index's size.
    conv_input alone, against the restatement evaluated only at the active sites and their neighbours."""
    S = _S()
    grid = (1, 41, 1440, 1440)
    g = torch.Generator().manual_seed(13)
    centres = torch.stack([torch.zeros(400, dtype=torch.int64), torch.randint(0, 41, (400,), generator=g),
                           torch.randint(0, 1440, (400,), generator=g), torch.randint(0, 1440, (400,), generator=g)], 1)
    centres[0] = torch.tensor([0, 40, 1439, 1439])
    centres[1] = torch.tensor([0, 0, 0, 0])
    near = centres.repeat_interleave(8, 0)
    near[:, 1:] += torch.randint(-1, 2, (near.shape[0], 3), generator=g)
    near[:, 1].clamp_(0, 40)
    near[:, 2:].clamp_(0, 1439)
    coors = torch.unique(torch.cat([centres, near]), dim=0)[:2000]
    coors = torch.cat([coors, torch.tensor([[0, 40, 1439, 1439]])])
    coors = torch.unique(coors, dim=0)
    coors = coors[torch.randperm(coors.shape[0], generator=g)].to(torch.int32).contiguous()
    n = coors.shape[0]
    assert 1500 <= n <= 2001 and (coors == torch.tensor([0, 40, 1439, 1439], dtype=torch.int32)).all(1).any()
    x = torch.randn(n, 5, generator=g)
    w = torch.randn(16, 3, 3, 3, 5, generator=g)
    scale, shift = 0.5 + torch.rand(16, generator=g), torch.randn(16, generator=g)
    cd, cnt = coors.to(dev), _count(n, dev)
    index = S.build_index(cd, cnt, grid)
    nbr = S.rulebook_subm(cd, cnt, index, grid)
    ref_nbr = R.nbr_subm(coors)
    assert torch.equal(nbr.cpu(), ref_nbr)
    assert (ref_nbr >= 0).sum().item() > 2 * n                   # the clusters do have neighbours
    got = S.conv(x.to(dev), nbr, cnt, S.pack_weight(w.to(dev)), scale.to(dev), shift.to(dev), Cin=5, Cout=16)
    want = R.conv_rows(x, ref_nbr, w, scale, shift)
    bound = 2.0 ** -15 * math.sqrt(27 * 5) * 4 * scale.max().item()
    assert (got.cpu().double() - want).abs().max().item() <= bound
