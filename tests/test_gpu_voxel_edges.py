"""Edges of the voxelizer (csrc/voxelize.hip: bin -> assign -> gather) against
the C restatement (oracle/voxelize_oracle.c), bit-exact: non-finite and huge
coordinates, points exactly on voxel planes, non-square grids, keys >= 2^31,
row shapes (F, nfeat_mean, max_points), one voxel holding everything, the tile
sizes of the three kernels, a voxel budget on an assign-chunk boundary, hash
probes built to wrap around the end of the LDS and the global table, a too
small workspace, and the SPConvVoxelization layer on top.

Every call is followed by a check of the workspace contract: the hash table,
the look-back words and the ticket/error words are all-ones again.

The wrapper (native.voxelize) allocates the outputs itself, so rows beyond the
voxel count cannot be pre-filled; they are unspecified and only [:M] is compared.
"""
import ctypes
import os

import numpy as np
import pytest
import torch

from conftest import ROOT

pytestmark = pytest.mark.gpu

NUS = dict(voxel_size=[0.075, 0.075, 0.2], coors_range=[-54.0, -54.0, -5.0, 54.0, 54.0, 3.0], grid=[1440, 1440, 40])
HASH_MUL = 2654435761    # hash_key() in csrc/voxelize.hip: (key * 2654435761u) & mask
P_SHARED = 4096


def _unit_geo(grid):
    """voxel size 1, range [0, grid): the quotient is the coordinate itself."""
    return dict(voxel_size=[1.0, 1.0, 1.0], coors_range=[0.0, 0.0, 0.0] + [float(g) for g in grid], grid=list(grid))


G753 = _unit_geo([7, 5, 3])
_LIB = []


def _oracle(pts, geo, max_points, max_voxels, nmean):
    if not _LIB:
        _LIB.append(ctypes.CDLL(os.path.join(ROOT, "oracle", "_build", "libvoxel_oracle.so")))
    fp, ip = ctypes.POINTER(ctypes.c_float), ctypes.POINTER(ctypes.c_int)
    pn = np.ascontiguousarray(pts, np.float32)
    n, F = pn.shape
    rv = np.zeros((max_voxels, max_points, F), np.float32)
    rc = np.zeros((max_voxels, 3), np.int32)
    rn = np.zeros((max_voxels,), np.int32)
    rm = np.zeros((max_voxels, nmean), np.float32)
    M = _LIB[0].cmt_oracle_voxelize(pn.ctypes.data_as(fp), n, F, np.array(geo["voxel_size"], np.float32).ctypes.data_as(fp),
                                    np.array(geo["coors_range"], np.float32).ctypes.data_as(fp),
                                    np.array(geo["grid"], np.int32).ctypes.data_as(ip), max_points, max_voxels, nmean,
                                    rv.ctypes.data_as(fp), rc.ctypes.data_as(ip), rn.ctypes.data_as(ip),
                                    rm.ctypes.data_as(fp))
    return M, rv[:M], rc[:M], rn[:M], rm[:M]


def _bits(a):
    """fp32 compared through the int32 view: -0.0 != 0.0 and every payload counts."""
    a = a.cpu().numpy() if isinstance(a, torch.Tensor) else a
    return np.ascontiguousarray(a, np.float32).view(np.int32)


def _same(got, ref):
    vox, coors, num, means, nvox = got
    M, rv, rc, rn, rm = ref
    assert int(nvox.item()) == M
    assert np.array_equal(coors[:M].cpu().numpy(), rc)
    assert np.array_equal(num[:M].cpu().numpy(), rn)
    assert np.array_equal(_bits(vox[:M]), _bits(rv))
    assert np.array_equal(_bits(means[:M]), _bits(rm))


def _assert_clean(ws, P):
    # Mirrors ws_layout (csrc/voxelize.hip) with cap = 2 P table slots: tkey, tfirst and thead are 3 x 4 cap =
    # 24 P bytes from offset 0; pslot, pnext and vslot (3 x 4 P = 12 P bytes, per-call scratch that stays dirty)
    # follow; the look-back words and the ticket and error words run from 36 P to the end.
    assert ws.numel() > 36 * P and ws.numel() < 72 * P
    assert bool((ws[: 24 * P] == 0xFF).all()), "hash table (tkey/tfirst/thead) not left all-ones"
    assert bool((ws[36 * P:] == 0xFF).all()), "look-back / ticket / error words not left all-ones"


def _capacity(n):
    p = 1024
    while p < n:
        p <<= 1
    return p


def _run(dev, pts, geo, ws, P, *, max_voxels, max_points=10, nmean=None):
    """One device call against the oracle, bit-exact, and the workspace left clean.  Returns the oracle's answer."""
    from projects.mmdet3d_plugin import native as N
    pts = np.array(pts, np.float32)                                    # a copy: the caller's array is only read
    nmean = pts.shape[1] if nmean is None else nmean
    got = N.voxelize(torch.from_numpy(pts).to(dev), max_points=max_points, max_voxels=max_voxels, nfeat_mean=nmean,
                     workspace=ws, **geo)
    ref = _oracle(pts, geo, max_points, max_voxels, nmean)
    _same(got, ref)
    _assert_clean(ws, P)
    return ref


@pytest.fixture(scope="module")
def ws(dev):
    from projects.mmdet3d_plugin import native as N
    return N.voxelize_workspace(P_SHARED, dev)


@pytest.fixture(scope="module")
def ws8k(dev):
    """N = 4097 needs the next capacity; shared by the tile and the budget cases."""
    from projects.mmdet3d_plugin import native as N
    return N.voxelize_workspace(8192, dev)


def _feats(rng, n, F):
    """Finite feature columns (index >= 3): only x, y, z ever carry non-finite values."""
    return rng.random((n, F - 3), dtype=np.float32) if F > 3 else np.zeros((n, 0), np.float32)


def _cloud(rng, n, geo, F=5, margin=0.0):
    lo = np.array(geo["coors_range"][:3]) - margin
    hi = np.array(geo["coors_range"][3:]) + margin
    xyz = (lo + rng.random((n, 3)) * (hi - lo)).astype(np.float32)
    return np.concatenate([xyz, _feats(rng, n, F)], 1)


def _centres(keys, geo, F=5, rng=None):
    """One point in the middle of each cell key = (z * gy + y) * gx + x; the last feature column (if any) is the
    point's index."""
    gx, gy, _ = geo["grid"]
    keys = np.asarray(keys, np.int64)
    cell = np.stack([keys % gx, (keys // gx) % gy, keys // (gx * gy)], 1)
    xyz = np.array(geo["coors_range"][:3]) + (cell + 0.5) * np.array(geo["voxel_size"])
    pts = np.zeros((len(keys), F), np.float32)
    pts[:, :3] = xyz
    if rng is not None:
        pts[:, 3:] = _feats(rng, len(keys), F)
    if F > 3:
        pts[:, F - 1] = np.arange(len(keys))
    return pts


def _keys_of(coors, geo):
    gx, gy, _ = geo["grid"]
    c = coors.astype(np.int64)
    return (c[:, 0] * gy + c[:, 1]) * gx + c[:, 2]


def _distinct_cells(rng, n, geo):
    gx, gy, gz = geo["grid"]
    keys = np.unique(rng.integers(0, gx * gy * gz, size=2 * n + 64))
    assert len(keys) >= n
    return rng.permutation(keys)[:n]


# ---------------------------------------------------------------------------------------------------------------
# 1. non-finite and huge coordinates
def test_non_finite_and_huge_coordinates_dropped(dev, ws, parity_log):
    rng = np.random.default_rng(101)
    n = 600
    pts = _cloud(rng, n, G753, margin=0.25)
    bad = np.unique(np.concatenate([[0, 255, 256, n - 1], rng.choice(n, 56, replace=False)]))
    values = [np.nan, np.inf, -np.inf, 3e9, -3e9, 1e30]
    for k, i in enumerate(bad):
        pts[i, k % 3] = values[(k // 3) % 6]
    assert len(bad) >= 56 and {0, 255, 256, n - 1} <= set(bad.tolist())
    M, rv, rc, rn, rm = _run(dev, pts, G753, ws, P_SHARED, max_voxels=200)
    # the oracle's answer holds no trace of the bad rows (a NaN row kept in cell 0 would make a mean NaN)
    assert M > 50 and np.isfinite(rv).all() and np.isfinite(rm).all() and np.abs(rv[:, :, :3]).max() < 8
    parity_log.append(f"voxel edges non-finite/huge: N={n} ({len(bad)} bad rows) M={M} == C oracle bit-exact")
    pts[:, 0] = np.nan
    M0, *_ = _run(dev, pts, G753, ws, P_SHARED, max_voxels=200)
    assert M0 == 0
    parity_log.append(f"voxel edges all-NaN: N={n} M=0 == C oracle bit-exact")


# ---------------------------------------------------------------------------------------------------------------
# 2. points exactly on voxel planes and one ulp either side
def _plane_points(geo):
    f32 = np.float32
    rmin, rmax = np.array(geo["coors_range"][:3], np.float64), np.array(geo["coors_range"][3:], np.float64)
    vs, grid = np.array(geo["voxel_size"], np.float64), geo["grid"]
    mid = (rmin + (np.array(grid) // 3 + 0.5) * vs).astype(f32)      # mid-voxel on the two other axes
    rows = []
    for a in range(3):
        g = grid[a]
        vals = []
        for k in sorted({0, 1, 2, g // 2 - 1, g // 2, g - 1, g}):     # 0, 1, 2, 719, 720, 1439, 1440 for g = 1440
            x = f32(rmin[a] + k * vs[a])
            vals += [np.nextafter(x, f32(-np.inf)), x, np.nextafter(x, f32(np.inf))]
        vals += [f32(rmax[a]), np.nextafter(f32(rmax[a]), f32(-np.inf)), f32(-0.0) if rmin[a] == 0 else f32(rmin[a])]
        for v in vals:
            p = mid.copy()
            p[a] = v
            rows.append(p)
    xyz = np.stack(rows)
    feat = np.arange(len(rows), dtype=np.float32)[:, None] * np.array([[1.0, 0.5]], np.float32)
    return np.concatenate([xyz, feat], 1)


@pytest.mark.parametrize("name", ["nuscenes", "7x5x3"])
def test_points_on_voxel_planes(name, dev, ws, parity_log):
    geo = NUS if name == "nuscenes" else G753
    pts = _plane_points(geo)
    M, rv, rc, rn, rm = _run(dev, pts, geo, ws, P_SHARED, max_voxels=500, max_points=20)
    kept = int(rn.sum())
    assert 0 < kept < len(pts)                                       # some planes keep, some drop
    # both ends of every axis are reached: the first and the last cell
    for a, col in enumerate((2, 1, 0)):
        assert rc[:, col].min() == 0 and rc[:, col].max() == geo["grid"][a] - 1
    parity_log.append(f"voxel edges planes {name}: N={len(pts)} kept={kept} M={M} == C oracle bit-exact")


# ---------------------------------------------------------------------------------------------------------------
# 3. non-square grids
@pytest.mark.parametrize("grid", [[7, 5, 3], [5, 7, 3]])
def test_non_square_grid_every_voxel_once(grid, dev, ws, parity_log):
    geo = _unit_geo(grid)
    gx, gy, gz = grid
    rng = np.random.default_rng(301 + gx)
    keys = rng.permutation(np.repeat(np.arange(gx * gy * gz), 2))      # every voxel twice, shuffled
    pts = _centres(keys, geo, rng=rng)
    pts[:, :3] += (rng.random((len(keys), 3), dtype=np.float32) - 0.5) * 0.5
    M, rv, rc, rn, rm = _run(dev, pts, geo, ws, P_SHARED, max_voxels=200)
    assert M == gx * gy * gz
    want = sorted((z, y, x) for z in range(gz) for y in range(gy) for x in range(gx))
    assert sorted(map(tuple, rc.tolist())) == want                     # every (z, y, x) exactly once
    parity_log.append(f"voxel edges grid {grid} full: N={len(pts)} M={M} == C oracle bit-exact")


def test_non_square_grid_random(dev, ws, parity_log):
    geo = _unit_geo([200, 3, 11])
    pts = _cloud(np.random.default_rng(303), 500, geo, margin=0.25)
    M, rv, rc, rn, rm = _run(dev, pts, geo, ws, P_SHARED, max_voxels=600)
    assert rc[:, 2].max() > 11 and rc[:, 1].max() == 2 and rc[:, 0].max() == 10   # x beyond the y and z extents
    parity_log.append(f"voxel edges grid [200, 3, 11]: N=500 M={M} == C oracle bit-exact")


# ---------------------------------------------------------------------------------------------------------------
# 4. keys at and above 2^31
def test_keys_above_2_pow_31(dev, ws, parity_log):
    geo = _unit_geo([2048, 2048, 600])
    rng = np.random.default_rng(401)
    hi = _cloud(rng, 300, geo)
    hi[:, 2] = 512 + rng.random(300, dtype=np.float32) * 87.5          # z cell >= 512: key >= 512 * 2^22 = 2^31
    hi[0, :3] = [0.5, 0.5, 512.5]                                      # key == 2^31 exactly
    hi[1, :3] = [2047.5, 2047.5, 599.5]                                # the largest key of the grid
    lo = _cloud(rng, 300, geo)
    lo[:, 2] = rng.random(300, dtype=np.float32) * 511.5
    lo[0, :3] = [2047.5, 2047.5, 511.5]                                # key == 2^31 - 1
    pts = np.concatenate([hi, lo])[rng.permutation(600)]
    pts = np.concatenate([pts, pts[:40]])                              # second points in 40 of the voxels
    pts[600:, 3:] += 1.0
    M, rv, rc, rn, rm = _run(dev, pts, geo, ws, P_SHARED, max_voxels=1000)
    keys = _keys_of(rc, geo)
    assert M == 600 and (keys >= 2 ** 31).sum() == 300 and keys.max() == 600 * 2 ** 22 - 1
    assert (2 ** 31 in keys) and (2 ** 31 - 1 in keys)
    parity_log.append(f"voxel edges keys >= 2^31: N={len(pts)} M={M} (300 keys >= 2^31) == C oracle bit-exact")


# ---------------------------------------------------------------------------------------------------------------
# 5. row shapes.  (6, 0) is not in the list: the wrapper's empty means tensor has a null data pointer, which the
# entry point rejects (see test_nfeat_mean_zero_is_rejected).
@pytest.mark.parametrize("F,nmean", [(3, 3), (4, 4), (5, 3), (9, 8)])
def test_row_shapes(F, nmean, dev, ws, parity_log):
    rng = np.random.default_rng(500 + 10 * F + nmean)
    dense = _cloud(rng, 1500, G753, F=F, margin=0.1)                   # ~14 points in each of 105 voxels
    cells = _distinct_cells(rng, 700, NUS)
    sparse = _centres(cells[rng.integers(0, 700, size=1500)], NUS, F=F, rng=rng)   # mostly 1 to 3 points per voxel
    sparse[:, :3] += ((rng.random((1500, 3)) - 0.5) * 0.5 * np.array(NUS["voxel_size"])).astype(np.float32)
    for max_points in (1, 2, 3, 10, 35):
        Md, _, _, rn, _ = _run(dev, dense, G753, ws, P_SHARED, max_voxels=200, max_points=max_points, nmean=nmean)
        assert Md == 105 and (max_points > 3 or (rn == max_points).all())   # overfull for small max_points
        Ms, _, _, rn, rm = _run(dev, sparse, NUS, ws, P_SHARED, max_voxels=1000, max_points=max_points,
                                nmean=nmean)
        assert rm.shape == (Ms, nmean)
        if max_points == 35:
            assert np.isin([1, 2, 3], rn).all() and (rn <= 3).mean() > 0.5
    parity_log.append(f"voxel edges rows F={F} nfeat_mean={nmean}: max_points 1,2,3,10,35 x (N=1500 dense M={Md}, "
                      f"N=1500 sparse M={Ms}) == C oracle bit-exact")


def test_nfeat_mean_zero_is_rejected(dev, ws):
    from projects.mmdet3d_plugin import native as N
    pts = torch.from_numpy(_cloud(np.random.default_rng(55), 100, G753, F=6)).to(dev)
    with pytest.raises(RuntimeError, match="cmt_voxelize"):
        N.voxelize(pts, max_points=3, max_voxels=200, nfeat_mean=0, workspace=ws, **G753)
    _assert_clean(ws, P_SHARED)


# ---------------------------------------------------------------------------------------------------------------
# 6. one voxel holds everything
@pytest.mark.parametrize("max_points", [1, 2, 35])
def test_one_voxel_holds_everything(max_points, dev, ws, parity_log):
    rng = np.random.default_rng(600)
    n = 3000
    pts = np.zeros((n, 5), np.float32)
    pts[:, :3] = np.array([3.0, 2.0, 1.0], np.float32) + rng.random((n, 3), dtype=np.float32) * 0.999
    pts[:, 3] = np.arange(n)
    pts[:, 4] = rng.random(n, dtype=np.float32)
    M, rv, rc, rn, rm = _run(dev, pts, G753, ws, P_SHARED, max_voxels=50, max_points=max_points)
    assert M == 1 and rc.tolist() == [[1, 2, 3]] and rn.tolist() == [min(n, max_points)]
    assert np.array_equal(_bits(rv[0]), _bits(pts[:max_points]))       # points 0 .. max_points-1, in order
    parity_log.append(f"voxel edges one voxel: N={n} max_points={max_points} M=1 == C oracle bit-exact")


def test_duplicate_rows_keep_their_slots(dev, ws, parity_log):
    row = np.array([[3.25, 2.5, 1.75, 0.125, 9.0]], np.float32)
    pts = np.repeat(row, 3, 0)
    M, rv, rc, rn, rm = _run(dev, pts, G753, ws, P_SHARED, max_voxels=50, max_points=5)
    assert M == 1 and rn.tolist() == [3]
    assert np.array_equal(rv[0, :3], pts) and not rv[0, 3:].any()
    parity_log.append("voxel edges duplicate rows: N=3 M=1 == C oracle bit-exact")


# ---------------------------------------------------------------------------------------------------------------
# 7. tile boundaries: bin 256, workspace capacity 1024 / 4096, assign chunk 2048
TILE_N = [0, 1, 255, 256, 257, 1023, 1024, 1025, 2047, 2048, 2049, 4096, 4097]


@pytest.fixture(scope="module")
def distinct_points():
    """4097 points, each in its own cell of the nuScenes grid, in a seeded order (never modified)."""
    rng = np.random.default_rng(700)
    pts = _centres(_distinct_cells(rng, 4097, NUS), NUS, rng=rng)
    pts.setflags(write=False)
    return pts


def test_tile_boundaries(dev, ws8k, distinct_points, parity_log):
    from projects.mmdet3d_plugin import native as N
    for shared in (False, True):
        for n in TILE_N:
            P = 8192 if shared else _capacity(n)                       # n == capacity at 1024 and 4096
            w = ws8k if shared else N.voxelize_workspace(n, dev)
            M, *_ = _run(dev, distinct_points[:n], NUS, w, P, max_voxels=5000)
            assert M == n                                              # every point is its own voxel
    parity_log.append(f"voxel edges tiles: N in {TILE_N}, fresh workspace each and one shared, M=N "
                      "== C oracle bit-exact")


def test_empty_cloud_through_the_layer(dev):
    from projects.mmdet3d_plugin.mmcv_custom.ops.voxel import SPConvVoxelization
    layer = SPConvVoxelization(voxel_size=NUS["voxel_size"], point_cloud_range=NUS["coors_range"], max_num_points=10,
                               max_voxels=(100, 200), num_point_features=5).eval()
    vox, coors, num = layer(torch.zeros((0, 5), device=dev))
    assert vox.shape == (0, 10, 5) and coors.shape == (0, 3) and num.shape == (0,)
    assert vox.dtype == torch.float32 and coors.dtype == torch.int32 and num.dtype == torch.int32
    assert layer.forward_mean(torch.zeros((0, 5), device=dev), 3)[3].shape == (0, 3)


# ---------------------------------------------------------------------------------------------------------------
# 8. the voxel budget on an assign-chunk boundary
def test_budget_on_chunk_boundary(dev, ws8k, distinct_points, parity_log):
    for mv in (1, 2047, 2048, 2049, 4096, 4097, 5000):
        M, *_ = _run(dev, distinct_points, NUS, ws8k, 8192, max_voxels=mv)
        assert M == min(mv, 4097)
    # every voxel visited twice; the budget keeps the first half of the voxels and both of their points
    pts = np.concatenate([distinct_points[:2048], distinct_points[:2048]])
    pts[:, 4] = np.arange(4096)
    M, rv, rc, rn, rm = _run(dev, pts, NUS, ws8k, 8192, max_voxels=1024)
    assert M == 1024 and (rn == 2).all()
    kept = np.sort(rv[:, :2, 4].ravel()).astype(np.int64)
    assert np.array_equal(kept, np.concatenate([np.arange(1024), 2048 + np.arange(1024)]))
    parity_log.append("voxel edges budget: N=4097 max_voxels 1..5000 and N=4096 (2048 voxels twice) max_voxels=1024 "
                      "M=1024 == C oracle bit-exact")


# ---------------------------------------------------------------------------------------------------------------
# 9. probe sequences that must wrap around the end of the table
def _cells_hashing_to(rng, count, mask, lo, geo):
    gx, gy, gz = geo["grid"]
    keys = np.unique(rng.integers(0, gx * gy * gz, size=400 * count).astype(np.uint64))
    home = ((keys * np.uint64(HASH_MUL)) & np.uint64(0xFFFFFFFF)) & np.uint64(mask)
    keys = rng.permutation(keys[home >= lo])[:count]
    assert len(keys) == count
    return keys.astype(np.int64)


def _home(keys, mask):
    return [((int(k) * HASH_MUL) % 2 ** 32) & mask for k in keys]


def test_lds_probe_wraps(dev, ws, parity_log):
    rng = np.random.default_rng(901)
    keys = _cells_hashing_to(rng, 200, 511, 480, NUS)
    # 200 distinct keys whose home entry is one of the last 32 of the 512-entry LDS table: the probe must wrap
    assert len(set(keys.tolist())) == 200 and all(480 <= h <= 511 for h in _home(keys, 511))
    first = np.concatenate([keys, keys[:56]])[rng.permutation(256)]    # one bin workgroup: points 0..255
    pts = np.concatenate([_centres(first, NUS, rng=rng), _cloud(rng, 344, NUS)])
    pts[:, 4] = np.arange(600)
    M, rv, rc, rn, rm = _run(dev, pts, NUS, ws, P_SHARED, max_voxels=1000)
    assert set(keys.tolist()) <= set(_keys_of(rc, NUS).tolist())
    parity_log.append(f"voxel edges LDS probe wrap: N=600 (200 keys at LDS entries 480..511) M={M} "
                      "== C oracle bit-exact")


def test_global_probe_wraps(dev, parity_log):
    from projects.mmdet3d_plugin import native as N
    rng = np.random.default_rng(902)
    keys = _cells_hashing_to(rng, 40, 2047, 2040, NUS)
    # capacity 1024 -> 2048 table slots; 40 distinct keys whose home slot is one of the last 8: the probe must wrap
    assert len(set(keys.tolist())) == 40 and all(2040 <= h <= 2047 for h in _home(keys, 2047))
    pts = _cloud(rng, 1000, NUS)
    where = rng.choice(1000, 80, replace=False)
    pts[where] = _centres(np.concatenate([keys, keys]), NUS, rng=rng)
    w = N.voxelize_workspace(1024, dev)
    M, rv, rc, rn, rm = _run(dev, pts, NUS, w, 1024, max_voxels=1000)
    assert set(keys.tolist()) <= set(_keys_of(rc, NUS).tolist())
    parity_log.append(f"voxel edges global probe wrap: N=1000 (40 keys at slots 2040..2047 of 2048) M={M} "
                      "== C oracle bit-exact")


# ---------------------------------------------------------------------------------------------------------------
# 10. a workspace that is too small
def test_workspace_too_small(dev, distinct_points, parity_log):
    from projects.mmdet3d_plugin import native as N
    w = N.voxelize_workspace(1024, dev)
    with pytest.raises(RuntimeError, match="workspace too small"):
        N.voxelize(torch.from_numpy(distinct_points[:1025].copy()).to(dev), max_points=10, max_voxels=2000,
                   nfeat_mean=5, workspace=w, **NUS)
    assert bool((w == 0xFF).all())                                     # untouched
    M, *_ = _run(dev, distinct_points[:1024], NUS, w, 1024, max_voxels=2000)
    assert M == 1024
    parity_log.append("voxel edges small workspace: N=1025 on capacity 1024 raises, then N=1024 M=1024 "
                      "== C oracle bit-exact")


# ---------------------------------------------------------------------------------------------------------------
# 11. the layer
def _layer(F, max_voxels, max_points=4):
    from projects.mmdet3d_plugin.mmcv_custom.ops.voxel import SPConvVoxelization
    return SPConvVoxelization(voxel_size=G753["voxel_size"], point_cloud_range=G753["coors_range"],
                              max_num_points=max_points, max_voxels=max_voxels, num_point_features=F)


def _same_trimmed(got, ref, with_means):
    M = ref[0]
    assert got[0].shape[0] == M and got[1].shape == (M, 3) and got[2].shape == (M,)
    assert np.array_equal(_bits(got[0]), _bits(ref[1]))
    assert np.array_equal(got[1].cpu().numpy(), ref[2]) and np.array_equal(got[2].cpu().numpy(), ref[3])
    if with_means:
        assert got[3].shape == ref[4].shape and np.array_equal(_bits(got[3]), _bits(ref[4]))


def test_layer_modes_and_shapes(dev, parity_log):
    pts = _cloud(np.random.default_rng(1101), 400, G753, F=4, margin=0.25)
    tp = torch.from_numpy(pts).to(dev)
    layer = _layer(4, (50, 200))
    assert layer.grid_size.tolist() == [7, 5, 3]
    ref_eval, ref_train = _oracle(pts, G753, 4, 200, 4), _oracle(pts, G753, 4, 50, 4)
    assert ref_eval[0] > 50 and ref_train[0] == 50                     # the budget bites in training only
    layer.train()
    _same_trimmed(layer(tp), ref_train, False)
    layer.eval()
    _same_trimmed(layer(tp), ref_eval, False)
    _same_trimmed(layer.forward_mean(tp, 3), _oracle(pts, G753, 4, 200, 3), True)
    padded = layer.forward_padded(tp, nfeat_mean=4)
    assert padded[0].shape == (200, 4, 4) and padded[3].shape == (200, 4) and padded[4].shape == (1,)
    _same(padded, ref_eval)
    _assert_clean(layer._ws, layer._ws_cap)
    # forward asks for min(F, 8) mean columns: F = 9 is above the gather kernel's 8-wide accumulator
    pts9 = _cloud(np.random.default_rng(1102), 400, G753, F=9, margin=0.25)
    layer9 = _layer(9, 200).eval()
    _same_trimmed(layer9(torch.from_numpy(pts9).to(dev)), _oracle(pts9, G753, 4, 200, 8), False)
    _assert_clean(layer9._ws, layer9._ws_cap)
    parity_log.append(f"voxel edges layer: F=4 train M={ref_train[0]} / eval M={ref_eval[0]}, forward, forward_mean(3), "
                      "forward_padded, F=9 forward == C oracle bit-exact")


def test_layer_input_dtypes_and_strides(dev, parity_log):
    rng = np.random.default_rng(1103)
    wide = np.concatenate([_cloud(rng, 400, G753, F=4, margin=0.25), rng.random((400, 2), dtype=np.float32)], 1)
    pts = np.ascontiguousarray(wide[:, :4])
    layer = _layer(4, 200).eval()
    ref = _oracle(pts, G753, 4, 200, 3)
    view = torch.from_numpy(wide).to(dev)[:, :4]
    assert not view.is_contiguous()
    for x in (torch.from_numpy(pts).to(dev), view, torch.from_numpy(pts).to(dev).double(), view.double()):
        _same_trimmed(layer.forward_mean(x, 3), ref, True)
    parity_log.append(f"voxel edges layer inputs: fp32 / fp64, contiguous / strided N=400 M={ref[0]} "
                      "== C oracle bit-exact")


def test_voxelize_batch_with_empty_middle_cloud(dev, parity_log):
    from projects.mmdet3d_plugin.mmcv_custom.ops.voxel import voxelize_batch
    rng = np.random.default_rng(1104)
    a, c = _cloud(rng, 300, G753, F=4, margin=0.25), _cloud(rng, 200, G753, F=4, margin=0.25)
    layer = _layer(4, 200).eval()
    clouds = [torch.from_numpy(a).to(dev), torch.zeros((0, 4), device=dev), torch.from_numpy(c).to(dev)]
    feats, nums, coors = voxelize_batch(layer, clouds, num_features=3)
    ra, rc_ = _oracle(a, G753, 4, 200, 3), _oracle(c, G753, 4, 200, 3)
    Ma, Mc = ra[0], rc_[0]
    assert feats.shape == (Ma + Mc, 3) and nums.shape == (Ma + Mc,) and coors.shape == (Ma + Mc, 4)
    batch = coors[:, 0].cpu().numpy()
    assert np.array_equal(batch, np.concatenate([np.zeros(Ma, np.int64), np.full(Mc, 2, np.int64)]))   # 0 and 2 only
    assert np.array_equal(coors[:, 1:].cpu().numpy(), np.concatenate([ra[2], rc_[2]]))
    assert np.array_equal(nums.cpu().numpy(), np.concatenate([ra[3], rc_[3]]))
    assert np.array_equal(_bits(feats), _bits(np.concatenate([ra[4], rc_[4]])))
    parity_log.append(f"voxel edges batch: clouds of 300 / 0 / 200 points M={Ma}+0+{Mc} == C oracle bit-exact")
