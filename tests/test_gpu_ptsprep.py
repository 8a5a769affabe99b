"""cmt_pts_prepare on the GPU against the numpy contract of tests/_pts_ref.py: remove_close, sweep transform, time
column, column selection, agent transform and range filter as an order-preserving compaction in two launches.

Every case writes into a destination that was pre-filled with a finite garbage value and has sentinel rows on both
sides.  It asserts that the sentinels are intact, that ``count`` is the contract's, that rows [0, count) equal the
contract's bit for bit and that rows [count, n) are the quiet NaN 0x7FC00000 in every column: the arithmetic is a
fixed sequence of IEEE operations, so there is no tolerance to choose.  One exception is spelled out in ``_same``:
where the contract's own value is a NaN that arithmetic produced (inf * 0, inf - inf), sign and payload are not
part of the contract and any NaN is accepted; NaNs that are merely copied keep their bits.
"""
import numpy as np
import pytest
import torch

import _pts_ref as R
from projects.mmdet3d_plugin import native_pts as NP

pytestmark = pytest.mark.gpu

GARBAGE = 777.25
SENTINEL = -12345.5
GUARD = 3      # sentinel rows on each side of the destination
RANGE = [-40.0, -40.0, -4.0, 40.0, 40.0, 2.0]
USE = {4: [0, 1, 2, 3], 5: [0, 1, 2, 4], 6: [0, 1, 2, 5, 3]}


def _T():
    return NP.tile_rows()


def _same(got, want):
    """uint32 words equal, or both NaN where the contract's NaN came out of arithmetic"""
    return (got == want) | (np.isnan(got.view(np.float32)) & np.isnan(want.view(np.float32)))


def _device_segments(dev, segs, load_dim, lead_rows=0, separate=False):
    """the segments' rows as consecutive slices of one device buffer (``lead_rows`` unused rows in front), or as
    separately allocated tensors"""
    out = []
    if separate:
        for s in segs:
            out.append(dict(s, points=torch.from_numpy(s["points"]).to(dev)))
        return out
    n = sum(s["points"].shape[0] for s in segs)
    raw = np.full((lead_rows + n, load_dim), 31.0, np.float32)
    raw[lead_rows:] = np.concatenate([s["points"] for s in segs], 0) if n else 0
    buf = torch.from_numpy(raw).to(dev)
    at = lead_rows
    for s in segs:
        k = s["points"].shape[0]
        out.append(dict(s, points=buf[at:at + k]))
        at += k
    return out


def _run_and_check(dev, segs, use_dim, load_dim, agent=None, rng=None, lead_rows=0, separate=False, workspace=None):
    """-> (destination words [n, F], count).  ``segs`` hold numpy rows (R.seg)."""
    n = sum(s["points"].shape[0] for s in segs)
    F = len(use_dim)
    buf = torch.full(((n + 2 * GUARD), F), GARBAGE, dtype=torch.float32, device=dev)
    buf[:GUARD] = SENTINEL
    buf[GUARD + n:] = SENTINEL
    out = buf[GUARD:GUARD + n]
    dsegs = _device_segments(dev, segs, load_dim, lead_rows, separate)
    v2i = None
    if agent is not None:
        v2i = np.eye(4)
        v2i[:3, :3], v2i[:3, 3] = agent
    got, count = NP.prepare_points(dsegs, use_dim=use_dim, load_dim=load_dim, agent_transform=v2i,
                                   point_cloud_range=rng, out=out, workspace=workspace)
    assert got.data_ptr() == out.data_ptr() and tuple(got.shape) == (n, F)
    assert count.dtype == torch.int32 and tuple(count.shape) == (1,) and count.device == out.device
    torch.cuda.synchronize()
    host = buf.cpu().numpy()
    assert np.all(host[:GUARD] == SENTINEL), "rows before the destination overwritten"
    assert np.all(host[GUARD + n:] == SENTINEL), "rows after the destination overwritten"
    words = host[GUARD:GUARD + n].view(np.uint32)
    want, want_count = R.padded(segs, use_dim, agent, rng)
    c = int(count.item())
    bad = ~_same(words[:want_count], want[:want_count]) if c == want_count else None
    print(f"ptsprep n {n} S {len(segs)} load_dim {load_dim} use {use_dim} agent {agent is not None} range "
          f"{rng is not None}: count {c} (contract {want_count}), "
          f"{'-' if bad is None else int(bad.sum())} kept words differ")
    assert c == want_count
    assert not bad.any(), f"kept rows differ from the contract at {np.argwhere(bad)[:4].tolist()}"
    assert np.all(words[c:] == R.QNAN), "the tail is not quiet NaN in every column"
    return words, c


def _cloud(rng, n, load_dim, scale=1.2):
    """rows around RANGE, a share of them outside it, some close to the sensor"""
    p = rng.uniform(-1, 1, (n, load_dim)).astype(np.float32)
    p[:, 0] *= np.float32(40 * scale)
    p[:, 1] *= np.float32(40 * scale)
    p[:, 2] = (p[:, 2] * np.float32(3 * scale) - np.float32(1)).astype(np.float32)
    p[:, 3:] = rng.uniform(0, 255, (n, load_dim - 3)).astype(np.float32)
    near = rng.random(n) < 0.1
    p[near, :2] = rng.uniform(-1.5, 1.5, (int(near.sum()), 2)).astype(np.float32)
    return p


def _split(rng, n, S, empty):
    """S segment sizes that sum to n, cut at random rows (inside tiles); the segments listed in ``empty`` hold none"""
    live = [s for s in range(S) if s not in empty] or [0]
    cuts = np.sort(rng.integers(0, n + 1, len(live) - 1)) if n else np.zeros(len(live) - 1, int)
    sizes = np.diff(np.concatenate([[0], cuts, [n]])).astype(int)
    out = [0] * S
    for s, k in zip(live, sizes):
        out[s] = int(k)
    return out


def _segments(rng, n, S, load_dim, empty=(), sweep=True, close=True, time=True):
    sizes = _split(rng, n, S, empty)
    segs = []
    for s, k in enumerate(sizes):
        rot, trans = R.rigid(rng, 2.0) if (sweep and s > 0) else (None, None)
        segs.append(R.seg(_cloud(rng, k, load_dim), rot, trans, (1.0 if s % 2 else 0.75) if (close and s > 0) else 0.0,
                          (load_dim - 1) if time else None, np.float32(0.05 * s) if time else None))
    return segs


def _empties(S, i):
    if S >= 5:
        return (0, S // 2, S - 1)
    if S == 3:
        return (i % 3,)
    return ()


def _sizes():
    T = _T()
    return [0, 1, 63, 64, 65, T - 1, T, T + 1, 3 * T + 5]


@pytest.mark.parametrize("i", range(9))
@pytest.mark.parametrize("S", [1, 3, 11, 16])
def test_sizes_and_segments(dev, i, S):
    """every size x every segment count; load_dim / use_dim and the optional steps cycle with the case"""
    n = _sizes()[i]
    k = i + [1, 3, 11, 16].index(S)
    load_dim = (4, 5, 6)[k % 3]
    use_dim = [0, 1, 2, 3, 4] if (load_dim >= 5 and k % 2) else USE[load_dim]
    rng = np.random.default_rng(1000 + 16 * i + S)
    segs = _segments(rng, n, S, load_dim, _empties(S, i), sweep=k % 4 != 3, close=k % 3 != 0, time=k % 5 != 4)
    agent = R.rigid(rng, 10.0) if k % 2 == 0 else None
    if agent is not None:
        agent = (agent[0], agent[1] * np.array([1.0, 1.0, 0.1]))
    _run_and_check(dev, segs, use_dim, load_dim, agent, RANGE if k % 7 != 6 else None)


@pytest.mark.parametrize("load_dim,use_dim", [(4, [0, 1, 2, 3]), (5, [0, 1, 2, 4]), (5, [0, 1, 2, 3, 4]),
                                               (6, [0, 1, 2, 5, 3]), (8, [0, 1, 2, 7, 6, 5, 4, 3]), (3, [0, 1, 2]),
                                               (5, [0, 1, 2, 1, 4, 0])])
def test_columns(dev, load_dim, use_dim):
    rng = np.random.default_rng(7 + load_dim)
    segs = _segments(rng, _T() + 77, 3, load_dim, time=load_dim > 3)
    agent = R.rigid(rng, 5.0)
    _run_and_check(dev, segs, use_dim, load_dim, (agent[0], agent[1] * 0.1), RANGE)


def test_time_column_on_a_coordinate_and_unselected(dev):
    """time_col may be any column: one that use_dim drops, or (oddly) a coordinate, which then holds the value
    after the sweep transform and before the agent transform"""
    rng = np.random.default_rng(3)
    p = _cloud(rng, 300, 5)
    rot, trans = R.rigid(rng, 1.0)
    _run_and_check(dev, [R.seg(p, rot, trans, 0.0, 3, 0.5)], [0, 1, 2, 4], 5, None, RANGE)
    _run_and_check(dev, [R.seg(p, rot, trans, 0.0, 2, -1.5)], [0, 1, 2, 3, 2], 5, R.rigid(rng, 1.0), RANGE)


@pytest.mark.parametrize("opts", range(32))
def test_each_optional_step_on_and_off(dev, opts):
    sweep, close, time, agent_on, range_on = ((opts >> b) & 1 for b in range(5))
    rng = np.random.default_rng(50 + opts)
    segs = _segments(rng, _T() + 1, 3, 5, sweep=bool(sweep), close=bool(close), time=bool(time))
    agent = R.rigid(rng, 5.0) if agent_on else None
    if agent is not None:
        agent = (agent[0], agent[1] * 0.1)
    words, c = _run_and_check(dev, segs, [0, 1, 2, 3, 4], 5, agent, RANGE if range_on else None)
    if not (close or range_on):
        assert c == _T() + 1
    else:
        assert 0 < c < _T() + 1


# ---- keep patterns -----------------------------------------------------------------------------------------------
def _pattern_rows(n, keep):
    """rows whose x lies inside RANGE where ``keep`` and outside elsewhere; features tell the rows apart"""
    p = np.zeros((n, 5), np.float32)
    p[:, 0] = np.where(keep, 1.0, 100.0)
    p[:, 1] = (np.arange(n) % 61) * 0.5 - 15
    p[:, 2] = -1.0
    p[:, 3] = np.arange(n)
    p[:, 4] = np.arange(n) % 7
    return p


@pytest.mark.parametrize("pattern", ["all", "none", "alternating", "last", "first", "last_of_full_tile", "one_per_tile"])
def test_keep_patterns(dev, pattern):
    T = _T()
    n = 2 * T if pattern == "last_of_full_tile" else 3 * T + 5
    keep = np.zeros(n, bool)
    if pattern == "all":
        keep[:] = True
    elif pattern == "alternating":
        keep[::2] = True
    elif pattern in ("last", "last_of_full_tile"):
        keep[-1] = True
    elif pattern == "first":
        keep[0] = True
    elif pattern == "one_per_tile":
        keep[T - 1::T] = True
    p = _pattern_rows(n, keep)
    cuts = [0, T // 2, T + 3, n]
    segs = [R.seg(p[a:b]) for a, b in zip(cuts[:-1], cuts[1:])]
    words, c = _run_and_check(dev, segs, [0, 1, 2, 3, 4], 5, None, RANGE)
    assert c == int(keep.sum())
    assert np.array_equal(words[:c, 3].view(np.float32), np.flatnonzero(keep).astype(np.float32))   # input order
    if pattern == "none":
        assert np.all(words == R.QNAN)


def test_more_tiles_than_threads(dev):
    """257 tiles and one row: a thread of the scatter launch sums more than one entry of the tiles' counts"""
    T = _T()
    n = 257 * T + 1
    keep = np.zeros(n, bool)
    keep[T - 1::T] = True
    keep[-1] = True
    p = _pattern_rows(n, keep)[:, :4].copy()
    words, c = _run_and_check(dev, [R.seg(p)], [0, 1, 2, 3], 4, None, RANGE)
    assert c == 258
    assert np.array_equal(words[:c, 3].view(np.float32), np.flatnonzero(keep).astype(np.float32))   # input order


# ---- edges -------------------------------------------------------------------------------------------------------
def test_range_faces(dev):
    """a coordinate exactly on one of the six faces drops the row, the next float inside keeps it"""
    lo, hi = np.array(RANGE[:3], np.float32), np.array(RANGE[3:], np.float32)
    rows, want = [], []
    for k in range(3):
        for face, inward in ((lo[k], hi[k]), (hi[k], lo[k])):
            on = np.array([1.0, 2.0, -1.0, 5.0, 0.0], np.float32)
            on[k] = face
            inside = on.copy()
            inside[k] = np.nextafter(face, inward)
            outside = on.copy()
            outside[k] = np.nextafter(face, 2 * face - inward)
            rows += [on, inside, outside]
            want += [False, True, False]
    p = np.stack(rows)
    words, c = _run_and_check(dev, [R.seg(p)], [0, 1, 2, 3, 4], 5, None, RANGE)
    assert c == 6 and np.array_equal(words[:c], p[np.array(want)].view(np.uint32))


def test_close_radius_edges(dev):
    r = np.float32(1.0)
    below = np.nextafter(r, np.float32(0))
    p = np.array([[r, 0.5, 0, 1, 0], [-r, 0.5, 0, 2, 0], [0.5, r, 0, 3, 0], [0.5, -r, 0, 4, 0],    # |x| or |y| == r: kept
                  [below, below, 0, 5, 0], [-below, below, 0, 6, 0], [0, -0.0, 0, 7, 0],            # both below: dropped
                  [below, r, 0, 8, 0], [np.nan, 0.1, 0, 9, 0], [0.1, np.nan, 0, 10, 0],             # NaN compares false: kept
                  [np.inf, 0.1, 0, 11, 0], [50, 50, 0, 12, 0]], np.float32)
    words, c = _run_and_check(dev, [R.seg(p[:5], remove_close=1.0), R.seg(p[5:], remove_close=1.0)], [0, 1, 2, 3], 5)
    assert words[:c, 3].view(np.float32).tolist() == [1, 2, 3, 4, 8, 9, 10, 11, 12]


SPECIALS = [0.0, -0.0, np.nan, np.inf, -np.inf, 1e-45, -1e-45, 1.1754942e-38, 5e-39, 3.4028235e38]


@pytest.mark.parametrize("mode", ["plain", "range", "all_steps"])
def test_special_values(dev, mode):
    """+-0, NaN, +-inf, subnormals and the largest float in each coordinate and in a feature column"""
    base = np.array([1.0, 2.0, -1.0, 5.0, 0.25], np.float32)
    rows = []
    for col in range(5):
        for v in SPECIALS:
            row = base.copy()
            row[col] = v
            rows.append(row)
    p = np.stack(rows).astype(np.float32)
    p = np.concatenate([p, p * np.float32(1e-40)])   # whole rows of subnormals
    rng = np.random.default_rng(9)
    if mode == "plain":
        # no filter: rows with NaN or inf coordinates are kept, as in the reference
        words, c = _run_and_check(dev, [R.seg(p)], [0, 1, 2, 3, 4], 5)
        assert c == p.shape[0] and np.array_equal(words, p.view(np.uint32))   # pure copies keep every bit
    elif mode == "range":
        words, c = _run_and_check(dev, [R.seg(p)], [0, 1, 2, 3, 4], 5, None, RANGE)
        kept = words[:c].view(np.float32)
        assert np.isfinite(kept[:, :3]).all()                     # NaN and +-inf coordinates are dropped
        assert np.isnan(kept[:, 3:]).any() and np.isinf(kept[:, 3:]).any()   # non-finite features are copied
        with np.errstate(invalid="ignore"):
            inside = np.all((p[:, :3] > np.array(RANGE[:3], np.float32)) & (p[:, :3] < np.array(RANGE[3:], np.float32)), 1)
        assert c == int(inside.sum()) < p.shape[0]
    else:
        rot, trans = R.rigid(rng, 1.0)
        agent = (np.eye(3) * 0.5, np.array([1e-39, 0.0, -1e-39]))   # subnormals stay subnormal through the products
        segs = [R.seg(p[:37], rot * 1e-3, trans * 1e-40, 0.5, 4, 1e-41), R.seg(p[37:], rot, trans, 1e-39, 3, -0.0)]
        _run_and_check(dev, segs, [0, 1, 2, 3, 4], 5, agent, None)
        _run_and_check(dev, segs, [0, 1, 2, 3, 4], 5, agent, [-1e-38, -40, -4, 40, 40, 1e-38])


def test_nan_feature_keeps_its_payload(dev):
    p = np.array([[1, 2, -1, 0, 0], [3, 4, -2, 0, 0]], np.float32)
    p.view(np.uint32)[0, 3] = 0x7FC12345
    p.view(np.uint32)[1, 4] = 0xFFA00001
    rot, trans = R.rigid(np.random.default_rng(2), 1.0)
    words, c = _run_and_check(dev, [R.seg(p, rot, trans)], [0, 1, 2, 3, 4], 5, R.rigid(np.random.default_rng(3), 1.0), RANGE)
    assert c == 2 and words[0, 3] == 0x7FC12345 and words[1, 4] == 0xFFA00001


# ---- layouts -----------------------------------------------------------------------------------------------------
def test_source_misaligned_to_16_bytes(dev):
    """a view that starts one 20-byte row into a load_dim = 5 buffer"""
    rng = np.random.default_rng(21)
    segs = _segments(rng, 2 * _T() + 9, 3, 5)
    dsegs = _device_segments(dev, segs, 5, lead_rows=1)
    assert dsegs[0]["points"].data_ptr() % 16 == 4
    _run_and_check(dev, segs, [0, 1, 2, 3, 4], 5, R.rigid(rng, 3.0), RANGE, lead_rows=1)


def test_separate_buffers_and_trim(dev):
    """segments that are not one buffer are concatenated first; trim=True returns the kept rows (a host read)"""
    rng = np.random.default_rng(22)
    segs = _segments(rng, _T() + 300, 3, 5)
    words, c = _run_and_check(dev, segs, [0, 1, 2, 4], 5, None, RANGE, separate=True)
    dsegs = _device_segments(dev, segs, 5)
    trimmed = NP.prepare_points(dsegs, use_dim=[0, 1, 2, 4], load_dim=5, point_cloud_range=RANGE, trim=True)
    assert tuple(trimmed.shape) == (c, 4)
    assert np.array_equal(trimmed.cpu().numpy().view(np.uint32), words[:c])
    # one buffer is used in place: no copy
    ptr, owner = NP._one_buffer([s["points"] for s in dsegs])
    assert ptr == dsegs[0]["points"].data_ptr() and owner is dsegs[0]["points"]
    ptr, owner = NP._one_buffer([dsegs[0]["points"], dsegs[2]["points"]])
    assert ptr != dsegs[0]["points"].data_ptr() and owner.shape[0] == dsegs[0]["points"].shape[0] + dsegs[2]["points"].shape[0]


def test_repeatable_and_workspace_reuse(dev):
    """two calls give identical bytes; another input through the same workspace is right: nothing to clean"""
    rng = np.random.default_rng(23)
    ws = NP.PointsWorkspace()
    a = _segments(rng, 3 * _T() + 5, 3, 5)
    w1, c1 = _run_and_check(dev, a, [0, 1, 2, 3, 4], 5, None, RANGE, workspace=ws)
    held = ws.get(0, dev)
    w2, c2 = _run_and_check(dev, a, [0, 1, 2, 3, 4], 5, None, RANGE, workspace=ws)
    assert c1 == c2 and np.array_equal(w1, w2)
    b = _segments(rng, _T() + 11, 11, 6, _empties(11, 0))
    _run_and_check(dev, b, USE[6], 6, R.rigid(rng, 2.0), RANGE, workspace=ws)
    _run_and_check(dev, a, [0, 1, 2, 3, 4], 5, None, RANGE, workspace=ws)
    assert ws.get(0, dev).data_ptr() == held.data_ptr()       # the holder kept its buffer
    raw = torch.full((64,), -1, dtype=torch.int32, device=dev)   # a caller's tensor, dirty
    w3, c3 = _run_and_check(dev, a, [0, 1, 2, 3, 4], 5, None, RANGE, workspace=raw)
    assert c3 == c1 and np.array_equal(w3, w1)
    with pytest.raises(ValueError, match="workspace"):
        NP.prepare_points(_device_segments(dev, a, 5), use_dim=5, workspace=raw[:2])


def test_graph_capture(dev):
    """no allocation, no synchronisation: the call replays from a HIP graph on new data"""
    rng = np.random.default_rng(24)
    n = 2 * _T() + 3
    segs = _segments(rng, n, 3, 5)
    dsegs = _device_segments(dev, segs, 5)
    out = torch.zeros((n, 5), dtype=torch.float32, device=dev)
    ws = torch.empty(16, dtype=torch.int32, device=dev)
    stream = torch.cuda.Stream()
    stream.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(stream):
        NP.prepare_points(dsegs, use_dim=5, point_cloud_range=RANGE, out=out, workspace=ws)   # warm-up
    torch.cuda.current_stream().wait_stream(stream)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        _, count = NP.prepare_points(dsegs, use_dim=5, point_cloud_range=RANGE, out=out, workspace=ws)
    other = _segments(rng, n, 3, 5)
    for s, d, o in zip(segs, dsegs, other):
        k = min(s["points"].shape[0], o["points"].shape[0])   # same segment sizes are baked in: reuse the first rows
        s["points"][:k] = o["points"][:k]
        d["points"].copy_(torch.from_numpy(s["points"]))
    out.fill_(GARBAGE)
    graph.replay()
    torch.cuda.synchronize()
    want, want_count = R.padded(segs, [0, 1, 2, 3, 4], None, RANGE)
    assert int(count.item()) == want_count
    assert np.array_equal(out.cpu().numpy().view(np.uint32), want)


# ---- downstream --------------------------------------------------------------------------------------------------
def test_voxelizer_equivalence(dev):
    """the padded buffer voxelizes like the trimmed one, with the voxel cap and the per-voxel cap both biting"""
    from projects.mmdet3d_plugin.mmcv_custom.ops.voxel import SPConvVoxelization
    rng = np.random.default_rng(31)
    n = 3 * _T() + 5
    p = rng.uniform(-1, 1, (n, 5)).astype(np.float32) * np.array([10, 10, 2.5, 1, 1], np.float32)
    pcr = [-8.0, -8.0, -2.0, 8.0, 8.0, 2.0]
    segs = [R.seg(p[:n // 3], time_col=4, time=0.0), R.seg(p[n // 3:], *R.rigid(rng, 0.5), 1.0, 4, 0.1)]
    padded, count = NP.prepare_points(_device_segments(dev, segs, 5), use_dim=5, point_cloud_range=pcr)
    c = int(count.item())
    assert 0 < c < n and torch.isnan(padded[c:]).all() and torch.isfinite(padded[:c]).all()
    layer = SPConvVoxelization(voxel_size=[0.5, 0.5, 4.0], point_cloud_range=pcr, max_num_points=3,
                               max_voxels=(600, 600), num_point_features=5).eval()
    a = [t.clone() for t in layer.forward_padded(padded)]
    b = [t.clone() for t in layer.forward_padded(padded[:c].contiguous())]
    torch.cuda.synchronize()
    m = int(a[4].item())
    assert m == int(b[4].item()) == 600            # 32 x 32 cells are occupied: the voxel cap bites
    assert int(a[2][:m].max().item()) == 3         # and the per-voxel cap
    for x, y, name in zip(a[:4], b[:4], ("voxels", "coors", "num_points", "mean")):
        assert torch.equal(x[:m], y[:m]), name


def test_detector_takes_the_padded_buffer(dev):
    """a small LiDAR-only CmtDetector gives identical boxes for points=[padded] and points=[trimmed]"""
    from projects.mmdet3d_plugin import build_detector
    from projects.mmdet3d_plugin import synthetic as S
    cfg = S.make_detector_cfg("cmt_lidar_nus", num_query=64, num_layers=2, grid_size=[256, 256, 40], spec_name="V-19-eSE")
    torch.manual_seed(0)
    det = build_detector(cfg)
    det.init_weights()
    S._jitter_(det, torch.Generator().manual_seed(1))
    det = det.eval().to(dev)
    pcr = cfg["pts_voxel_layer"]["point_cloud_range"]
    key = S.synthetic_points(1500, pcr, seed=5, margin=2.0)
    sweep = S.synthetic_points(1500, pcr, seed=6, margin=2.0)
    raw = torch.cat([key, sweep]).to(dev)
    rot, trans = R.rigid(np.random.default_rng(7), 0.5)
    segs = [dict(points=raw[:1500], time_col=4, time=0.0),
            dict(points=raw[1500:], rotation=rot, translation=trans, remove_close=1.0, time_col=4, time=0.05)]
    padded, count = NP.prepare_points(segs, use_dim=5, point_cloud_range=pcr)
    c = int(count.item())
    assert 0 < c < 3000
    with torch.no_grad():
        a = det(return_loss=False, points=[[padded]], img_metas=[[dict()]])[0]["pts_bbox"]
        b = det(return_loss=False, points=[[padded[:c].contiguous()]], img_metas=[[dict()]])[0]["pts_bbox"]
    assert a["scores_3d"].numel() > 0
    for k in ("boxes_3d", "scores_3d", "labels_3d"):
        assert torch.equal(a[k], b[k]), k


def test_cli_sweeps(dev, tmp_path):
    """tools/test.py --detector --sweeps in this process: both coop clouds go through prepare_points with the config's
    plan (vehicle2infrastructure and the range filter included) and the detector takes the padded buffers"""
    import importlib.util
    import json
    import os
    from conftest import PKG
    spec = importlib.util.spec_from_file_location("cmt_test_cli_pts", os.path.join(PKG, "tools", "test.py"))
    cli = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(cli)
    out = tmp_path / "f.json"
    rc = cli.main(["cmtcoop_lidar_tumtraf", "--synthetic", "--detector", "--sweeps", "2", "--num-query", "64",
                   "--num-layers", "1", "--grid", "32", "32", "--points", "700", "--out", str(out)])
    assert rc == 0
    fr = json.loads(out.read_text())["frames"][0]
    n = len(fr["scores_3d"])
    assert n > 0 and len(fr["boxes_3d"]) == n == len(fr["labels_3d"]) and len(fr["boxes_3d"][0]) == 9
    assert len(fr["voxels"]) == 2
    for v in fr["voxels"]:
        assert v["voxels"] > 0 and 0 < v["points_kept"] < 3 * 700   # the margin and the moved vehicle cloud drop rows
