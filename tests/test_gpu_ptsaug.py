"""cmt_points_in_boxes, cmt_pts_augment and cmt_boxes_augment on the GPU against the numpy contract of
tests/_aug_ref.py.

Every destination is pre-filled with a finite garbage value and has sentinel rows on both sides.  The transforms are
a fixed sequence of IEEE float32 operations, so rows are compared bit for bit (``_same`` accepts any NaN where the
contract's own value is a NaN that arithmetic produced).  The inside test binds only points farther than the
contract's margin from every face plane; ``R.inside_inputs`` builds such points and asserts that they are, and on
those the device's answers equal the float64 reference exactly.  Shapes are the smallest at which the kernels take
another path: around the tile T of the compaction and the box chunk Cb.
"""
import ctypes

import numpy as np
import pytest
import torch

import _aug_ref as R
from projects.mmdet3d_plugin import native
from projects.mmdet3d_plugin import native_aug as NA

pytestmark = pytest.mark.gpu

GARBAGE = 777.25
SENTINEL = -12345.5
IGARBAGE = 7777
ISENTINEL = -424242
GUARD = 3
RANGE = [-18.0, -18.0, -3.0, 18.0, 18.0, 3.0]
YAWS = [0.0, np.pi / 2, -2.5, 7.0]
EINVAL = 1001
ALL = dict(angle=0.3, scale=1.04, trans=[0.4, -0.3, 0.1], flip_h=True, flip_v=True)
STEPS = {"rot": dict(angle=-0.6), "scale": dict(scale=0.93), "trans": dict(trans=[0.5, -0.25, 0.125]),
         "flip_h": dict(flip_h=True), "flip_v": dict(flip_v=True), "all": ALL}


def _T():
    return NA.tile_rows()


def _same(got, want):
    return (got == want) | (np.isnan(got.view(np.float32)) & np.isnan(want.view(np.float32)))


def _boxes(rng, m, D=7, spread=12.0):
    """m finite boxes, extents 1.5 .. 5 m, the yaws of YAWS in turn"""
    b = np.zeros((m, D), np.float32)
    b[:, :2] = rng.uniform(-spread, spread, (m, 2))
    b[:, 2] = rng.uniform(-2, 0, m)
    b[:, 3:6] = rng.uniform(1.5, 5.0, (m, 3))
    b[:, 6] = [YAWS[i % 4] for i in range(m)]
    if D == 9:
        b[:, 7:] = rng.uniform(-5, 5, (m, 2))
    return b


def _guarded(dev, n, width, dtype):
    """-> (whole buffer, the view to write): garbage between GUARD sentinel rows on each side"""
    fl = dtype == torch.float32
    shape = (n + 2 * GUARD, width) if width else (n + 2 * GUARD,)
    buf = torch.full(shape, GARBAGE if fl else IGARBAGE, dtype=dtype, device=dev)
    buf[:GUARD] = SENTINEL if fl else ISENTINEL
    buf[GUARD + n:] = SENTINEL if fl else ISENTINEL
    return buf, buf[GUARD:GUARD + n]


def _guards_intact(buf, n):
    host = buf.cpu().numpy()
    s = SENTINEL if host.dtype == np.float32 else ISENTINEL
    assert np.all(host[:GUARD] == s), "rows before the destination overwritten"
    assert np.all(host[GUARD + n:] == s), "rows after the destination overwritten"
    return host[GUARD:GUARD + n]


# ---- points_in_boxes ---------------------------------------------------------------------------------------------
def _pib(dev, pts, boxes, count=None, bop=True, cpb=True):
    """the raw call into guarded outputs, checked against the reference -> (box_of_point, count_per_box)"""
    n, m = pts.shape[0], boxes.shape[0]
    dp, db = torch.from_numpy(pts).to(dev), torch.from_numpy(boxes).to(dev)
    bbuf, bview = _guarded(dev, n, 0, torch.int32)
    cbuf, cview = _guarded(dev, m, 0, torch.int32)
    cnt = None if count is None else torch.tensor([count], dtype=torch.int32, device=dev)
    a = native.PointsInBoxesArgs()
    a.N, a.M, a.F, a.D = n, m, pts.shape[1], boxes.shape[1]
    a.points, a.boxes, a.count_in = native._p(dp), native._p(db), native._p(cnt)
    a.box_of_point = native._p(bview) if bop else None
    a.count_per_box = native._p(cview) if cpb else None
    rc = native.lib().cmt_points_in_boxes(ctypes.byref(a), native._stream())
    assert rc == 0, native.lib().cmt_last_error().decode()
    torch.cuda.synchronize()
    got_b, got_c = _guards_intact(bbuf, n), _guards_intact(cbuf, m)
    want_b, want_c = R.points_in_boxes(pts, boxes, count)
    print(f"points_in_boxes N {n} M {m} count {count}: {int((want_b >= 0).sum())} points inside, "
          f"box_of_point differs at {int((got_b != want_b).sum()) if bop else '-'}, "
          f"count_per_box at {int((got_c != want_c).sum()) if cpb else '-'}")
    if bop:
        assert np.array_equal(got_b, want_b)
    else:
        assert np.all(got_b == IGARBAGE)
    if cpb:
        assert np.array_equal(got_c, want_c)
    else:
        assert np.all(got_c == IGARBAGE)
    return got_b, got_c


@pytest.mark.parametrize("mi", range(4))
@pytest.mark.parametrize("ni", range(6))
def test_pib_sizes(dev, ni, mi):
    T, Cb = _T(), NA.box_chunk()
    n = [0, 1, T - 1, T, T + 1, 2 * T + 1][ni]
    m = [0, 1, Cb, Cb + 1][mi]
    rng = np.random.default_rng(100 + 10 * ni + mi)
    boxes = _boxes(rng, m, D=9 if (ni + mi) % 2 else 7)
    pts = R.inside_inputs(rng, n, boxes, F=(3, 5, 8)[(ni + mi) % 3])
    b, c = _pib(dev, pts, boxes)
    if n > 64 and m > 0:
        assert (b >= 0).sum() > n // 8 and (b < 0).sum() > n // 8
        assert c.sum() >= (b >= 0).sum()


def test_pib_each_yaw(dev):
    """one box per yaw, far apart: each holds its own points"""
    rng = np.random.default_rng(7)
    boxes = _boxes(rng, 4)
    boxes[:, :2] = [[-10, -10], [10, -10], [-10, 10], [10, 10]]
    boxes[:, 3:5] = [4.5, 1.6]
    pts = R.inside_inputs(rng, 600, boxes)
    b, c = _pib(dev, pts, boxes)
    assert (c > 40).all() and np.array_equal(np.bincount(b[b >= 0], minlength=4), c)


def test_pib_overlapping_boxes(dev):
    """the lowest index wins and both counts rise"""
    rng = np.random.default_rng(8)
    boxes = np.array([[5, 5, -1, 4, 2, 1.5, 0.3], [6, 5.5, -1, 4, 2, 2, -2.5], [5, 5, -1, 4, 2, 1.5, 0.3]], np.float32)
    pts = R.inside_inputs(rng, 700, boxes)
    both = R.inside(pts, boxes)[:, :2].all(1)
    assert both.sum() > 10
    b, c = _pib(dev, pts, boxes)
    assert (b[both] == 0).all() and not (b == 2).any() and c[0] == c[2]
    assert c[0] + c[1] == (b == 0).sum() + (b == 1).sum() + both.sum()


def test_pib_degenerate_boxes_and_nan(dev):
    """dx = 0, a NaN point, a NaN box: nothing is inside"""
    rng = np.random.default_rng(9)
    good = np.array([[0, 0, -1, 4, 2, 2, 0.5]], np.float32)
    pts = R.inside_inputs(rng, 300, good)
    boxes = np.repeat(good, 6, 0)
    boxes[0, 3] = 0.0          # no extent
    boxes[1, 4] = -1.0         # a negative extent
    boxes[2, 6] = np.nan
    boxes[3, 0] = np.nan
    boxes[4, 5] = np.nan
    pts[5, 0] = np.nan
    pts[6, 2] = np.nan
    pts[7, 1] = np.inf
    b, c = _pib(dev, pts, boxes)
    assert c[:5].tolist() == [0] * 5 and c[5] > 50 and set(np.unique(b)) == {-1, 5}
    assert (b[5:8] == -1).all()


@pytest.mark.parametrize("count", [0, 1, 700, 5000])
def test_pib_count_in(dev, count):
    rng = np.random.default_rng(10)
    boxes = _boxes(rng, 5)
    pts = R.inside_inputs(rng, _T() + 9, boxes)
    b, c = _pib(dev, pts, boxes, count=count)
    assert (b[min(count, b.size):] == -1).all()
    if count == 0:
        assert not c.any()


def test_pib_each_output_alone_and_wrapper(dev):
    rng = np.random.default_rng(11)
    boxes = _boxes(rng, NA.box_chunk() + 3, D=9)
    pts = R.inside_inputs(rng, _T() + 70, boxes)
    b, _ = _pib(dev, pts, boxes, cpb=False)
    _, c = _pib(dev, pts, boxes, bop=False)
    dp, db = torch.from_numpy(pts).to(dev), torch.from_numpy(boxes).to(dev)
    cnt = torch.tensor([900], dtype=torch.int32, device=dev)
    wb, wc = NA.points_in_boxes(dp, db)
    assert wb.dtype == torch.int32 and wc.dtype == torch.int32
    assert np.array_equal(wb.cpu().numpy(), b) and np.array_equal(wc.cpu().numpy(), c)
    only = NA.points_in_boxes(dp, db, count=cnt, want="count_per_box")
    assert np.array_equal(only.cpu().numpy(), R.points_in_boxes(pts, boxes, 900)[1])
    (first,) = NA.points_in_boxes(dp, db, count=cnt, want=("box_of_point",))
    assert np.array_equal(first.cpu().numpy(), R.points_in_boxes(pts, boxes, 900)[0])


# ---- augment_points ----------------------------------------------------------------------------------------------
def _aug(dev, src, params, count=None, paste=None, paste_boxes=None, paste_first=False, rng=None, order=None,
         workspace=None):
    """the wrapper into a guarded destination, checked against the reference -> (words [n_in, F], count)"""
    n_src, F = src.shape
    n_in = n_src + (0 if paste is None else paste.shape[0])
    buf, out = _guarded(dev, n_in, F, torch.float32)
    cnt = None if count is None else torch.tensor([count], dtype=torch.int32, device=dev)
    kw = {}
    if paste is not None:
        kw = dict(paste_points=torch.from_numpy(paste).to(dev), paste_boxes=torch.from_numpy(paste_boxes).to(dev))
    shuffle = None if order is None else torch.tensor(order, dtype=torch.int32, device=dev)
    got, c = NA.augment_points(torch.from_numpy(src).to(dev), params, count=cnt, paste_first=paste_first,
                               point_cloud_range=rng, shuffle=shuffle, out=out, workspace=workspace, **kw)
    assert got.data_ptr() == out.data_ptr() and tuple(got.shape) == (n_in, F)
    assert c.dtype == torch.int32 and tuple(c.shape) == (1,) and c.device == out.device
    torch.cuda.synchronize()
    words = _guards_intact(buf, n_in).view(np.uint32)
    want = R.augment_points(src, params, count, paste, paste_boxes, paste_first, rng, order)
    k = int(c.item())
    bad = ~_same(words[:k], want.view(np.uint32)) if k == want.shape[0] else None
    print(f"augment_points n_src {n_src} n_paste {n_in - n_src} F {F} K {0 if paste_boxes is None else len(paste_boxes)} "
          f"params {sorted(k_ for k_, v in params.items() if v is not None and v is not False)}: count {k} "
          f"(contract {want.shape[0]}), {'-' if bad is None else int(bad.sum())} kept words differ")
    assert k == want.shape[0]
    assert not bad.any(), f"kept rows differ from the contract at {np.argwhere(bad)[:4].tolist()}"
    assert np.all(words[k:] == R.QNAN), "the tail is not quiet NaN in every column"
    return words, k


def _scene(rng, n_src, F, n_paste, K):
    """-> (src, paste | None, paste_boxes | None): src clear of every paste-box face, paste rows inside the range"""
    boxes = _boxes(rng, K)
    src = R.inside_inputs(rng, n_src, boxes, F=F)
    if n_paste == 0 and K == 0:
        return src, None, None
    paste = np.zeros((n_paste, F), np.float32)
    paste[:, :3] = rng.uniform(-10, 10, (n_paste, 3)) * np.array([1, 1, 0.2])
    paste[:, 3:] = rng.uniform(0, 255, (n_paste, F - 3))
    return src, paste, boxes


@pytest.mark.parametrize("ni", range(5))
@pytest.mark.parametrize("step", sorted(STEPS))
def test_aug_steps_and_sizes(dev, step, ni):
    """each step alone and all together x every size; F, n_paste, paste_first and K cycle with the case"""
    T = _T()
    n_src = [0, 1, T - 1, T + 1, 2 * T + 1][ni]
    k = ni + sorted(STEPS).index(step)
    F, n_paste, K = (3, 5, 8)[k % 3], (0, 7)[k % 2], (0, 1, 33)[(k // 2) % 3]
    rng = np.random.default_rng(200 + 10 * ni + k)
    src, paste, boxes = _scene(rng, n_src, F, n_paste, K)
    words, c = _aug(dev, src, STEPS[step], paste=paste, paste_boxes=boxes, paste_first=bool((k // 3) % 2), rng=RANGE)
    if n_src > 64:
        assert 0 < c < n_src + n_paste


def test_aug_identity_is_a_copy(dev):
    """no step switched on: the input bit for bit, NaN payloads of columns 3 and beyond included"""
    rng = np.random.default_rng(21)
    src = R.inside_inputs(rng, _T() + 5, np.zeros((0, 7), np.float32), F=5)
    src.view(np.uint32)[3, 3] = 0x7FC12345
    src.view(np.uint32)[_T() + 1, 4] = 0xFFA00001
    src[9, 4] = np.inf
    src[10, 3] = -0.0
    words, c = _aug(dev, src, dict(angle=None, scale=None, trans=None, flip_h=False, flip_v=False))
    assert c == src.shape[0] and np.array_equal(words, src.view(np.uint32))
    # with steps on, the feature columns still keep their bits
    words, c = _aug(dev, src, ALL)
    assert c == src.shape[0] and np.array_equal(words[:, 3:], src.view(np.uint32)[:, 3:])


@pytest.mark.parametrize("which", ["zero", "all_but_one"])
def test_aug_count_in(dev, which):
    rng = np.random.default_rng(22)
    n_src = _T() + 1
    src, paste, boxes = _scene(rng, n_src, 5, 7, 1)
    count = 0 if which == "zero" else n_src - 1
    for first in (False, True):
        words, c = _aug(dev, src, ALL, count=count, paste=paste, paste_boxes=boxes, paste_first=first, rng=RANGE)
        if count == 0:
            assert c <= 7


@pytest.mark.parametrize("kind", ["reversed", "permutation", "out_of_range"])
def test_aug_order(dev, kind):
    rng = np.random.default_rng(23)
    n_src = 2 * _T() + 1
    src, paste, boxes = _scene(rng, n_src, 5, 7, 33)
    n_in = n_src + 7
    if kind == "reversed":
        order = np.arange(n_in)[::-1].copy()
    else:
        order = np.random.default_rng(5).permutation(n_in)
    if kind == "out_of_range":
        order[[0, 70, _T(), n_in - 1]] = [n_in, -1, 2 ** 31 - 1, -2 ** 31]
    _aug(dev, src, ALL, count=n_src - 40, paste=paste, paste_boxes=boxes, paste_first=True, rng=RANGE, order=order)


def test_aug_every_row_dropped(dev):
    rng = np.random.default_rng(24)
    src, _, _ = _scene(rng, _T() + 1, 5, 0, 0)
    words, c = _aug(dev, src, dict(trans=[100.0, 0, 0]), rng=RANGE)
    assert c == 0 and np.all(words == R.QNAN)
    # and by one paste box that covers the cloud
    box = np.array([[0, 0, -50, 200, 200, 100, 0.4]], np.float32)
    words, c = _aug(dev, src, {}, paste=np.zeros((0, 5), np.float32), paste_boxes=box)
    assert c == 0 and np.all(words == R.QNAN)


def test_aug_more_tiles_than_threads(dev):
    """257 tiles and one slot, one kept row per tile and the last: a thread of the scatter launch sums more than
    one entry of the tiles' counts"""
    T = _T()
    n = 257 * T + 1
    keep = np.zeros(n, bool)
    keep[T - 1::T] = True
    keep[-1] = True
    src = np.zeros((n, 4), np.float32)
    src[:, 0] = np.where(keep, 1.0, 100.0)      # inside RANGE where kept
    src[:, 1] = (np.arange(n) % 61) * 0.5 - 15
    src[:, 2] = -1.0
    src[:, 3] = np.arange(n)
    words, c = _aug(dev, src, {}, rng=RANGE)
    assert c == 258
    assert np.array_equal(words[:c, 3].view(np.float32), np.flatnonzero(keep).astype(np.float32))   # input order


def test_aug_workspace_reuse(dev):
    """two different calls through one workspace, nothing cleaned between them; a caller's dirty tensor"""
    rng = np.random.default_rng(25)
    ws = NA.PointsWorkspace()
    a = _scene(rng, 2 * _T() + 1, 5, 7, 33)
    b = _scene(rng, _T() - 1, 8, 0, 1)
    w1, c1 = _aug(dev, a[0], ALL, paste=a[1], paste_boxes=a[2], rng=RANGE, workspace=ws)
    _aug(dev, b[0], STEPS["rot"], paste=b[1], paste_boxes=b[2], rng=RANGE, workspace=ws)
    w2, c2 = _aug(dev, a[0], ALL, paste=a[1], paste_boxes=a[2], rng=RANGE, workspace=ws)
    assert c1 == c2 and np.array_equal(w1, w2)
    raw = torch.full((64,), -1, dtype=torch.int32, device=dev)
    w3, c3 = _aug(dev, a[0], ALL, paste=a[1], paste_boxes=a[2], rng=RANGE, workspace=raw)
    assert c3 == c1 and np.array_equal(w3, w1)
    with pytest.raises(ValueError, match="workspace"):
        NA.augment_points(torch.from_numpy(a[0]).to(dev), ALL, workspace=raw[:2])


def test_aug_voxelize_batch(dev):
    """the padded pair voxelizes like the trimmed rows"""
    from projects.mmdet3d_plugin.mmcv_custom.ops.voxel import SPConvVoxelization
    from projects.mmdet3d_plugin.mmcv_custom.ops.voxel.spconv_voxelize import voxelize_batch
    rng = np.random.default_rng(26)
    src, paste, boxes = _scene(rng, 2 * _T() + 1, 5, 7, 33)
    padded, count = NA.augment_points(torch.from_numpy(src).to(dev), ALL, paste_points=torch.from_numpy(paste).to(dev),
                                      paste_boxes=torch.from_numpy(boxes).to(dev), point_cloud_range=RANGE,
                                      shuffle=torch.Generator(device=dev).manual_seed(3))
    c = int(count.item())
    assert 0 < c < padded.shape[0] and torch.isnan(padded[c:]).all() and torch.isfinite(padded[:c]).all()
    layer = SPConvVoxelization(voxel_size=[0.5, 0.5, 6.0], point_cloud_range=RANGE, max_num_points=3,
                               max_voxels=(400, 400), num_point_features=5).eval()
    a = [t.clone() for t in voxelize_batch(layer, [padded])]
    b = [t.clone() for t in voxelize_batch(layer, [padded[:c].contiguous()])]
    assert a[0].shape[0] > 20
    for x, y, name in zip(a, b, ("features", "num_points", "coors")):
        assert torch.equal(x, y), name


def test_aug_generator_shuffle(dev):
    """the same seed gives the same bytes; the kept rows are the unshuffled call's, in another order"""
    rng = np.random.default_rng(27)
    src, paste, boxes = _scene(rng, _T() + 1, 5, 7, 1)
    dsrc, dpaste, dboxes = (torch.from_numpy(x).to(dev) for x in (src, paste, boxes))

    def run(shuffle):
        p, c = NA.augment_points(dsrc, ALL, paste_points=dpaste, paste_boxes=dboxes, point_cloud_range=RANGE,
                                 shuffle=shuffle)
        return p.cpu().numpy().view(np.uint32), int(c.item())
    plain, c0 = run(None)
    s1, c1 = run(torch.Generator(device=dev).manual_seed(11))
    s2, c2 = run(torch.Generator(device=dev).manual_seed(11))
    s3, c3 = run(torch.Generator().manual_seed(11))            # a host generator: drawn there, copied over
    assert c0 == c1 == c2 == c3 and np.array_equal(s1, s2)
    assert not np.array_equal(s1[:c1], plain[:c0])
    for s in (s1, s3):
        assert np.all(s[c1:] == R.QNAN)
        assert sorted(map(bytes, s[:c1])) == sorted(map(bytes, plain[:c0]))


# ---- augment_boxes -----------------------------------------------------------------------------------------------
def _run_boxes(dev, boxes, labels, params, rng, num_classes, gravity, split=None):
    n, D = boxes.shape
    db, dl = torch.from_numpy(boxes).to(dev), torch.from_numpy(labels).to(dev)
    if split is None:
        ob, ol, c = NA.augment_boxes(db, dl, params, point_cloud_range=rng, num_classes=num_classes, gravity=gravity)
    else:
        ob, ol, c = NA.augment_boxes(db[:split].contiguous(), dl[:split].contiguous(), params,
                                     paste_boxes=db[split:].contiguous(), paste_labels=dl[split:].contiguous(),
                                     point_cloud_range=rng, num_classes=num_classes, gravity=gravity)
    torch.cuda.synchronize()
    assert tuple(ob.shape) == (n, D) and tuple(ol.shape) == (n,) and ol.dtype == torch.int64 and c.dtype == torch.int32
    k = int(c.item())
    want_b, want_l = R.augment_boxes(boxes, labels, params, rng, num_classes, gravity)
    words, labs = ob.cpu().numpy().view(np.uint32), ol.cpu().numpy()
    bad = ~_same(words[:k], want_b.view(np.uint32)) if k == want_b.shape[0] else None
    print(f"augment_boxes n {n} D {D} gravity {gravity}: count {k} (contract {want_b.shape[0]}), "
          f"{'-' if bad is None else int(bad.sum())} kept words differ")
    assert k == want_b.shape[0]
    assert not bad.any(), f"kept boxes differ from the contract at {np.argwhere(bad)[:4].tolist()}"
    assert np.array_equal(labs[:k], want_l)
    assert np.all(words[k:] == R.QNAN) and np.all(labs[k:] == -1)
    return words, labs, k


@pytest.mark.parametrize("D", [7, 9])
@pytest.mark.parametrize("n", [0, 1, 64, 65, 300])
def test_boxes_sizes(dev, n, D):
    rng = np.random.default_rng(300 + n + D)
    boxes = _boxes(rng, n, D=D, spread=21.0)                    # some centres beyond the BEV range
    boxes[:, 6] = rng.uniform(-7, 7, n)
    labels = rng.integers(-1, 5, n).astype(np.int64)            # -1 and num_classes = 4 are dropped
    gravity = bool((n + D) % 2)
    for params in (ALL, STEPS["flip_v"], {}):
        words, labs, k = _run_boxes(dev, boxes, labels, params, RANGE, 4, gravity)
    if n >= 64:
        assert 0 < k < n
    _run_boxes(dev, boxes, labels, ALL, None, 4, not gravity, split=n // 2)


def test_boxes_bev_edges_and_labels(dev):
    rows = []
    for col, face in ((0, RANGE[0]), (0, RANGE[3]), (1, RANGE[1]), (1, RANGE[4])):
        on = np.array([1.0, 2.0, 0.0, 1, 1, 1, 0.5, 0.1, 0.2], np.float32)
        on[col] = face
        just_in = on.copy()
        just_in[col] = np.nextafter(np.float32(face), np.float32(0))
        rows += [on, just_in]
    rows.append(np.array([1.0, 2.0, 100.0, 1, 1, 1, 3 * np.pi, 0, 0], np.float32))   # z is not tested; yaw wraps
    boxes = np.stack(rows)
    _, labs, k = _run_boxes(dev, boxes, np.arange(9, dtype=np.int64), {}, RANGE, 9, False)
    assert labs[:k].tolist() == [1, 3, 5, 7, 8]
    _, labs, k = _run_boxes(dev, boxes, np.array([0, -1, 3, 2, 1, 0, -5, 2 ** 40, 0], np.int64), {}, None, 3, True)
    assert labs[:k].tolist() == [0, 2, 1, 0, 0]


# ---- raw-struct rejections: CMT_EINVAL, cmt_last_error set, nothing written -------------------------------------
def _aug_args(dev, keep):
    """a valid cmt_pts_augment call on 100 + 7 rows with 2 paste boxes; ``keep`` holds the tensors alive"""
    t = dict(src=torch.zeros((100, 5), device=dev), paste=torch.zeros((7, 5), device=dev),
             boxes=torch.ones((2, 7), device=dev), dst=torch.full((107, 5), GARBAGE, device=dev),
             count=torch.full((1,), IGARBAGE, dtype=torch.int32, device=dev),
             ws=torch.full((16,), IGARBAGE, dtype=torch.int32, device=dev))
    keep.update(t)
    a = native.PtsAugmentArgs()
    a.n_src, a.n_paste, a.F, a.K = 100, 7, 5, 2
    a.src, a.paste, a.paste_boxes = native._p(t["src"]), native._p(t["paste"]), native._p(t["boxes"])
    a.dst, a.count, a.workspace, a.workspace_bytes = native._p(t["dst"]), native._p(t["count"]), native._p(t["ws"]), 64
    a.xf.has_rot, a.xf.has_scale, a.xf.has_trans, a.xf.has_range = 1, 1, 1, 1
    a.xf.rot32[:] = [1, 0, 0, 0, 1, 0, 0, 0, 1]
    a.xf.scale = 1.0
    a.xf.range[:] = RANGE
    return a


def _set(a, **kw):
    for k, v in kw.items():
        obj = a
        *path, leaf = k.split("__")
        for p in path:
            obj = getattr(obj, p)
        if isinstance(v, tuple):
            getattr(obj, leaf)[v[0]] = v[1]
        else:
            setattr(obj, leaf, v)


AUG_REJECTS = {
    "K above the limit": (dict(K=129), "K must be"),
    "K negative": (dict(K=-1), "K must be"),
    "F 2": (dict(F=2), "F must be"),
    "F 9": (dict(F=9), "F must be"),
    "rotation nan": (dict(xf__rot32=(4, float("nan"))), "non-finite rotation"),
    "angle inf": (dict(xf__angle32=float("inf")), "non-finite rotation"),
    "scale nan": (dict(xf__scale=float("nan")), "non-finite scale"),
    "translation inf": (dict(xf__trans32=(2, float("-inf"))), "non-finite translation"),
    "range nan": (dict(xf__range=(1, float("nan"))), "non-finite range"),
    "range min >= max": (dict(xf__range=(3, -18.0)), "range min"),
    "n_src negative": (dict(n_src=-1), "negative"),
    "n_in 2^31": (dict(n_src=2 ** 31 - 7), "2^31"),
    "shift_height": (dict(shift_height=1), "shift_height"),
    "null src": (dict(src=None), "src must be"),
    "null paste": (dict(paste=None), "paste must be"),
    "null paste_boxes": (dict(paste_boxes=None), "paste_boxes must be"),
    "null dst": (dict(dst=None), "dst must be"),
    "null count": (dict(count=None), "count must be"),
    "null workspace": (dict(workspace=None), "workspace must be"),
    "workspace too small": (dict(workspace_bytes=3), "workspace below"),
}


@pytest.mark.parametrize("case", sorted(AUG_REJECTS) + ["misaligned dst", "misaligned order"])
def test_pts_augment_rejects(dev, case):
    keep = {}
    a = _aug_args(dev, keep)
    if case == "misaligned dst":
        a.dst, text = keep["dst"].data_ptr() + 2, "dst must be"
    elif case == "misaligned order":
        a.order, text = keep["ws"].data_ptr() + 1, "order"
    else:
        kw, text = AUG_REJECTS[case]
        _set(a, **kw)
    L = native.lib()
    rc = L.cmt_pts_augment(ctypes.byref(a), native._stream())
    msg = L.cmt_last_error().decode()
    torch.cuda.synchronize()
    assert rc == EINVAL, f"{case}: status {rc}"
    assert text in msg and "cmt_pts_augment" in msg, f"{case}: {msg!r}"
    assert (keep["dst"] == GARBAGE).all() and int(keep["count"].item()) == IGARBAGE and (keep["ws"] == IGARBAGE).all()


def test_switched_off_transforms_may_be_non_finite(dev):
    keep = {}
    a = _aug_args(dev, keep)
    a.xf.has_rot = a.xf.has_scale = a.xf.has_trans = a.xf.has_range = 0
    a.xf.rot32[0] = a.xf.scale = a.xf.trans32[0] = a.xf.range[0] = float("nan")
    a.K = 0
    assert native.lib().cmt_pts_augment(ctypes.byref(a), native._stream()) == 0
    torch.cuda.synchronize()
    assert int(keep["count"].item()) == 107 and (keep["dst"] == 0).all()


def test_other_calls_reject(dev):
    L = native.lib()
    pts, boxes = torch.zeros((10, 5), device=dev), torch.ones((3, 9), device=dev)
    out = torch.full((10,), IGARBAGE, dtype=torch.int32, device=dev)

    def pib(**kw):
        a = native.PointsInBoxesArgs()
        a.N, a.M, a.F, a.D = 10, 3, 5, 9
        a.points, a.boxes, a.box_of_point = native._p(pts), native._p(boxes), native._p(out)
        _set(a, **kw)
        return L.cmt_points_in_boxes(ctypes.byref(a), native._stream()), L.cmt_last_error().decode()
    for kw, text in ((dict(F=2), "F must be"), (dict(F=9), "F must be"), (dict(D=8), "D must be"), (dict(N=-1), "N must be"),
                     (dict(M=-1), "M must be"), (dict(points=None), "points must be"), (dict(boxes=None), "boxes must be"),
                     (dict(box_of_point=out.data_ptr() + 2), "4-byte aligned")):
        rc, msg = pib(**kw)
        assert rc == EINVAL and text in msg and "cmt_points_in_boxes" in msg, (kw, msg)
    assert pib()[0] == 0
    torch.cuda.synchronize()
    assert (out == -1).all()                                   # the origin lies below the boxes' z_bottom = 1
    ob = torch.full((3, 9), GARBAGE, device=dev)
    lab = torch.zeros(3, dtype=torch.int64, device=dev)
    ol = torch.full((3,), IGARBAGE, dtype=torch.int64, device=dev)
    cnt = torch.full((1,), IGARBAGE, dtype=torch.int32, device=dev)

    def bx(**kw):
        a = native.BoxesAugmentArgs()
        a.n, a.D, a.num_classes = 3, 9, 2
        a.boxes, a.labels, a.out_boxes, a.out_labels, a.count = (native._p(boxes), native._p(lab), native._p(ob),
                                                                 native._p(ol), native._p(cnt))
        _set(a, **kw)
        return L.cmt_boxes_augment(ctypes.byref(a), native._stream()), L.cmt_last_error().decode()
    for kw, text in ((dict(n=-1), "n must be"), (dict(n=65537), "n must be"), (dict(D=8), "D must be"),
                     (dict(num_classes=-1), "num_classes"), (dict(count=None), "count must be"),
                     (dict(labels=None), "labels"), (dict(out_labels=ol.data_ptr() + 4), "8-byte aligned"),
                     (dict(out_boxes=None), "out_boxes"), (dict(xf__has_scale=1, xf__scale=float("inf")), "non-finite scale"),
                     (dict(xf__has_range=1), "range min")):
        rc, msg = bx(**kw)
        assert rc == EINVAL and text in msg and "cmt_boxes_augment" in msg, (kw, msg)
    torch.cuda.synchronize()
    assert (ob == GARBAGE).all() and (ol == IGARBAGE).all() and int(cnt.item()) == IGARBAGE
    assert bx()[0] == 0
    torch.cuda.synchronize()
    assert int(cnt.item()) == 3


def test_cli_count_gt_points(dev, capsys):
    """tools/test.py --eval nds --count-gt-points in this process: gt_num_pts comes from points_in_boxes over the
    frame's cloud; without the flag the nds line has no such entry"""
    import importlib.util
    import json
    import os
    from conftest import PKG
    from projects.mmdet3d_plugin import synthetic as S
    spec = importlib.util.spec_from_file_location("cmt_test_cli_aug", os.path.join(PKG, "tools", "test.py"))
    cli = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(cli)
    base = ["cmt_lidar_nus", "--synthetic", "--num-query", "32", "--num-layers", "1", "--grid", "16", "16",
            "--points", "3000", "--eval", "nds"]
    assert cli.main(base + ["--count-gt-points"]) == 0
    with_flag = json.loads(capsys.readouterr().out.strip().splitlines()[-1])
    assert cli.main(base) == 0
    without = json.loads(capsys.readouterr().out.strip().splitlines()[-1])
    assert "gt_without_points" not in without and set(with_flag) - set(without) == {"gt_without_points"}
    # the same count from the float64 reference on the same synthetic frame
    pcr = cli.eval_pc_range("cmt_lidar_nus")
    gb, _ = cli.frame_ground_truth(0, 0, pcr, 10)
    lidar = gb[:, :7].clone()
    lidar[:, 2] -= lidar[:, 5] * 0.5
    pts = S.synthetic_points(3000, pcr, seed=0)
    _, per_box = R.points_in_boxes(pts.numpy(), lidar.numpy())
    # the condition on the inputs: no point of this seeded frame lies within the contract's margin of a face
    d, m = R.face_distances(pts.numpy(), lidar.numpy()), R.margin(pts.numpy(), lidar.numpy())[..., None]
    assert not ((d > -m).all(-1) & (np.abs(d) < m).any(-1)).any()
    assert 0 < int((per_box == 0).sum()) < 20
    assert with_flag["gt_without_points"] == int((per_box == 0).sum())
    with pytest.raises(SystemExit):
        cli.main(base[:-2] + ["--eval", "bbox", "--count-gt-points"])


def test_graph_capture(dev):
    """no allocation, no synchronisation inside: the three calls replay from a HIP graph on new data"""
    rng = np.random.default_rng(28)
    src, paste, boxes = _scene(rng, _T() + 1, 5, 7, 33)
    src2 = R.inside_inputs(rng, _T() + 1, boxes, F=5)
    dsrc, dpaste, dboxes = (torch.from_numpy(x).to(dev) for x in (src, paste, boxes))
    n_in = src.shape[0] + 7
    out = torch.zeros((n_in, 5), device=dev)
    ws = torch.empty(16, dtype=torch.int32, device=dev)
    order = torch.from_numpy(np.random.default_rng(1).permutation(n_in).astype(np.int32)).to(dev)
    kw = dict(paste_points=dpaste, paste_boxes=dboxes, point_cloud_range=RANGE, shuffle=order, out=out, workspace=ws)
    stream = torch.cuda.Stream()
    stream.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(stream):
        NA.augment_points(dsrc, ALL, **kw)
        NA.points_in_boxes(dsrc, dboxes)
    torch.cuda.current_stream().wait_stream(stream)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        _, count = NA.augment_points(dsrc, ALL, **kw)
        bop, cpb = NA.points_in_boxes(dsrc, dboxes)
    dsrc.copy_(torch.from_numpy(src2))
    out.fill_(GARBAGE)
    graph.replay()
    torch.cuda.synchronize()
    want = R.augment_points(src2, ALL, None, paste, boxes, False, RANGE, order.cpu().numpy())
    assert int(count.item()) == want.shape[0]
    assert np.array_equal(out.cpu().numpy().view(np.uint32), R.padded(want, n_in, 5))
    wb, wc = R.points_in_boxes(src2, boxes)
    assert np.array_equal(bop.cpu().numpy(), wb) and np.array_equal(cpb.cpu().numpy(), wc)
