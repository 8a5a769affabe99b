"""cmt_gtdb_extract, cmt_gtdb_gather and cmt_gtdb_collide on the GPU against the numpy contract of tests/_gtdb_ref.py,
and GtDatabase / UnifiedDataBaseSampler end to end against the numpy chain of _gtdb_ref and _aug_ref.

Every destination is pre-filled with a finite garbage value and has sentinel rows on both sides.  The extraction's
and the gather's arithmetic is one IEEE float32 subtraction or addition per value, so rows are compared bit for bit;
the inside test binds only points clear of every face, which ``_aug_ref.inside_inputs`` builds and asserts.  The
collision test binds only scenes whose float64 evaluation has no comparison within ``tol``; the tests assert that
margin (hand-made scenes) or skip the scene (random ones, at most 24 of 60).  Shapes are the smallest at which the
kernels take another path: around the tile T and the box chunk Cb.
"""
import ctypes
import types

import numpy as np
import pytest
import torch

import _aug_ref as A
import _gtdb_ref as G
from projects.mmdet3d_plugin import native
from projects.mmdet3d_plugin import native_aug as NA
from projects.mmdet3d_plugin import native_gtdb as NG
from projects.mmdet3d_plugin import native_imgaug as NI

pytestmark = pytest.mark.gpu

GARBAGE = 777.25
SENTINEL = -12345.5
IGARBAGE = 7777
ISENTINEL = -424242
GUARD = 3
YAWS = [0.0, np.pi / 2, -2.5, 7.0]
RANGE = [-18.0, -18.0, -4.0, 18.0, 18.0, 4.0]


def _boxes(rng, m, D=7, spread=12.0):
    b = np.zeros((m, D), np.float32)
    b[:, :2] = rng.uniform(-spread, spread, (m, 2))
    b[:, 2] = rng.uniform(-2, 0, m)
    b[:, 3:6] = rng.uniform(1.5, 5.0, (m, 3))
    b[:, 6] = [YAWS[i % 4] for i in range(m)]
    if D == 9:
        b[:, 7:] = rng.uniform(-5, 5, (m, 2))
    return b


def _guarded(dev, n, width, dtype):
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


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


# ---- extract -----------------------------------------------------------------------------------------------------
def _extract(dev, pts, boxes, count=None, cap=None):
    """the raw call into guarded outputs and an exact, guarded workspace, checked against the reference
    -> (rows [cap, F], offsets [M + 1]) as numpy"""
    n, m, F = pts.shape[0], boxes.shape[0], pts.shape[1]
    want_rows, want_off = G.extract(pts, boxes, count)
    total = int(want_off[-1])
    cap = total if cap is None else cap
    dp, db = torch.from_numpy(pts).to(dev), torch.from_numpy(boxes).to(dev)
    rbuf, rview = _guarded(dev, cap, F, torch.float32)
    obuf, oview = _guarded(dev, m + 1, 0, torch.int32)
    need = NG.workspace_bytes(n, m)
    assert need % 4 == 0
    wbuf, wview = _guarded(dev, need // 4, 0, torch.int32)
    cnt = None if count is None else torch.tensor([count], dtype=torch.int32, device=dev)
    a = native.GtdbExtractArgs()
    a.N, a.cap, a.M, a.F, a.D = n, cap, m, F, boxes.shape[1]
    a.points, a.count_in, a.boxes = native._p(dp), native._p(cnt), native._p(db)
    a.rows, a.offsets = native._p(rview), native._p(oview)
    a.workspace, a.workspace_bytes = (native._p(wview) if need else None), need
    rc = native.lib().cmt_gtdb_extract(ctypes.byref(a), native._stream())
    assert rc == 0, native.lib().cmt_last_error().decode()
    torch.cuda.synchronize()
    got_rows, got_off = _guards_intact(rbuf, cap), _guards_intact(obuf, m + 1)
    _guards_intact(wbuf, need // 4)
    k = min(total, cap)
    bad = int((_bits(got_rows[:k]) != _bits(want_rows[:k])).any(1).sum()) if k else 0
    print(f"extract N {n} M {m} F {F} D {boxes.shape[1]} count {count} cap {cap}: total {total}, offsets differ at "
          f"{int((got_off != want_off).sum())}, rows differ at {bad}")
    assert np.array_equal(got_off, want_off)
    assert bad == 0
    assert np.all(got_rows[k:] == GARBAGE), "a row at or beyond min(total, cap) was written"
    return got_rows, got_off


@pytest.mark.parametrize("mi", range(6))
@pytest.mark.parametrize("ni", range(6))
def test_extract_sizes(dev, ni, mi):
    T, Cb = NA.tile_rows(), NA.box_chunk()
    n = [0, 1, T - 1, T, T + 1, 2 * T + 1][ni]
    m = [0, 1, Cb - 1, Cb, Cb + 1, 2 * Cb + 1][mi]
    rng = np.random.default_rng(300 + 10 * ni + mi)
    boxes = _boxes(rng, m, D=9 if (ni + mi) % 2 else 7)
    pts = A.inside_inputs(rng, n, boxes, F=(3, 5, 8)[(ni + mi) % 3])
    rows, off = _extract(dev, pts, boxes)
    if n > 64 and m > 0:
        assert off[-1] > n // 8
    if n > 64 and m > 1:
        assert off[-1] > A.inside(pts, boxes).any(1).sum()      # boxes overlap: some rows are in two segments


def test_extract_overlapping_boxes(dev):
    """a row inside two boxes appears in both segments, moved to each box's own centre"""
    rng = np.random.default_rng(8)
    boxes = np.array([[5, 5, -1, 4, 2, 1.5, 0.3], [6, 5.5, -1, 4, 2, 2, -2.5], [5, 5, -1, 4, 2, 1.5, 0.3]], np.float32)
    pts = A.inside_inputs(rng, 700, boxes)
    both = A.inside(pts, boxes)[:, :2].all(1)
    assert both.sum() > 10
    rows, off = _extract(dev, pts, boxes)
    assert off[1] - off[0] == off[3] - off[2] and off[3] > 700 // 2
    assert np.array_equal(_bits(rows[off[0]:off[1]]), _bits(rows[off[2]:off[3]]))


@pytest.mark.parametrize("count", [-1, 0, 517, 5000])
def test_extract_count_in(dev, count):
    rng = np.random.default_rng(21)
    boxes = _boxes(rng, 3)
    pts = A.inside_inputs(rng, NA.tile_rows() + 1, boxes)
    _, off = _extract(dev, pts, boxes, count=count)
    assert (off[-1] == 0) == (count <= 0)


def test_extract_nan_and_flat_boxes(dev):
    """NaN points are in no box; a NaN box and a box with dz <= 0 hold nothing"""
    rng = np.random.default_rng(22)
    good = _boxes(rng, 4)
    pts = A.inside_inputs(rng, 1500, good)
    pts[::7, 0] = np.nan
    pts[3::11, 2] = np.nan
    nanbox, flat, neg = good[0].copy(), good[1].copy(), good[2].copy()
    nanbox[6] = np.nan
    flat[5] = 0.0
    neg[5] = -1.0
    boxes = np.stack([good[0], nanbox, good[1], flat, neg, good[2], good[3]])
    _, off = _extract(dev, pts, boxes)
    d = np.diff(off)
    assert d[1] == d[3] == d[4] == 0 and (d[[0, 2, 5, 6]] > 20).all()


def test_extract_cap_below_total(dev):
    rng = np.random.default_rng(23)
    boxes = _boxes(rng, 70, spread=8.0)
    pts = A.inside_inputs(rng, 2 * NA.tile_rows() + 1, boxes)
    total = int(G.extract(pts, boxes)[1][-1])
    for cap in (0, 1, total // 2, total - 1):
        _extract(dev, pts, boxes, cap=cap)
    _extract(dev, pts, boxes, cap=total + 5)


def test_extract_counts_and_repeatability(dev):
    """diff(offsets) is cmt_points_in_boxes' count_per_box; two runs through the wrapper are bit-equal"""
    rng = np.random.default_rng(24)
    boxes = _boxes(rng, 66, D=9)
    pts = A.inside_inputs(rng, 3000, boxes, F=5)
    dp, db = torch.from_numpy(pts).to(dev), torch.from_numpy(boxes).to(dev)
    want_rows, want_off = G.extract(pts, boxes)
    out1 = torch.full((int(want_off[-1]) + 4, 5), GARBAGE, device=dev)
    out2 = out1.clone()
    r1, o1 = NG.extract_objects(dp, db, out=out1)
    r2, o2 = NG.extract_objects(dp, db, out=out2, workspace=torch.empty(NG.workspace_bytes(3000, 66) // 4, dtype=torch.int32, device=dev))
    cpb = NA.points_in_boxes(dp, db, want="count_per_box")
    torch.cuda.synchronize()
    assert r1.data_ptr() == out1.data_ptr()
    assert torch.equal(o1[1:] - o1[:-1], cpb) and np.array_equal(o1.cpu().numpy(), want_off)
    assert torch.equal(r1.view(torch.int32), r2.view(torch.int32)) and torch.equal(o1, o2)
    assert np.array_equal(_bits(r1[:want_off[-1]].cpu().numpy()), _bits(want_rows))
    # the default destination holds N rows
    r3, o3 = NG.extract_objects(dp[:100], db[:1])
    assert tuple(r3.shape) == (100, 5) and tuple(o3.shape) == (2,)


# ---- gather ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("K,F", [(0, 5), (1, 3), (7, 8), (128, 5)])
def test_gather(dev, K, F):
    rng = np.random.default_rng(40 + K)
    R = 6000
    rows = rng.uniform(-30, 30, (R, F)).astype(np.float32)
    lens = rng.integers(0, 90, K).astype(np.int32)
    if K > 2:
        lens[1] = 0                                            # an empty segment
        lens[2] = 5000                                         # more rows than the segment's workgroups cover in one pass
    seg = np.array([rng.integers(0, R - int(n) + 1) for n in lens], np.int32)
    centre = rng.uniform(-40, 40, (K, 3)).astype(np.float32)
    dst_off = np.concatenate([[0], np.cumsum(lens)]).astype(np.int32)
    n_dst = int(dst_off[-1])
    want = G.gather(rows, seg, lens, centre)
    buf, view = _guarded(dev, n_dst, F, torch.float32)
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    got = NG.gather_objects(t(rows), t(seg), t(lens), t(dst_off[:-1]), t(centre).reshape(K, 3), n_dst, out=view)
    torch.cuda.synchronize()
    assert got.data_ptr() == view.data_ptr()
    host = _guards_intact(buf, n_dst)
    bad = int((_bits(host) != _bits(want)).any(1).sum()) if n_dst else 0
    print(f"gather K {K} F {F}: {n_dst} rows, {bad} differ")
    assert bad == 0


def test_gather_tables_outside_their_buffers(dev):
    """a source row beyond ``rows`` or a destination row beyond ``dst`` moves nothing; the rest arrives"""
    rows = np.arange(40, dtype=np.float32).reshape(10, 4)
    t = lambda a, dt: torch.tensor(a, dtype=dt, device=dev)
    buf, view = _guarded(dev, 6, 4, torch.float32)
    NG.gather_objects(t(rows, torch.float32), t([8, 0, -1], torch.int32), t([4, 5, 1], torch.int32),
                      t([0, 4, 2], torch.int32), torch.zeros((3, 3), device=dev), 6, out=view)
    torch.cuda.synchronize()
    host = _guards_intact(buf, 6)
    assert np.array_equal(host[0], rows[8]) and np.array_equal(host[1], rows[9])      # rows 10, 11 do not exist
    assert np.all(host[2:4] == GARBAGE)
    assert np.array_equal(host[4], rows[0]) and np.array_equal(host[5], rows[1])      # destination rows 6.. do not


# ---- collide -----------------------------------------------------------------------------------------------------
def _collide(dev, boxes, n_gt, group):
    n_s = boxes.shape[0] - n_gt
    kbuf, kview = _guarded(dev, n_s, 0, torch.int32)
    cbuf, cview = _guarded(dev, 1, 0, torch.int32)
    g = np.ascontiguousarray(group, np.int32)
    db = torch.from_numpy(np.ascontiguousarray(boxes)).to(dev)
    a = native.GtdbCollideArgs()
    a.n_gt, a.n_s, a.D = n_gt, n_s, boxes.shape[1]
    a.boxes, a.group, a.keep, a.count = native._p(db), ctypes.c_void_p(g.ctypes.data), native._p(kview), native._p(cview)
    rc = native.lib().cmt_gtdb_collide(ctypes.byref(a), native._stream())
    assert rc == 0, native.lib().cmt_last_error().decode()
    torch.cuda.synchronize()
    return _guards_intact(kbuf, n_s), int(_guards_intact(cbuf, 1)[0])


def test_collide_hand_scenes(dev):
    for name, (boxes, n_gt, group, want) in G.hand_scenes().items():
        keep, count, margin = G.collide(boxes, n_gt, group)
        assert margin > G.tol(boxes) and keep.tolist() == want.tolist(), name
        got, cnt = _collide(dev, boxes, n_gt, group)
        print(f"collide {name}: margin {margin:.3g} tol {G.tol(boxes):.3g} keep {got.tolist()}")
        assert got.tolist() == want.tolist() and cnt == int(want.sum()), name
    # nine-column boxes and the wrapper
    boxes, n_gt, group, want = G.hand_scenes()["rejected_of_earlier_group"]
    nine = np.concatenate([boxes, np.full((boxes.shape[0], 2), 3.0, np.float32)], 1)
    keep, cnt = NG.collide(torch.from_numpy(nine).to(dev), n_gt, group.tolist())
    assert keep.cpu().tolist() == want.tolist() and int(cnt) == int(want.sum())
    # exact copies, every value dyadic and yaw 0: float32 evaluates the reference's ties exactly, and its strict
    # comparisons say "no collision" (tests/test_gtdb_host.py works this out)
    got, cnt = _collide(dev, G.IDENTICAL, 1, [0])
    assert got.tolist() == [1] and cnt == 1
    # no candidates: count alone
    got, cnt = _collide(dev, G.IDENTICAL, 2, [])
    assert cnt == 0 and got.shape == (0,)


def test_collide_random_scenes(dev):
    rs = np.random.RandomState(0)
    skipped = wrong = 0
    for i in range(60):
        boxes, n_gt, group = G.random_scene(rs)
        keep, count, margin = G.collide(boxes, n_gt, group)
        if margin <= G.tol(boxes):
            skipped += 1
            continue
        got, cnt = _collide(dev, boxes, n_gt, group)
        ok = got.tolist() == keep.tolist() and cnt == count
        wrong += not ok
        print(f"scene {i}: n_gt {n_gt} n_s {len(group)} margin {margin:.3g} tol {G.tol(boxes):.3g} kept {count} "
              f"{'ok' if ok else 'DIFFERS ' + str(np.nonzero(got != keep)[0].tolist())}")
    print(f"{skipped} of 60 scenes skipped (a comparison within tol)")
    assert skipped <= 24
    assert wrong == 0


def test_collide_at_the_cap(dev):
    """n = 512, one group, every candidate crossing every other: the first is rejected (the later ones are live), and
    so on down to the last, which is kept.  Exact copies would NOT do: the reference's strict comparisons see no
    collision between identical rectangles.  So candidate k is the same 20 x 10 m box moved by (k / 32, k / 64):
    any two are offset along both axes by less than their extents and their edges cross; with yaw 0 every corner,
    difference and product is exact in float32, so no tolerance is involved."""
    n = 512
    b = np.zeros((n, 7), np.float32)
    b[:, 0], b[:, 1] = np.arange(n) / 32.0, np.arange(n) / 64.0
    b[:, 2:6] = [-1.0, 20.0, 10.0, 1.5]
    sub = b[::37]                                               # the reference on a sample: all pairs collide
    mat, _ = G.collision_rows(sub, 0)
    assert mat.sum() == len(sub) * (len(sub) - 1)
    got, cnt = _collide(dev, b, 0, np.zeros(n, np.int32))
    assert got.tolist() == [0] * (n - 1) + [1] and cnt == 1
    # each in a group of its own, behind one box to avoid that touches none of them: the first is kept and every
    # later one collides with it
    far = np.array([[500.0, 500.0, -1.0, 2.0, 2.0, 1.5, 0.0]], np.float32)
    got, cnt = _collide(dev, np.concatenate([far, b[:511]]), 1, np.arange(511, dtype=np.int32))
    assert got.tolist() == [1] + [0] * 510 and cnt == 1


# ---- end to end ----------------------------------------------------------------------------------------------------
CLASSES = ["car", "truck", "ped"]
HW = (240, 320)
# camera 0 looks along +x, camera 1 along -x: depth = +-x, u = 160 + 100 * y / depth, v = 120 + 100 * z / depth
CAMS = np.array([[[160.0, 100, 0, 0], [120.0, 0, 100, 0], [1.0, 0, 0, 0], [0, 0, 0, 1.0]],
                 [[-160.0, 100, 0, 0], [-120.0, 0, 100, 0], [-1.0, 0, 0, 0], [0, 0, 0, 1.0]]])
PARAMS = dict(angle=0.2, scale=1.03, trans=[0.3, -0.2, 0.1], flip_h=True, flip_v=False)
GROUPS = dict(car=4, truck=3, ped=3)
PREPARE = dict(filter_by_difficulty=[-1], filter_by_min_points=dict(car=5, truck=5, ped=5))


def _scenario():
    """three frames of 6 boxes and 3 000 points, and a scene to paste into; all on the host"""
    rng = np.random.default_rng(77)
    frames = []
    for f in range(3):
        boxes = _boxes(rng, 6, D=9)
        names = [CLASSES[(i + f) % 3] for i in range(6)]
        frames.append(dict(boxes=boxes, names=names, points=A.inside_inputs(rng, 3000, boxes, F=5),
                           images=rng.integers(0, 256, (2,) + HW + (3,), dtype=np.uint8)))
    gt = _boxes(rng, 4, D=9)
    gt_labels = np.array([0, 0, 1, 2], np.int64)
    every = np.concatenate([gt] + [f["boxes"] for f in frames])
    scene = A.inside_inputs(rng, 2500, every, F=5)             # clear of the faces of whatever gets pasted
    return frames, gt, gt_labels, scene, rng.integers(0, 256, (2,) + HW + (3,), dtype=np.uint8)


def _reference_chain(frames, gt, gt_labels):
    """the database and one sample_all in numpy: _gtdb_ref.extract per frame, the sampler's draws over the host
    records, _gtdb_ref.collide, _gtdb_ref.gather"""
    infos, rows, used = {}, [], 0
    for f in frames:
        r, off = G.extract(f["points"], f["boxes"])
        rows.append(r)
        for i, name in enumerate(f["names"]):
            infos.setdefault(name, []).append(dict(name=name, box3d_lidar=f["boxes"][i].copy(), difficulty=0,
                                                   num_points_in_gt=int(off[i + 1] - off[i]),
                                                   segment=(used + int(off[i]), int(off[i + 1] - off[i])), patch=None))
        used += int(off[-1])
    rows = np.concatenate(rows, 0)
    stub = types.SimpleNamespace(db_infos=infos, rows=None, device=None)
    s = NG.UnifiedDataBaseSampler(stub, 1.0, PREPARE, GROUPS, CLASSES, np.random.RandomState(5))
    cand, group = [], []
    for g, (name, num) in enumerate(zip(s.sample_classes, s.sample_counts(gt_labels))):
        if num > 0:
            drawn = s.sampler_dict[name].sample(num)
            cand += drawn
            group += [g] * len(drawn)
    sp = np.stack([c["box3d_lidar"] for c in cand])
    boxes = np.concatenate([gt, sp], 0)
    keep, count, margin = G.collide(boxes, len(gt), group)
    assert margin > G.tol(boxes), (margin, G.tol(boxes))
    kept = [c for c, k in zip(cand, keep) if k]
    points = G.gather(rows, [c["segment"][0] for c in kept], [c["segment"][1] for c in kept],
                      [c["box3d_lidar"][:3] for c in kept])
    return dict(rows=rows, n_cand=len(cand), kept=kept, points=points, boxes=sp[keep.astype(bool)],
                labels=np.array([CLASSES.index(c["name"]) for c in kept], np.int64))


def test_database_end_to_end(dev):
    frames, gt, gt_labels, scene, scene_img = _scenario()
    ref = _reference_chain(frames, gt, gt_labels)
    K = len(ref["kept"])
    assert 0 < K < ref["n_cand"], "the scene must keep some candidates and reject some"

    capacity = ref["rows"].shape[0] + 100
    db = NG.GtDatabase(CLASSES, 5, dev, capacity_rows=capacity)
    dev_frames = []
    for i, f in enumerate(frames):
        dev_frames.append(torch.from_numpy(f["images"]).to(dev))
        added = db.add_frame(torch.from_numpy(f["points"]).to(dev), f["boxes"], f["names"], frames=dev_frames[-1],
                             lidar2img=CAMS, sample_idx=100 + i)
        assert [a["gt_idx"] for a in added] == list(range(6)) and all(a["image_idx"] == 100 + i for a in added)
    assert len(db) == 18 and db.used_rows == ref["rows"].shape[0]
    assert np.array_equal(_bits(db.rows[:db.used_rows].cpu().numpy()), _bits(ref["rows"]))
    assert sorted(i["group_id"] for v in db.db_infos.values() for i in v) == list(range(18))
    n_patch = 0
    for name, lst in db.db_infos.items():
        for info in lst:
            f = frames[info["image_idx"] - 100]
            assert np.array_equal(info["box3d_lidar"], f["boxes"][info["gt_idx"]]) and info["name"] == f["names"][info["gt_idx"]]
            plan = NG.crop_plan(G.box_corners(f["boxes"][info["gt_idx"]:info["gt_idx"] + 1])[0], CAMS, HW)
            if plan is None:
                assert info["patch"] is None and info["image_crop_key"] == "" and info["image_crop_depth"] == 0
            else:
                x0, y0, x1, y1 = plan["bbox"]
                assert info["image_crop_key"] == plan["cam"] and info["image_crop_depth"] == plan["depth"]
                assert np.array_equal(info["patch"].cpu().numpy(), f["images"][plan["cam"], y0:y1, x0:x1])
                n_patch += 1
    assert n_patch >= 6, "the cameras must see some of the boxes"
    with pytest.raises(RuntimeError, match=f"holds {capacity} rows"):      # a fourth frame does not fit
        db.add_frame(torch.from_numpy(frames[0]["points"]).to(dev), frames[0]["boxes"], frames[0]["names"])
    assert len(db) == 18 and db.used_rows == ref["rows"].shape[0]

    s = NG.UnifiedDataBaseSampler(db, 1.0, PREPARE, GROUPS, CLASSES, np.random.RandomState(5))
    ret = s.sample_all(gt, gt_labels, with_img=True)
    assert ret is not None and set(ret) == {"gt_bboxes_3d", "gt_labels_3d", "points", "points_idx", "images", "group_ids"}
    assert np.array_equal(_bits(ret["gt_bboxes_3d"].cpu().numpy()), _bits(ref["boxes"]))
    assert ret["gt_labels_3d"].cpu().tolist() == ref["labels"].tolist()
    assert np.array_equal(_bits(ret["points"].cpu().numpy()), _bits(ref["points"]))
    lens = [c["segment"][1] for c in ref["kept"]]
    assert ret["points_idx"].tolist() == np.repeat(np.arange(K), lens).tolist()
    assert ret["group_ids"].tolist() == list(range(4, 4 + K)) and len(ret["images"]) == K

    # the sampled objects through the point and box augmentation
    dscene = torch.from_numpy(scene).to(dev)
    got, cnt = NA.augment_points(dscene, PARAMS, paste_points=ret["points"], paste_boxes=ret["gt_bboxes_3d"],
                                 point_cloud_range=RANGE)
    want = A.augment_points(scene, PARAMS, paste=ref["points"], paste_boxes=ref["boxes"], rng=RANGE)
    n = int(cnt)
    assert n == want.shape[0] and 0 < n < scene.shape[0] + ref["points"].shape[0]
    assert np.array_equal(_bits(got[:n].cpu().numpy()), _bits(want))
    ob, ol, oc = NA.augment_boxes(torch.from_numpy(gt).to(dev), torch.from_numpy(gt_labels).to(dev), PARAMS,
                                  paste_boxes=ret["gt_bboxes_3d"], paste_labels=ret["gt_labels_3d"],
                                  point_cloud_range=RANGE, num_classes=3, gravity=True)
    wb, wl = A.augment_boxes(np.concatenate([gt, ref["boxes"]]), np.concatenate([gt_labels, ref["labels"]]), PARAMS,
                             rng=RANGE, num_classes=3, gravity=True)
    m = int(oc)
    assert m == wb.shape[0] and np.array_equal(_bits(ob[:m].cpu().numpy()), _bits(wb)) and ol[:m].cpu().tolist() == wl.tolist()

    # ... and the patches through the image paste
    for c, img in zip(ref["kept"], ret["images"]):
        mine = next(i for i in db.db_infos[c["name"]] if i["segment"] == c["segment"])
        if mine["patch"] is None:
            assert img.numel() == 0
        else:
            assert torch.equal(img, mine["patch"])
    corners = G.box_corners(np.concatenate([gt, ref["boxes"]]))
    plan = NI.paste_plan(corners, CAMS, HW, K)
    dimg = torch.from_numpy(scene_img).to(dev)
    out = NI.paste_images(dimg, plan, ret["images"])
    torch.cuda.synchronize()
    assert out.data_ptr() == dimg.data_ptr()
    if any(len(p) and (p[:, 4] >= 0).any() and any(ret["images"][j].numel() for j in p[p[:, 4] >= 0, 4]) for p in plan):
        assert not np.array_equal(out.cpu().numpy(), scene_img)

    # nothing to sample: the class is already present often enough
    full = NG.UnifiedDataBaseSampler(db, 1.0, PREPARE, dict(car=2), CLASSES, np.random.RandomState(5))
    assert full.sample_all(gt, gt_labels) is None               # two cars are present: int(2 - 2) = 0 to draw
