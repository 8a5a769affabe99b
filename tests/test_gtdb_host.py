"""Host side of the ground-truth database (native_gtdb.py): the ABI of the three new calls and their argument errors
(every one before any device work, with null device pointers), the numpy restatement of tests/_gtdb_ref.py against
answers worked out by hand, the draw order of BatchSampler, ``crop_plan``, the sampler's counts and the ``db_sampler``
of the reference configs.  No test here needs a device.
"""
import ctypes
import os
import types

import numpy as np
import pytest
import torch

import _gtdb_ref as G

REF_CONFIGS = "/root/reference/projects/configs"
EINVAL = 1001


def _lib():
    from projects.mmdet3d_plugin import native
    if not native.available():
        pytest.skip("libcmt_hip.so not built")
    return native, native.lib()


# ---- ABI ---------------------------------------------------------------------------------------------------------
def test_gtdb_abi():
    native, L = _lib()
    from projects.mmdet3d_plugin import native_aug as NA
    from projects.mmdet3d_plugin import native_gtdb as NG
    assert L.cmt_abi_version() == 25
    for key, cls in (("gtdb_extract", native.GtdbExtractArgs), ("gtdb_gather", native.GtdbGatherArgs),
                     ("gtdb_collide", native.GtdbCollideArgs)):
        assert native.STRUCTS[key] is cls
        assert getattr(L, f"cmt_{key}_args_size")() == ctypes.sizeof(cls), key
        assert hasattr(L, f"cmt_{key}")
    T = NA.tile_rows()
    assert NG.workspace_bytes(0, 5) == 0 == NG.workspace_bytes(5, 0)
    assert NG.workspace_bytes(1, 1) == 8 == NG.workspace_bytes(T, 1)
    assert NG.workspace_bytes(T + 1, 3) == 2 * 2 * 3 * 4 and NG.workspace_bytes(300000, 64) == 8 * 64 * -(-300000 // T)
    assert NG.MAX_FRAME_BOXES == 1024 and NG.MAX_COLLIDE_BOXES == 512 and NG.MAX_PASTE_BOXES == 128


def test_null_structs_are_rejected():
    _, L = _lib()
    for name in ("cmt_gtdb_extract", "cmt_gtdb_gather", "cmt_gtdb_collide"):
        assert getattr(L, name)(None, None) == EINVAL
        assert name in L.cmt_last_error().decode()


def _extract_args(native, **kw):
    a = native.GtdbExtractArgs()
    a.N, a.cap, a.M, a.F, a.D = 0, 0, 0, 5, 7
    for k, v in kw.items():
        setattr(a, k, v)
    return a


@pytest.mark.parametrize("kw,text", [
    (dict(M=1025), "M must"), (dict(M=2048), "M must"), (dict(M=-1), "M must"),
    (dict(N=-1), "N must"), (dict(N=2 ** 31), "N must"), (dict(N=2 ** 22, M=512), "N * M"),
    (dict(F=2), "F must"), (dict(F=9), "F must"), (dict(D=8), "D must"), (dict(D=6), "D must"),
    (dict(cap=-1), "cap must"), (dict(cap=2 ** 31), "cap must"),
    (dict(N=2049, M=3, workspace_bytes=71), "workspace below"),            # 2 * 3 tiles * 3 boxes * 4 = 72
    (dict(N=2049, M=3, workspace_bytes=72), "points must"),                # enough: the null points are next
    (dict(N=1, points=0x1002), "points must"),
    (dict(M=1, boxes=0x1002), "boxes must"),
    (dict(), "offsets must"), (dict(offsets=0x1002), "offsets must"),
    (dict(offsets=0x1000, count_in=0x1001), "count_in and rows"),
    (dict(offsets=0x1000, rows=0x1002), "count_in and rows"),
    (dict(offsets=0x1000, cap=4), "rows must be non-null"),
])
def test_extract_einval(kw, text):
    """the pointers are null or made-up numbers: every case must return before any device work"""
    native, L = _lib()
    assert L.cmt_gtdb_extract(ctypes.byref(_extract_args(native, **kw)), None) == EINVAL
    msg = L.cmt_last_error().decode()
    assert "cmt_gtdb_extract" in msg and text in msg, msg


@pytest.mark.parametrize("kw,text", [
    (dict(K=129), "K must"), (dict(K=-1), "K must"), (dict(F=2), "F must"), (dict(F=9), "F must"),
    (dict(n_rows=-1), "n_rows and n_dst"), (dict(n_dst=2 ** 31), "n_rows and n_dst"),
    (dict(K=1, rows=0x1002), "4-byte aligned"), (dict(K=1, seg_len=0x1001), "4-byte aligned"),
    (dict(K=1, centre=0x1003), "4-byte aligned"), (dict(K=1, dst=0x1002), "4-byte aligned"),
    (dict(K=1), "must be non-null with K > 0"),
])
def test_gather_einval(kw, text):
    native, L = _lib()
    a = native.GtdbGatherArgs()
    a.n_rows, a.n_dst, a.K, a.F = 10, 10, 0, 5
    for k, v in kw.items():
        setattr(a, k, v)
    assert L.cmt_gtdb_gather(ctypes.byref(a), None) == EINVAL
    msg = L.cmt_last_error().decode()
    assert "cmt_gtdb_gather" in msg and text in msg, msg


@pytest.mark.parametrize("n_gt,n_s,D,group,text", [
    (0, 513, 7, None, "at most 512"), (512, 1, 7, None, "at most 512"), (2 ** 31 - 1, 2 ** 31 - 1, 7, None, "at most 512"),
    (-1, 2, 7, None, "at most 512"), (1, -1, 7, None, "at most 512"),
    (1, 1, 8, [0], "D must"), (1, 3, 7, None, "group must be non-null"),
    (1, 3, 7, [0, 1, 0], "must not decrease"), (0, 2, 9, [5, 4], "must not decrease"),
    (1, 3, 7, [0, 0, 1], "count must"),                                     # a good group: the null count is next
])
def test_collide_einval(n_gt, n_s, D, group, text):
    native, L = _lib()
    a = native.GtdbCollideArgs()
    a.n_gt, a.n_s, a.D = n_gt, n_s, D
    g = None if group is None else np.asarray(group, np.int32)
    a.group = None if g is None else ctypes.c_void_p(g.ctypes.data)
    assert L.cmt_gtdb_collide(ctypes.byref(a), None) == EINVAL
    msg = L.cmt_last_error().decode()
    assert "cmt_gtdb_collide" in msg and text in msg, msg


def test_wrapper_argument_errors():
    from projects.mmdet3d_plugin import native_gtdb as NG
    p, b = torch.zeros((4, 5)), torch.zeros((2, 7))
    i32 = torch.zeros(2, dtype=torch.int32)
    c = torch.zeros((2, 3))
    bad = [
        (NG.extract_objects, (p.double(), b), {}),
        (NG.extract_objects, (p[:, :2], b), {}),
        (NG.extract_objects, (p, b[:, :6]), {}),
        (NG.extract_objects, (p, torch.zeros((1025, 7))), {}),
        (NG.extract_objects, (p, b), dict(count=torch.zeros(1))),
        (NG.extract_objects, (p, b), dict(out=torch.zeros((4, 4)))),
        (NG.extract_objects, (p, b), dict(out=torch.zeros((4, 5), dtype=torch.float64))),
        (NG.extract_objects, (p, b), {}),                                   # CPU tensors: no CPU path
        (NG.gather_objects, (p, i32, i32, i32, c, 4), dict(out=torch.zeros((3, 5)))),
        (NG.gather_objects, (p, i32.long(), i32, i32, c, 4), {}),
        (NG.gather_objects, (p, i32, i32[:1], i32, c, 4), {}),
        (NG.gather_objects, (p, i32, i32, i32, c[:, :2], 4), {}),
        (NG.gather_objects, (p, i32, i32, i32, c, -1), {}),
        (NG.gather_objects, (p, torch.zeros(129, dtype=torch.int32), i32, i32, c, 4), {}),
        (NG.gather_objects, (p, i32, i32, i32, c, 4), {}),                  # CPU tensors: no CPU path
        (NG.collide, (torch.zeros((513, 7)), 0, [0] * 513), {}),
        (NG.collide, (b, 3, []), {}),
        (NG.collide, (b, 0, [0]), {}),
        (NG.collide, (b, 0, [1, 0]), {}),
        (NG.collide, (b[:, :6], 0, [0, 0]), {}),
        (NG.collide, (b, 1, [0]), {}),                                      # CPU tensors: no CPU path
        (NG.GtDatabase, (["car"], 2, "cuda:0", 10), {}),
        (NG.GtDatabase, (["car"], 5, "cuda:0", 0), {}),
        (NG.GtDatabase, (["car"], 5, "cpu", 10), {}),
        (NG.crop_plan, (np.zeros((4, 3)), np.zeros((1, 4, 4)), (10, 10)), {}),
        (NG.crop_plan, (np.zeros((8, 3)), np.zeros((4, 4)), (10, 10)), {}),
        (NG.crop_plan, (np.zeros((8, 3)), np.zeros((1, 4, 4)), (0, 10)), {}),
        (NG.crop_plan, (np.zeros((8, 3)), np.tile(np.eye(4), (1, 1, 1)), (10, 10)), {}),   # depth 0: non-finite
    ]
    for fn, args, kw in bad:
        with pytest.raises(ValueError):
            fn(*args, **kw)


# ---- the collision test against answers worked out by hand -------------------------------------------------------
def _rect(x0, y0, x1, y1):
    """clockwise corners in center_to_corner_box2d's order for an axis-aligned rectangle"""
    return np.array([[x0, y0], [x0, y1], [x1, y1], [x1, y0]], np.float64)


def test_corners_order_and_rotation():
    c = G.corners(np.array([[1.0, 2.0, 0, 4.0, 2.0, 1, 0.0], [0, 0, 0, 2.0, 1.0, 1, np.pi / 2]], np.float32))
    assert np.array_equal(c[0], _rect(-1, 1, 3, 3))                       # (-,-), (-,+), (+,+), (+,-)
    # a quarter turn counter-clockwise: (-1, -0.5) -> (0.5, -1)
    assert np.allclose(c[1], [[0.5, -1], [-0.5, -1], [-0.5, 1], [0.5, 1]], atol=1e-6)


def test_collide_pair_known_answers():
    plus_h, plus_v = _rect(-2, -0.5, 2, 0.5), _rect(-0.5, -2, 0.5, 2)
    assert G.collide_pair(plus_h, plus_v) and G.collide_pair(plus_v, plus_h)          # a cross: edges intersect
    big, small = _rect(-5, -4, 5, 4), _rect(0, 0, 1, 0.5)
    assert G.collide_pair(big, small) and G.collide_pair(small, big)                  # containment, no edge touches
    assert not G.collide_pair(_rect(0, 0, 2, 2), _rect(5, 0, 7, 2))                   # a gap: iw = 2 - 5 < 0
    assert not G.collide_pair(_rect(0, 0, 2, 2), _rect(2, 0, 4, 2))                   # sharing an edge: iw = 0
    # identical rectangles: every edge pair is collinear or meets at an end point, every product pair ties and the
    # strict '>' is false both times; every corner lies ON an edge, cross = 0, not < 0.  The reference's test says
    # "no collision" for an exact copy, and so does this restatement.
    assert not G.collide_pair(_rect(0, 0, 4, 2), _rect(0, 0, 4, 2))
    # ... while a copy moved a little along both axes crosses it
    assert G.collide_pair(_rect(0, 0, 4, 2), _rect(0.25, 0.125, 4.25, 2.125))


def test_hand_scenes():
    for name, (boxes, n_gt, group, want) in G.hand_scenes().items():
        keep, count, margin = G.collide(boxes, n_gt, group)
        assert keep.tolist() == want.tolist() and count == int(want.sum()), name
        assert margin > G.tol(boxes), (name, margin, G.tol(boxes))
    # the two thin boxes at 45 degrees: their stand-up rectangles overlap, so the edge and containment tests ran
    b = G.hand_scenes()["standup_only"][0]
    c = G.corners(b)
    assert min(c[0, :, 0].max(), c[1, :, 0].max()) - max(c[0, :, 0].min(), c[1, :, 0].min()) > 0.5
    keep, _, margin = G.collide(G.IDENTICAL, 1, [0])
    assert keep.tolist() == [1] and margin == 0.0          # exact ties: outside the tolerance contract, exact in fp32


def test_greedy_known_answers():
    # boxes 0..1 to avoid, candidates 2..5; groups [0, 0, 1, 1]
    mat = np.zeros((6, 6), bool)

    def hit(i, j):
        mat[i, j] = mat[j, i] = True
    hit(2, 3)                 # candidate 0 touches only the later candidate 1 of its group: 0 goes, 1 stays
    hit(4, 2)                 # candidate 2 (group 1) touches only the rejected candidate 0: stays
    hit(5, 3)                 # candidate 3 touches the kept candidate 1 of an earlier group: goes
    assert G.greedy(mat, 2, [0, 0, 1, 1]).tolist() == [0, 1, 1, 0]
    # in ONE group later candidates are live too: 0 goes (touches 1), 1 goes (touches the later 3), 2 stays (0 is
    # gone), 3 stays (1 is gone)
    assert G.greedy(mat, 2, [0, 0, 0, 0]).tolist() == [0, 0, 1, 1]
    # each alone in its group: 0 stays (1 is not there yet), 1 goes (touches kept 0), 2 goes, 3 stays
    assert G.greedy(mat, 2, [0, 1, 2, 3]).tolist() == [1, 0, 0, 1]
    m2 = np.zeros((3, 3), bool)
    m2[1, 0] = m2[0, 1] = True
    assert G.greedy(m2, 1, [0, 0]).tolist() == [0, 1]      # a box to avoid rejects


def test_random_scenes_skip_count():
    """the GPU test's generator: at most 24 of its 60 scenes may fall inside the tolerance"""
    rs = np.random.RandomState(0)
    skipped = 0
    for _ in range(60):
        b, n_gt, group = G.random_scene(rs)
        skipped += G.collide(b, n_gt, group)[2] <= G.tol(b)
    print(f"{skipped} of 60 random scenes have a comparison within tol")
    assert skipped <= 24


def test_extract_and_gather_restatement():
    pts = np.array([[1, 1, 0.5, 7], [5, 5, 0.5, 8], [1.5, 1, 0.25, 9], [1, 1, 5, 10]], np.float32)
    boxes = np.array([[1, 1, 0, 2, 2, 1, 0.0], [9, 9, 0, 1, 1, 1, 0.0], [1.25, 1, 0, 1, 1, 1, 0.0]], np.float32)
    rows, off = G.extract(pts, boxes)
    assert off.tolist() == [0, 2, 2, 4]
    assert rows.tolist() == [[0, 0, 0.5, 7], [0.5, 0, 0.25, 9], [-0.25, 0, 0.5, 7], [0.25, 0, 0.25, 9]]
    assert G.extract(pts, boxes, count=1)[1].tolist() == [0, 1, 1, 2]
    back = G.gather(rows, [2, 0], [2, 1], [[1.25, 1, 0], [1, 1, 0]])
    assert back.tolist() == [[1, 1, 0.5, 7], [1.5, 1, 0.25, 9], [1, 1, 0.5, 7]]


# ---- BatchSampler --------------------------------------------------------------------------------------------------
def test_batch_sampler_draw_order():
    from projects.mmdet3d_plugin.native_gtdb import BatchSampler
    items = ["a", "b", "c", "d", "e"]
    bs = BatchSampler(items, np.random.RandomState(0))
    probe = np.random.RandomState(0)
    idx = np.arange(5)
    probe.shuffle(idx)                                      # construction
    first = idx.copy()
    assert first.tolist() == [2, 0, 1, 3, 4]                # RandomState(0).shuffle(arange(5))
    assert bs.sample(2) == [items[i] for i in first[:2]]
    assert bs.sample(2) == [items[i] for i in first[2:4]]
    assert bs.sample(2) == [items[first[4]]]                # 4 + 2 >= 5: the tail alone, then a reshuffle
    probe.shuffle(idx)                                      # ... of the shuffled array, in place
    second = idx.copy()
    assert bs.sample(1) == [items[second[0]]]
    assert bs.sample(4) == [items[i] for i in second[1:]]   # 1 + 4 >= 5: reaches the end exactly, resets
    probe.shuffle(idx)
    assert bs.sample(3) == [items[i] for i in idx[:3]]
    assert BatchSampler([], np.random.RandomState(0)).sample(3) == []


# ---- crop_plan -------------------------------------------------------------------------------------------------------
# a camera looking along +x: depth = x, u = 200 + 100 * y / x, v = 100 + 100 * z / x
CAM = np.array([[200.0, 100, 0, 0], [100.0, 0, 100, 0], [1.0, 0, 0, 0], [0, 0, 0, 1.0]])
HW = (300, 400)


def _corners8(ys, zs, x=10.0):
    """eight points at depth x: (y0 z0), (y0 z1), (y1 z0), (y1 z1), twice; corner 2 is (ys[1], zs[0])"""
    c = np.array([[x, y, z] for y in ys for z in zs] * 2, np.float64)
    return c


def test_crop_plan_known_answers():
    from projects.mmdet3d_plugin.native_gtdb import crop_plan
    L = CAM[None]
    got = crop_plan(_corners8([-2, 3], [-1, 2]), L, HW)                    # u in {180, 230}, v in {90, 120}
    assert got == dict(cam=0, bbox=(180, 90, 230, 120), depth=10.0)
    got = crop_plan(_corners8([-2.07, 30], [-0.91, 2]), L, HW)             # 179.3 truncates, 500 clips to W - 1
    assert got["bbox"] == (179, 90, 399, 120)
    got = crop_plan(_corners8([-2, 3], [-1, 25]), L, HW)                   # v 350 clips to H - 1
    assert got["bbox"] == (180, 90, 230, 299)
    assert crop_plan(_corners8([0, 1.0], [-1, 2]), L, HW) is None          # 10 pixels wide: '<= 10' drops it
    assert crop_plan(_corners8([0, 1.1], [-1, 2]), L, HW)["bbox"] == (200, 90, 211, 120)
    assert crop_plan(_corners8([-2, 3], [1, 2]), L, HW) is None            # 10 pixels high


def test_crop_plan_row_two_quirk():
    """``coord_img[2] <= 0`` reads corner 2's row (u, v, depth, w), not the depth column"""
    from projects.mmdet3d_plugin.native_gtdb import crop_plan
    L = CAM[None]
    base = _corners8([-2, 3], [-1, 2])
    off_left = base.copy()
    off_left[2] = [10, -25, 2]                                             # corner 2 projects to u = -50
    assert crop_plan(off_left, L, HW) is None
    other = base.copy()
    other[5] = [10, -25, 2]                                                # the same point as corner 5: kept, clipped
    assert crop_plan(other, L, HW)["bbox"] == (0, 90, 230, 120)
    behind = base.copy()
    behind[5] = [-10, 1, 1]                                                # corner 5 BEHIND the camera still passes
    got = crop_plan(behind, L, HW)                                         # it projects to (190, 90)
    assert got["bbox"] == (180, 90, 230, 120) and got["depth"] == 7.5
    behind2 = base.copy()
    behind2[2] = [-10, 1, 1]                                               # corner 2 behind the camera: skipped
    assert crop_plan(behind2, L, HW) is None
    with pytest.raises(ValueError, match="non-finite"):
        zero = base.copy()
        zero[4] = [0, 1, 1]
        crop_plan(zero, L, HW)


def test_crop_plan_tie_rule():
    from projects.mmdet3d_plugin.native_gtdb import crop_plan
    c = _corners8([-1, 1], [-1, 1])                                        # 20 x 20 pixels through CAM
    wide = CAM.copy()
    wide[0, 1] = 200                                                       # 40 x 20 pixels
    assert crop_plan(c, np.stack([CAM, CAM]), HW)["cam"] == 0              # a tie: the first camera
    assert crop_plan(c, np.stack([CAM, wide]), HW)["cam"] == 1             # strictly larger wins
    assert crop_plan(c, np.stack([wide, CAM]), HW)["cam"] == 0
    assert crop_plan(c, np.stack([wide, CAM, CAM]), HW) == dict(cam=0, bbox=(180, 90, 220, 110), depth=10.0)
    # the reference never updates crop_area: its last qualifying camera wins
    assert crop_plan(c, np.stack([wide, CAM, CAM]), HW, keep_largest=False)["cam"] == 2
    assert crop_plan(c, np.stack([CAM, CAM]), HW, keep_largest=False)["cam"] == 1


def test_box_corners_order():
    from projects.mmdet3d_plugin.native_gtdb import box_corners
    got = box_corners(np.array([[1.0, 2.0, -1.0, 4.0, 2.0, 3.0, 0.0, 9, 9]]))[0]
    assert got.tolist() == [[-1, 1, -1], [-1, 1, 2], [-1, 3, 2], [-1, 3, -1], [3, 1, -1], [3, 1, 2], [3, 3, 2], [3, 3, -1]]
    assert np.array_equal(got, G.box_corners(np.array([[1.0, 2.0, -1.0, 4.0, 2.0, 3.0, 0.0]]))[0])
    turned = box_corners(np.array([[0, 0, 0, 2.0, 1.0, 1.0, np.pi / 2]]))[0]
    assert np.allclose(turned[0], [0.5, -1, 0], atol=1e-12)               # (-1, -0.5) a quarter turn counter-clockwise


# ---- the sampler on the host ---------------------------------------------------------------------------------------
def _info(name, n, difficulty=0):
    return dict(name=name, num_points_in_gt=n, difficulty=difficulty, box3d_lidar=np.zeros(7, np.float32),
                segment=(0, n), patch=None)


def _stub_db(**per_class):
    return types.SimpleNamespace(db_infos={k: list(v) for k, v in per_class.items()}, rows=None, device=None)


def test_sampler_counts_and_filters():
    from projects.mmdet3d_plugin.native_gtdb import UnifiedDataBaseSampler
    db = _stub_db(car=[_info("car", n) for n in (3, 5, 9, 4)] + [_info("car", 50, difficulty=-1)],
                  truck=[_info("truck", 7), _info("truck", 2)], bus=[_info("bus", 1)])
    classes = ["car", "truck", "bus"]

    def make(rate, groups=dict(car=4, truck=3), prepare=None):
        prepare = dict(filter_by_difficulty=[-1], filter_by_min_points=dict(car=5, truck=0, tram=5)) if prepare is None else prepare
        return UnifiedDataBaseSampler(db, rate, prepare, groups, classes, np.random.RandomState(0))
    s = make(1.0)
    assert [len(s.db_infos[k]) for k in ("car", "truck", "bus")] == [2, 2, 1]      # 5 and 9 points; min 0 keeps all
    assert len(db.db_infos["car"]) == 5                                              # the database is not edited
    assert s.sample_classes == ["car", "truck"] and s.sample_max_nums == [4, 3]
    assert s.sample_counts([0, 0, 1, 2]) == [2, 2]                                   # 4 - 2 cars, 3 - 1 trucks
    assert s.sample_counts(np.array([], np.int64)) == [4, 3]
    assert s.sample_counts([0] * 6) == [-2, 3]                                       # more present than wanted
    assert make(0.5).sample_counts([0, 0, 1, 2]) == [1, 1]
    assert make(0.25).sample_counts([0, 0, 1, 2]) == [0, 0]                          # np.round(0.5) = 0: half to even
    assert make(0.5, dict(car=5, truck=3)).sample_counts([]) == [2, 2]               # 2.5 -> 2, 1.5 -> 2
    # one BatchSampler per class of the database, shuffled in its order at construction
    probe = np.random.RandomState(0)
    for k in ("car", "truck", "bus"):
        idx = np.arange(len(s.db_infos[k]))
        probe.shuffle(idx)
        assert s.sampler_dict[k]._indices.tolist() == idx.tolist()
    with pytest.raises(ValueError):
        make(1.0, dict(tram=2))
    with pytest.raises(ValueError):
        make(1.0, prepare=dict(filter_by_size=1))
    with pytest.raises(ValueError):
        UnifiedDataBaseSampler(object(), 1.0, {}, dict(car=1), classes, np.random.RandomState(0))


def _ref_db_configs():
    return ["CMT_Nuscenes/lidar/cmt_lidar_voxel0075_cbgs.py",
            "CMT_Nuscenes/fusion/cmt_voxel0075_vov_1600x640_cbgs.py",
            "CMT_Nuscenes/fusion/cmt_voxel0100_r50_800x320_cbgs.py",
            "CMTCoop_TUMTraf/fusion/coop/cmt_voxel0075_vov_1600x640_cbgs_a9coop_pretrained.py",
            "CMTCoop_TUMTraf/lidar/coop/cmt_lidar_voxel0075_cbgs_a9coop_pretrained.py",
            "CMTCoop_TUMTraf/lidar/vehicle/cmt_lidar_voxel0075_cbgs_a9coop_vehicle_pretrained.py",
            "CMTCoop_TUMTraf/fusion/infra/cmt_voxel0075_vov_1600x640_cbgs_a9coop_infrastructure_pretrained.py"]


@pytest.mark.parametrize("name", _ref_db_configs())
def test_db_sampler_from_reference_config(name):
    if not os.path.isdir(REF_CONFIGS):
        pytest.skip("reference checkout not present")
    from projects.mmdet3d_plugin.config import load_config
    from projects.mmdet3d_plugin.native_gtdb import db_sampler_from_config
    cfg = load_config(os.path.join(REF_CONFIGS, name))
    classes = list(cfg["class_names"])
    db = _stub_db(**{c: [_info(c, 10 * (i + 1)) for i in range(4)] for c in classes})
    s = db_sampler_from_config(cfg, db, np.random.RandomState(0))
    assert s.classes == classes and float(s.rate) > 0
    assert set(s.sample_classes) <= set(classes) and len(s.sample_classes) > 0
    assert all(isinstance(v, int) for v in s.sample_max_nums)
    assert set(s.prepare) <= {"filter_by_difficulty", "filter_by_min_points"}
    assert sorted(s.sampler_dict) == sorted(classes)
    counts = s.sample_counts(np.zeros(0, np.int64))
    assert counts == s.sample_max_nums


def test_db_sampler_from_config_without_sampler():
    from projects.mmdet3d_plugin.native_gtdb import db_sampler_from_config
    cfg = dict(data=dict(train=dict(type="CBGSDataset", dataset=dict(pipeline=[dict(type="LoadPointsFromFile")]))))
    with pytest.raises(ValueError, match="no object sampler"):
        db_sampler_from_config(cfg, _stub_db())
    step = dict(type="UnifiedObjectSample", db_sampler=dict(type="UnifiedDataBaseSampler", info_path="x.pkl", data_root=None,
                                                             rate=0.5, prepare=dict(filter_by_min_points=dict(car=2)),
                                                             classes=["car", "bus"], sample_groups=dict(car=3),
                                                             points_loader=dict(type="LoadPointsFromFile")))
    cfg["data"]["train"]["dataset"]["pipeline"].append(step)
    s = db_sampler_from_config(cfg, _stub_db(car=[_info("car", 1), _info("car", 2)]), np.random.RandomState(1))
    assert s.rate == 0.5 and len(s.db_infos["car"]) == 1 and s.sample_counts([1]) == [2]   # round(1.5) = 2
