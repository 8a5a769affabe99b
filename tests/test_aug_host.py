"""Host side of the training point / box pipeline (native_aug.py): the numpy restatement of tests/_aug_ref.py against
hand-computed answers, the order of the random draws, the lidar2img update, the training plan of a config, the
wrappers' argument errors and the ABI of the three new calls.  No test here needs a device.
"""
import ctypes
import os

import numpy as np
import pytest
import torch

import _aug_ref as R

REF_CONFIGS = "/root/reference/projects/configs"
RANGE = [-40.0, -40.0, -4.0, 40.0, 40.0, 2.0]


# ---- the restatement against hand-computed answers --------------------------------------------------------------
def test_quarter_turn():
    """(1, 0, 0) turned by pi / 2 counter-clockwise is (cos, sin, 0) of the rounded matrix: (fl32(6.1e-17), 1, 0)"""
    got = R.xform_xyz(np.array([[1.0, 0.0, 0.0]], np.float32), dict(angle=np.pi / 2))
    assert got.dtype == np.float32
    assert got[0, 1] == 1.0 and got[0, 2] == 0.0 and abs(got[0, 0]) < 1e-7
    assert got[0, 0] == np.float32(np.cos(np.pi / 2))
    # and R is [[c, -s, 0], [s, c, 0], [0, 0, 1]]
    m = R.rot32(0.3)
    assert m[0, 1] == -m[1, 0] < 0 and m[0, 0] == m[1, 1] and m[2, 2] == 1 and m[1, 0] == np.float32(np.sin(0.3))


def test_flips_of_a_nine_column_box():
    box = np.array([[1.0, 2.0, 3.0, 4.0, 5.0, 6.0, 0.25, 0.5, -0.75]], np.float32)
    lab = np.array([0])
    h, _ = R.augment_boxes(box, lab, dict(flip_h=True))
    assert h[0].tolist() == [1.0, -2.0, 3.0, 4.0, 5.0, 6.0, -0.25, 0.5, 0.75]
    v, _ = R.augment_boxes(box, lab, dict(flip_v=True))
    assert v[0, [0, 1, 2, 7, 8]].tolist() == [-1.0, 2.0, 3.0, -0.5, -0.75]
    assert v[0, 6] == np.float32(np.float32(-0.25) + np.float32(np.pi))
    hv, _ = R.augment_boxes(box, lab, dict(flip_h=True, flip_v=True))   # horizontal first: yaw -> -yaw -> yaw + pi
    assert hv[0, [0, 1, 7, 8]].tolist() == [-1.0, -2.0, -0.5, 0.75]
    assert hv[0, 6] == R.limit_yaw(np.float32(np.float32(0.25) + np.float32(np.pi)))
    seven, _ = R.augment_boxes(box[:, :7], lab, dict(flip_h=True, flip_v=True))
    assert np.array_equal(seven[0], hv[0, :7])


def test_limit_yaw_edges():
    P, pi = np.float32(2 * np.pi), np.float32(np.pi)
    assert R.limit_yaw(np.float32(0.0)) == 0.0
    assert R.limit_yaw(pi) == np.float32(pi - P)            # floor(0.5 + 0.5) = 1: +pi maps to -pi
    assert R.limit_yaw(-pi) == -pi                          # floor(-0.5 + 0.5) = 0: -pi stays
    three = np.float32(3 * np.pi)
    assert R.limit_yaw(three) == np.float32(three - np.float32(2) * P)   # 3 pi -> -pi (floor(1.5 + 0.5) = 2)
    assert abs(float(R.limit_yaw(three)) + np.pi) < 1e-6
    assert R.limit_yaw(np.float32(1.0)) == 1.0 and R.limit_yaw(np.float32(-3.0)) == np.float32(-3.0)


def test_box_on_the_bev_edge_is_dropped():
    rows = []
    for col, face in ((0, RANGE[0]), (0, RANGE[3]), (1, RANGE[1]), (1, RANGE[4])):
        on = np.array([1.0, 2.0, 0.0, 1, 1, 1, 0.0], np.float32)
        on[col] = face
        just_in = on.copy()
        just_in[col] = np.nextafter(np.float32(face), np.float32(0))
        rows += [on, just_in]
    rows.append(np.array([1.0, 2.0, 100.0, 1, 1, 1, 0.0], np.float32))   # z is not tested
    b = np.stack(rows)
    kept, labs = R.augment_boxes(b, np.arange(9), {}, rng=RANGE, num_classes=9)
    assert labs.tolist() == [1, 3, 5, 7, 8]
    kept, labs = R.augment_boxes(b, np.array([0, -1, 3, 2, 1, 0, 0, 0, 0]), {}, rng=None, num_classes=3)
    assert labs.tolist() == [0, 2, 1, 0, 0, 0, 0]


def test_point_on_z_bottom_is_outside():
    box = np.array([[0.0, 0.0, -1.0, 2.0, 4.0, 1.5, 0.0]], np.float32)
    pts = np.array([[0, 0, -1.0], [0, 0, -0.999], [0, 0, 0.5], [0, 0, 0.499], [1.0, 0, 0], [0.999, 0, 0],
                    [0, 2.0, 0], [0, -1.999, 0], [np.nan, 0, 0]], np.float32)
    assert R.inside(pts, box)[:, 0].tolist() == [False, True, False, True, False, True, False, True, False]
    first, cnt = R.points_in_boxes(pts, box)
    assert first.tolist() == [-1, 0, -1, 0, -1, 0, -1, 0, -1] and cnt.tolist() == [4]
    # a quarter-turned box swaps its extents in the world
    turned = np.array([[0.0, 0.0, -1.0, 2.0, 4.0, 1.5, np.pi / 2]], np.float32)
    assert R.inside(np.array([[1.9, 0, 0], [0, 1.9, 0]], np.float32), turned)[:, 0].tolist() == [True, False]
    # nothing is inside a box without extent, a NaN box, or with no boxes at all
    flat = box.copy()
    flat[0, 3] = 0
    nanbox = box.copy()
    nanbox[0, 6] = np.nan
    assert not R.inside(pts, flat).any() and not R.inside(pts, nanbox).any()
    assert R.points_in_boxes(pts, np.zeros((0, 7), np.float32))[0].tolist() == [-1] * 9


def test_inside_inputs_are_clear_of_every_face():
    rng = np.random.default_rng(0)
    boxes = np.array([[5, 5, -1, 4, 2, 1.5, 0.3], [6, 5.5, -1, 4, 2, 2, -2.5]], np.float32)
    pts = R.inside_inputs(rng, 500, boxes)
    m = R.inside(pts, boxes)
    assert 100 < m.any(1).sum() < 450 and (m.sum(1) == 2).any()
    with pytest.raises(AssertionError, match="margin"):
        R.assert_clear_of_faces(np.array([[5.0, 5.0, -1.0 + 1e-5]], np.float32), boxes)


def test_reference_pipeline_order():
    """rows dropped by count, paste box and range; paste rows in front or behind; an out-of-range order entry"""
    src = np.array([[0, 0, 0, 1], [10, 0, 0, 2], [0, 30, 0, 3], [5, 5, 0, 4]], np.float32)
    paste = np.array([[0.1, 0.1, 0.2, 9]], np.float32)
    box = np.array([[0, 0, -1, 2, 2, 2, 0.0]], np.float32)
    got = R.augment_points(src, dict(trans=[1, 0, 0]), count=3, paste=paste, paste_boxes=box, paste_first=True,
                           rng=[-20, -20, -2, 20, 20, 2])
    assert got[:, 3].tolist() == [9, 2]
    assert got[0, 0] == np.float32(0.1) + np.float32(1) and got[1, 0] == 11.0
    got = R.augment_points(src, {}, paste=paste, paste_boxes=box, order=[4, 7, 3, -1, 0, 1])
    assert got[:, 3].tolist() == [9, 4, 2]


# ---- the random draws --------------------------------------------------------------------------------------------
PLAN = dict(rot_range=[-0.785, 0.785], scale_ratio_range=[0.9, 1.1], translation_std=[0.5, 0.5, 0.5],
            flip_ratio_bev_horizontal=0.5, flip_ratio_bev_vertical=0.5)


def test_sample_augmentation_draw_order():
    from projects.mmdet3d_plugin import native_aug as NA
    got = NA.sample_augmentation(PLAN, np.random.RandomState(0))
    rs = np.random.RandomState(0)
    angle = rs.uniform(-0.785, 0.785)
    scale = rs.uniform(0.9, 1.1)
    trans = rs.normal(scale=np.array([0.5, 0.5, 0.5], np.float32), size=3).T
    fh = rs.rand() < 0.5
    fv = rs.rand() < 0.5
    assert got["angle"] == angle and got["scale"] == scale and np.array_equal(got["trans"], trans)
    assert got["flip_h"] == fh and got["flip_v"] == fv
    assert set(got) == {"angle", "scale", "trans", "flip_h", "flip_v"}


def test_sample_augmentation_absent_steps_consume_no_draw():
    from projects.mmdet3d_plugin import native_aug as NA
    no_flip = dict(PLAN, flip_ratio_bev_horizontal=None, flip_ratio_bev_vertical=None)
    rs = np.random.RandomState(0)
    got = NA.sample_augmentation(no_flip, rs)
    assert got["flip_h"] is False and got["flip_v"] is False and got["angle"] is not None
    probe = np.random.RandomState(0)
    probe.uniform(), probe.uniform(), probe.normal(size=3)
    assert rs.rand() == probe.rand()                      # five values were drawn, no more
    no_grst = dict(PLAN, rot_range=None, scale_ratio_range=None, translation_std=None)
    rs = np.random.RandomState(0)
    got = NA.sample_augmentation(no_grst, rs)
    assert got["angle"] is None and got["scale"] is None and got["trans"] is None
    probe = np.random.RandomState(0)
    assert got["flip_h"] == bool(probe.rand() < 0.5) and got["flip_v"] == bool(probe.rand() < 0.5)
    rs = np.random.RandomState(3)
    state = rs.get_state()[1].copy()
    got = NA.sample_augmentation(dict(), rs)
    assert got == dict(angle=None, scale=None, trans=None, flip_h=False, flip_v=False)
    assert np.array_equal(rs.get_state()[1], state)


# ---- lidar2img ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("flips", [(False, False), (True, False), (False, True), (True, True)])
def test_augment_lidar2img_projects_alike(flips):
    from projects.mmdet3d_plugin import native_aug as NA
    rng = np.random.default_rng(4)
    params = dict(angle=0.37, scale=1.07, trans=[0.4, -0.3, 0.2], flip_h=flips[0], flip_v=flips[1])
    L = rng.normal(size=(6, 4, 4))
    before = L.copy()
    got = NA.augment_lidar2img(L, params)
    assert got.dtype == np.float64 and got.shape == (6, 4, 4) and np.array_equal(L, before)
    p = rng.uniform(-30, 30, (50, 3))
    # the augmented points in float64: flip(scale * R p + t)
    q = (p @ NA.rotation_matrix(0.37).T) * 1.07 + np.array([0.4, -0.3, 0.2])
    q = q * np.array([-1.0 if flips[1] else 1.0, -1.0 if flips[0] else 1.0, 1.0])
    hp = np.concatenate([p, np.ones((50, 1))], 1)
    hq = np.concatenate([q, np.ones((50, 1))], 1)
    a = np.einsum("vij,nj->vni", L, hp)
    b = np.einsum("vij,nj->vni", got, hq)
    assert np.abs(a - b).max() <= 1e-9 * np.abs(a).max()
    assert np.array_equal(NA.augment_lidar2img(L[0], params), got[0])
    assert np.array_equal(NA.augment_lidar2img(L, dict()), L)
    with pytest.raises(ValueError):
        NA.augment_lidar2img(np.eye(3), params)


# ---- the plan of a config ----------------------------------------------------------------------------------------
CLASSES = ["car", "truck", "bus"]
PCR = [-54.0, -54.0, -5.0, 54.0, 54.0, 3.0]


def _cfg(steps, wrap=True):
    ds = dict(type="SomeDataset", pipeline=steps)
    return dict(data=dict(train=dict(type="CBGSDataset", dataset=ds) if wrap else ds))


def _tail(coop=""):
    return [dict(type="PointsRangeFilter" + coop, point_cloud_range=PCR),
            dict(type="ObjectRangeFilter", point_cloud_range=PCR),
            dict(type="ObjectNameFilter", classes=CLASSES),
            dict(type="PointShuffle" + coop)]


def test_train_plan_coop_unified():
    from projects.mmdet3d_plugin import native_aug as NA
    steps = [dict(type="LoadPointsFromFileCoop", load_dim=5, use_dim=5),
             dict(type="UnifiedObjectSampleCoop", sample_2d=True, db_sampler=dict(type="UnifiedDataBaseSampler")),
             dict(type="GlobalRotScaleTransAllCoop", rot_range=[-0.3925, 0.3925], scale_ratio_range=[0.95, 1.05],
                  translation_std=[0, 0, 0])] + _tail("Coop")
    assert NA.train_plan_from_config(_cfg(steps)) == dict(
        sampler="UnifiedObjectSampleCoop", paste_first=False, image_paste=True, rot_range=[-0.3925, 0.3925],
        scale_ratio_range=[0.95, 1.05], translation_std=[0.0, 0.0, 0.0], flip_ratio_bev_horizontal=None,
        flip_ratio_bev_vertical=None, point_cloud_range=PCR, object_range=PCR, num_classes=3, shuffle=True)


def test_train_plan_nus_unified():
    from projects.mmdet3d_plugin import native_aug as NA
    steps = [dict(type="UnifiedObjectSample", sample_2d=False),
             dict(type="ModalMask3D", mode="test"),
             dict(type="GlobalRotScaleTransAll", rot_range=0.785, translation_std=0.5),
             dict(type="CustomRandomFlip3D", sync_2d=False, flip_ratio_bev_horizontal=0.5,
                  flip_ratio_bev_vertical=0.25)] + _tail()
    plan = NA.train_plan_from_config(_cfg(steps, wrap=False))
    assert plan == dict(sampler="UnifiedObjectSample", paste_first=False, image_paste=False, rot_range=[-0.785, 0.785],
                        scale_ratio_range=[0.95, 1.05], translation_std=[0.5, 0.5, 0.5], flip_ratio_bev_horizontal=0.5,
                        flip_ratio_bev_vertical=0.25, point_cloud_range=PCR, object_range=PCR, num_classes=3,
                        shuffle=True)


def test_train_plan_nus_object_sample():
    from projects.mmdet3d_plugin import native_aug as NA
    steps = [dict(type="ObjectSample", db_sampler=dict()),
             dict(type="GlobalRotScaleTrans", rot_range=[-0.785, 0.785], scale_ratio_range=[0.9, 1.1],
                  translation_std=[0.5, 0.5, 0.5]),
             dict(type="RandomFlip3D", sync_2d=False, flip_ratio_bev_horizontal=0.5, flip_ratio_bev_vertical=0.5),
             dict(type="PointsRangeFilter", point_cloud_range=PCR)]
    plan = NA.train_plan_from_config(_cfg(steps))
    assert plan["sampler"] == "ObjectSample" and plan["paste_first"] is True and plan["image_paste"] is False
    assert plan["object_range"] is None and plan["num_classes"] is None and plan["shuffle"] is False
    assert plan["flip_ratio_bev_vertical"] == 0.5 and plan["scale_ratio_range"] == [0.9, 1.1]
    assert NA.train_plan_from_config(_cfg([dict(type="ObjectSampleCoop")]))["paste_first"] is True
    empty = NA.train_plan_from_config(_cfg([dict(type="LoadPointsFromFile")]))
    assert empty["sampler"] is None and empty["rot_range"] is None and empty["flip_ratio_bev_horizontal"] is None


@pytest.mark.parametrize("step,text", [
    (dict(type="GlobalRotScaleTransAll", shift_height=True), "shift_height"),
    (dict(type="GlobalRotScaleTransCoop", shift_height=True), "shift_height"),
    (dict(type="ModalMask3D", mode="train"), "ModalMask3D"),
    (dict(type="GlobalRotScaleTransImage", rot_range=[-0.3, 0.3]), "GlobalRotScaleTransImage"),
    (dict(type="RandomFlip3D", flip_ratio_bev_horizontal=0.5), "sync_2d"),
])
def test_train_plan_refusals(step, text):
    from projects.mmdet3d_plugin import native_aug as NA
    with pytest.raises(NotImplementedError, match=text):
        NA.train_plan_from_config(_cfg([dict(type="LoadPointsFromFile"), step] + _tail()))


NUS_PCR = [-54.0, -54.0, -5.0, 54.0, 54.0, 3.0]
REF_PLANS = {
    "CMT_Nuscenes/lidar/cmt_lidar_voxel0075_cbgs.py": dict(
        sampler="ObjectSample", paste_first=True, image_paste=False, rot_range=[-0.785, 0.785],
        scale_ratio_range=[0.9, 1.1], translation_std=[0.5, 0.5, 0.5], flip_ratio_bev_horizontal=0.5,
        flip_ratio_bev_vertical=0.5, point_cloud_range=NUS_PCR, object_range=NUS_PCR, num_classes=10, shuffle=True),
    "CMT_Nuscenes/fusion/cmt_voxel0075_vov_1600x640_cbgs.py": "ModalMask3D",
    "CMT_Nuscenes/fusion/cmt_voxel0100_r50_800x320_cbgs.py": "ModalMask3D",
    "CMT_Nuscenes/camera/cmt_camera_vov_1600x640_cbgs.py": "GlobalRotScaleTransImage",
}


@pytest.mark.parametrize("name", sorted(REF_PLANS))
def test_train_plan_from_reference_config(name):
    if not os.path.isdir(REF_CONFIGS):
        pytest.skip("reference checkout not present")
    from projects.mmdet3d_plugin import native_aug as NA
    from projects.mmdet3d_plugin.config import load_config
    cfg = load_config(os.path.join(REF_CONFIGS, name))
    want = REF_PLANS[name]
    if isinstance(want, str):
        with pytest.raises(NotImplementedError, match=want):
            NA.train_plan_from_config(cfg)
    else:
        assert NA.train_plan_from_config(cfg) == want


@pytest.mark.parametrize("name", ["fusion/coop/cmt_voxel0075_vov_1600x640_cbgs_a9coop_pretrained.py",
                                  "lidar/coop/cmt_lidar_voxel0075_cbgs_a9coop_pretrained.py",
                                  "lidar/vehicle/cmt_lidar_voxel0075_cbgs_a9coop_vehicle_pretrained.py",
                                  "fusion/infra/cmt_voxel0075_vov_1600x640_cbgs_a9coop_infrastructure_pretrained.py"])
def test_train_plan_from_reference_coop_config(name):
    if not os.path.isdir(REF_CONFIGS):
        pytest.skip("reference checkout not present")
    from projects.mmdet3d_plugin import native_aug as NA
    from projects.mmdet3d_plugin.config import load_config
    cfg = load_config(os.path.join(REF_CONFIGS, "CMTCoop_TUMTraf", name))
    plan = NA.train_plan_from_config(cfg)
    assert plan["sampler"] in ("UnifiedObjectSampleCoop", "UnifiedObjectSample", "ObjectSampleCoop", "ObjectSample")
    assert plan["paste_first"] == (plan["sampler"] in ("ObjectSampleCoop", "ObjectSample"))
    assert plan["rot_range"] == [-0.3925, 0.3925] and plan["scale_ratio_range"] == [0.95, 1.05]
    assert plan["translation_std"] == [0.0, 0.0, 0.0] and plan["flip_ratio_bev_horizontal"] is None
    assert plan["shuffle"] is True and plan["num_classes"] == len(cfg["class_names"])
    assert plan["point_cloud_range"] == plan["object_range"] == [float(v) for v in cfg["point_cloud_range"]]
    assert plan["image_paste"] == ("fusion" in name)


# ---- wrapper argument errors (before any device check: every tensor here is a CPU tensor) -----------------------
def test_wrapper_argument_errors():
    from projects.mmdet3d_plugin import native_aug as NA
    p, b = torch.zeros((4, 5)), torch.zeros((2, 7))
    lab = torch.zeros(2, dtype=torch.int64)
    cnt = torch.zeros(1, dtype=torch.int32)
    bad_points = [
        (NA.points_in_boxes, (p.double(), b), {}),
        (NA.points_in_boxes, (p[:, :2], b), {}),
        (NA.points_in_boxes, (p, b[:, :6]), {}),
        (NA.points_in_boxes, (p, b), dict(want=("box_of_point", "volume"))),
        (NA.points_in_boxes, (p, b), dict(want=())),
        (NA.points_in_boxes, (p, b), dict(count=torch.zeros(1))),
        (NA.points_in_boxes, (p.t().contiguous().t(), b), {}),
        (NA.points_in_boxes, (p, b), {}),                                   # CPU tensors: no CPU path
        (NA.augment_points, (p, dict(colour=1)), {}),
        (NA.augment_points, (p, dict(angle=float("nan"))), {}),
        (NA.augment_points, (p, dict(scale=float("inf"))), {}),
        (NA.augment_points, (p, dict(trans=[0, 1])), {}),
        (NA.augment_points, (p, dict(trans=[0, 1, float("nan")])), {}),
        (NA.augment_points, (p, [0.1, 1.0]), {}),
        (NA.augment_points, (p, {}), dict(point_cloud_range=[0, 0, 0, 1, 1, 0])),
        (NA.augment_points, (p, {}), dict(point_cloud_range=[0, 0, 0, 1, 1])),
        (NA.augment_points, (p, {}), dict(paste_points=p)),
        (NA.augment_points, (p, {}), dict(paste_points=p[:, :4].contiguous(), paste_boxes=b)),
        (NA.augment_points, (p, {}), dict(paste_points=p, paste_boxes=torch.zeros((129, 7)))),
        (NA.augment_points, (p, {}), dict(shuffle=torch.zeros(4, dtype=torch.int64))),
        (NA.augment_points, (p, {}), dict(shuffle=torch.zeros(5, dtype=torch.int32))),
        (NA.augment_points, (p, {}), dict(shuffle="yes")),
        (NA.augment_points, (p, {}), dict(count=torch.zeros(2, dtype=torch.int32))),
        (NA.augment_points, (torch.zeros((4, 9)), {}), {}),
        (NA.augment_points, (p, {}), dict(count=cnt)),                      # CPU tensors: no CPU path
        (NA.augment_boxes, (b, lab.int(), {}), dict(num_classes=3)),
        (NA.augment_boxes, (b, lab[:1], {}), dict(num_classes=3)),
        (NA.augment_boxes, (torch.zeros((2, 8)), lab, {}), dict(num_classes=3)),
        (NA.augment_boxes, (b, lab, {}), dict(num_classes=-1)),
        (NA.augment_boxes, (b, lab, {}), dict(num_classes=3, paste_boxes=b)),
        (NA.augment_boxes, (b, lab, {}), dict(num_classes=3, paste_boxes=torch.zeros((2, 9)), paste_labels=lab)),
        (NA.augment_boxes, (b, lab, dict(angle=float("inf"))), dict(num_classes=3)),
        (NA.augment_boxes, (b, lab, {}), dict(num_classes=3, point_cloud_range=[1, 0, 0, 1, 1, 1])),
        (NA.augment_boxes, (b, lab, {}), dict(num_classes=3)),              # CPU tensors: no CPU path
    ]
    for fn, args, kw in bad_points:
        with pytest.raises(ValueError):
            fn(*args, **kw)
    with pytest.raises(TypeError):
        NA.augment_boxes(b, lab, {})                                        # num_classes is required


# ---- ABI ---------------------------------------------------------------------------------------------------------
def _lib():
    from projects.mmdet3d_plugin import native
    if not native.available():
        pytest.skip("libcmt_hip.so not built")
    return native, native.lib()


def test_aug_abi():
    native, L = _lib()
    from projects.mmdet3d_plugin import native_aug as NA
    assert L.cmt_abi_version() == 25
    for key, cls in (("points_in_boxes", native.PointsInBoxesArgs), ("pts_augment", native.PtsAugmentArgs),
                     ("boxes_augment", native.BoxesAugmentArgs)):
        assert native.STRUCTS[key] is cls
        assert getattr(L, f"cmt_{key}_args_size")() == ctypes.sizeof(cls), key
        assert hasattr(L, f"cmt_{key}")
    T, Cb = NA.tile_rows(), NA.box_chunk()
    assert T > 0 and T % 64 == 0 and 0 < Cb <= 256
    assert NA.workspace_bytes(0) == 0 and NA.workspace_bytes(1) == 4 == NA.workspace_bytes(T)
    assert NA.workspace_bytes(T + 1) == 8 and NA.workspace_bytes(304000) == 4 * -(-304000 // T)
    assert NA.MAX_PASTE_BOXES == 128


def test_null_structs_are_rejected():
    _, L = _lib()
    for name in ("cmt_points_in_boxes", "cmt_pts_augment", "cmt_boxes_augment"):
        assert getattr(L, name)(None, None) == 1001   # CMT_EINVAL
        assert name in L.cmt_last_error().decode()
