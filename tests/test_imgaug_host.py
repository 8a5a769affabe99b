"""CPU tests of the training-side image pipeline: the numpy restatement of the contracts (tests/_imgaug_ref.py)
against hand-computed answers, native_imgaug's host helpers (order of draws, matrices, paste plan, config plans)
and every argument check of the three entry points and their wrappers, through the loaded library where it is
built (no device is touched: every case is rejected before any device work).
"""
import ctypes
import math
import os

import numpy as np
import pytest
import torch

import _imgaug_ref as A
import _resize_ref as R

REF_CONFIGS = "/root/reference/projects/configs"
BGR = dict(mean=[103.530, 116.280, 123.675], std=[57.375, 57.120, 58.395])


def _img(h, w, seed, n=1):
    return np.random.default_rng(seed).integers(0, 256, (n, h, w, 3), dtype=np.uint8)


def _nia():
    from projects.mmdet3d_plugin import native_imgaug as NIA
    return NIA


# ---- the rotation ------------------------------------------------------------------------------------------------
def test_rotation_by_180_and_90_of_a_4x4_crop():
    """about (2, 2): 180 degrees reads T(4 - y, 4 - x), 90 degrees T(x, 4 - y); index 4 lies outside and reads 0"""
    NIA = _nia()
    T = np.arange(1, 49, dtype=np.int64).reshape(4, 4, 3)
    got180 = A.warp_sums(T, NIA.warp_inverse(4, 4, 180))
    got90 = A.warp_sums(T, NIA.warp_inverse(4, 4, 90))
    want180, want90 = np.zeros_like(T), np.zeros_like(T)
    for y in range(4):
        for x in range(4):
            if x >= 1 and y >= 1:
                want180[y, x] = 1024 * T[4 - y, 4 - x]
            if y >= 1:
                want90[y, x] = 1024 * T[x, 4 - y]
    assert np.array_equal(got180, want180)
    assert np.array_equal(got90, want90)
    assert (got180[0] == 0).all() and (got180[:, 0] == 0).all() and (got90[0] == 0).all()


def test_identity_is_a_pass_through_and_equals_the_resize_reference():
    NIA = _nia()
    assert NIA.warp_inverse(40, 16, 0) == list(A.IDENTITY) and NIA.warp_inverse(40, 16, -0.0) == list(A.IDENTITY)
    ix, fx, iy, fy = A.warp_coords(7, 5, A.IDENTITY)
    assert (fx == 0).all() and (fy == 0).all()
    assert np.array_equal(ix, np.broadcast_to(np.arange(7), (5, 7))) and np.array_equal(iy[:, 0], np.arange(5))
    src = _img(23, 37, 1, n=2)
    images = [dict(Hr=17, Wr=30, x0=3, y0=-2, flip=False, zero=False, iM=A.IDENTITY)] * 2
    got = A.augment(src, images, 20, 12, 16, 24, BGR["mean"], BGR["std"], True)
    want = R.reference(src, (30, 17), (3, -2, 20, 12), 16, 24, BGR["mean"], BGR["std"], True)
    assert np.array_equal(got.view(np.uint32), want.view(np.uint32))


def test_rotated_ramp_is_sampled_at_the_quantised_position():
    """b = x + 2 y is linear, so the bilinear sample equals the ramp at (ix + fx / 32, iy + fy / 32), times 1024"""
    NIA = _nia()
    h, w = 24, 40
    ramp = (np.arange(w)[None, :] + 2 * np.arange(h)[:, None]).astype(np.int64)
    T = np.repeat(ramp[..., None], 3, axis=2)
    for deg in (5.4, -17.0, 33.3):
        iM = NIA.warp_inverse(w, h, deg)
        ix, fx, iy, fy = A.warp_coords(w, h, iM)
        inside = (ix >= 0) & (ix + 1 < w) & (iy >= 0) & (iy + 1 < h)
        assert inside.sum() > 200
        want = 1024 * ix + 32 * fx + 2 * (1024 * iy + 32 * fy)
        got = A.warp_sums(T, iM)
        assert np.array_equal(got[inside], np.repeat(want[inside][:, None], 3, axis=1))
        # float64 agreement of the quantised position with the affine map, within the 1/32 pixel grid
        x, y = np.meshgrid(np.arange(w), np.arange(h))
        assert np.abs(ix + fx / 32 - (iM[0] * x + iM[1] * y + iM[2])).max() <= 1 / 32 + 1e-9


@pytest.mark.parametrize("flip", [False, True])
def test_window_overhangs_the_resized_image_on_four_sides(flip):
    src = _img(6, 7, 2)
    Hr, Wr, x0, y0, w, h = 8, 10, -2, -1, 14, 11
    resized = R.resize_u8(src, Hr, Wr)[0]
    want = np.zeros((h, w, 3), np.uint8)
    for y in range(h):
        for x in range(w):
            ry, rx = y0 + y, x0 + (w - 1 - x if flip else x)
            if 0 <= ry < Hr and 0 <= rx < Wr:
                want[y, x] = resized[ry, rx]
    want = R.normalise_pad(want[None], 12, 16, BGR["mean"], BGR["std"], False)
    got = A.augment(src, [dict(Hr=Hr, Wr=Wr, x0=x0, y0=y0, flip=flip)], w, h, 12, 16, BGR["mean"], BGR["std"], False)
    assert np.array_equal(got.view(np.uint32), want.view(np.uint32))
    zero = A.augment(src, [dict(Hr=Hr, Wr=Wr, x0=x0, y0=y0, flip=flip, zero=True)], w, h, 12, 16, BGR["mean"], BGR["std"], False)
    black = R.normalise_pad(np.zeros((1, h, w, 3), np.uint8), 12, 16, BGR["mean"], BGR["std"], False)
    assert np.array_equal(zero.view(np.uint32), black.view(np.uint32))


# ---- GridMask ----------------------------------------------------------------------------------------------------
def _grid_mask_loops(h, w, d, l, st_h, st_w, use_h, use_w, mode):
    """the reference's construction (grid_mask.py), r = 0 so that the rotation is the identity"""
    hh, ww = int(1.5 * h), int(1.5 * w)
    mask = np.ones((hh, ww), np.float32)
    if use_h:
        for i in range(hh // d):
            s = d * i + st_h
            t = min(s + l, hh)
            mask[s:t, :] *= 0
    if use_w:
        for i in range(ww // d):
            s = d * i + st_w
            t = min(s + l, ww)
            mask[:, s:t] *= 0
    mask = mask[(hh - h) // 2:(hh - h) // 2 + h, (ww - w) // 2:(ww - w) // 2 + w]
    return 1 - mask if mode == 1 else mask


@pytest.mark.parametrize("case", [(19, 30, 7, 3, 2, 5), (19, 30, 2, 1, 1, 0), (32, 64, 7, 4, 6, 0), (21, 10, 20, 10, 19, 13),
                                  (16, 16, 5, 4, 4, 4), (9, 33, 8, 1, 7, 7), (5, 7, 4, 2, 3, 1), (640, 1600, 333, 167, 200, 45)])
def test_grid_mask_predicate_equals_the_loop_construction(case):
    """includes d not dividing hh, st + l beyond hh (d = 20, l = 10, st = 19 of hh = 31) and both modes"""
    h, w, d, l, st_h, st_w = case
    for use_h, use_w in ((True, True), (True, False), (False, True), (False, False)):
        for mode in (0, 1):
            got = A.grid_mask(h, w, d, l, st_h, st_w, use_h, use_w, mode)
            want = _grid_mask_loops(h, w, d, l, st_h, st_w, use_h, use_w, mode)
            assert got.shape == (h, w) and np.array_equal(got, want), (case, use_h, use_w, mode)


def test_grid_mask_stores_the_product():
    src = _img(9, 12, 3)
    g = dict(d=3, l=2, st_h=1, st_w=0, use_h=True, use_w=True, mode=0)
    got = A.augment(src, [dict(Hr=9, Wr=12, x0=0, y0=0)], 12, 9, 12, 16, BGR["mean"], BGR["std"], False, grid=g)
    plain = A.augment(src, [dict(Hr=9, Wr=12, x0=0, y0=0)], 12, 9, 12, 16, BGR["mean"], BGR["std"], False)
    m = A.grid_mask(12, 16, **g)
    assert set(np.unique(m)) == {0.0, 1.0}
    assert np.array_equal(got[0, :, m == 1], plain[0, :, m == 1]) and (got[0, :, m == 0] == 0).all()
    assert np.signbit(got[0, :, m == 0]).any()   # a masked negative value is -0.f


# ---- the paste ---------------------------------------------------------------------------------------------------
def test_paste_rules():
    frames = _img(12, 15, 4, n=1)
    patch = _img(3, 5, 5)[0]
    raw = [np.array([[2, 1, 9, 8, -1]])]
    assert np.array_equal(A.paste(frames, raw, [], -1), frames)
    # m = 0.5: v * 0.5 + v * 0.5 == v exactly, raw boxes stay
    assert np.array_equal(A.paste(frames, raw, [], 0.5), frames)
    # m = 0.3: trunc(v * 0.7 + v * 0.3) in float64, which is v - 1 for the bytes whose two products round below v
    got = A.paste(frames, raw, [], 0.3)
    v = frames[0, 1:8, 2:9].astype(np.float64)
    want = np.array([[[math.floor(float(b) * (1.0 - 0.3) + float(b) * 0.3) for b in px] for px in row] for row in v.tolist()])
    assert np.array_equal(got[0, 1:8, 2:9], want)
    assert (want <= v).all() and (want >= v - 1).all() and (want != v).any()
    outside = np.ones(frames.shape[1:3], bool)
    outside[1:8, 2:9] = False
    assert np.array_equal(got[0][outside], frames[0][outside])
    # a sampled box: the resized patch, pasted or mixed
    plan = [np.array([[4, 2, 11, 9, 0]])]
    c = R.resize_u8(patch[None], 7, 7)[0]
    assert np.array_equal(A.paste(frames, plan, [patch], -1)[0, 2:9, 4:11], c)
    mixed = A.paste(frames, plan, [patch], 0.3)[0, 2:9, 4:11]
    assert np.array_equal(mixed, np.trunc(frames[0, 2:9, 4:11] * (1.0 - 0.3) + c * 0.3).astype(np.uint8))
    # overlapping boxes follow the list order: the later one wins where both lie
    two = [np.array([[0, 0, 8, 8, 0], [4, 4, 12, 12, 1]])]
    p0, p1 = np.full((2, 2, 3), 10, np.uint8), np.full((1, 1, 3), 200, np.uint8)
    got = A.paste(frames, two, [p0, p1], -1)[0]
    assert (got[:4, :8] == 10).all() and (got[4:12, 4:12] == 200).all() and (got[4:8, :4] == 10).all()
    rev = A.paste(frames, [two[0][::-1]], [p0, p1], -1)[0]
    assert (rev[:8, :8] == 10).all() and (rev[8:12, 4:12] == 200).all()
    # an empty patch is skipped, whatever the rate
    skip = [np.array([[0, 0, 8, 8, 0]])]
    for m in (-1, 0.5):
        assert np.array_equal(A.paste(frames, skip, [np.zeros((0, 0, 3), np.uint8)], m), frames)


# ---- host helpers ------------------------------------------------------------------------------------------------
CONF = dict(resize_lim=(0.94, 1.25), final_dim=(640, 1600), bot_pct_lim=(0.0, 0.1), rot_lim=(-5.4, 5.4), H=900, W=1600,
            rand_flip=True)


def _replay(rs, conf):
    """the reference's _sample_augmentation(training=True), call for call"""
    H, W = conf["H"], conf["W"]
    fH, fW = conf["final_dim"]
    resize = rs.uniform(*conf["resize_lim"])
    newW, newH = int(W * resize), int(H * resize)
    crop_h = int((1 - rs.uniform(*conf["bot_pct_lim"])) * newH) - fH
    crop_w = int(rs.uniform(0, max(0, newW - fW)))
    flip = False
    if conf["rand_flip"] and rs.choice([0, 1]):
        flip = True
    rotate = rs.uniform(*conf["rot_lim"])
    return dict(resize=resize, resize_dims=(newW, newH), crop=(crop_w, crop_h, crop_w + fW, crop_h + fH), flip=flip, rotate=rotate)


@pytest.mark.parametrize("pic_wise", [False, True])
@pytest.mark.parametrize("rand_flip", [False, True])
def test_order_of_draws(pic_wise, rand_flip):
    NIA = _nia()
    conf = dict(CONF, rand_flip=rand_flip)
    a, b = np.random.RandomState(7), np.random.RandomState(7)
    got = NIA.sample_images_plan(conf, a, 3, pic_wise=pic_wise) + NIA.sample_images_plan(conf, a, 1, pic_wise=pic_wise)
    want = []
    for n in (3, 1):   # the coop sample: the infrastructure images, then the vehicle's
        aug = _replay(b, conf)
        for _ in range(n):
            if pic_wise:
                aug = _replay(b, conf)
            want.append(aug)
    assert got == want
    assert a.rand() == b.rand()   # the same number of draws consumed
    assert (got[0] == got[1]) == (not pic_wise)
    test = NIA.sample_image_augmentation(conf, a, training=False)
    assert test == dict(resize=1.0, resize_dims=(1600, 900), crop=(0, 215, 1600, 855), flip=False, rotate=0)
    assert a.rand() == b.rand()   # test mode draws nothing


def test_modal_mask_grid_mask_and_bev_draws():
    NIA = _nia()

    class Fixed:
        def __init__(self, v):
            self.v = v

        def rand(self):
            return self.v

    assert [NIA.sample_modal_mask(Fixed(v)) for v in (0.76, 0.75, 0.51, 0.5, 0.1)] == ["image", "points", "points", None, None]
    conf = dict(NIA.DETECTOR_GRID_MASK)
    a, b = np.random.RandomState(3), np.random.RandomState(3)
    got = [NIA.sample_grid_mask(conf, 640, a) for _ in range(8)]
    want = []
    for _ in range(8):
        if b.rand() > 0.7:
            want.append(None)
            continue
        d = b.randint(2, 640)
        st_h, st_w = b.randint(d), b.randint(d)
        b.randint(1)
        want.append(dict(d=d, l=min(max(int(d * 0.5 + 0.5), 1), d - 1), st_h=st_h, st_w=st_w, use_h=True, use_w=True, mode=1))
    assert got == want and None in got and any(g is not None for g in got)
    assert NIA.sample_grid_mask(conf, 640, a, training=False) is None and b.rand() is not None and a.rand() == b.rand()
    for bad in (dict(conf, rotate=2), dict(conf, offset=True)):
        with pytest.raises(NotImplementedError):
            NIA.sample_grid_mask(bad, 640, a)
    step = dict(rot_range=[-0.3925, 0.3925], scale_ratio_range=[0.95, 1.05], reverse_angle=True, flip_dx_ratio=0.5,
                flip_dy_ratio=0.5)
    a, b = np.random.RandomState(5), np.random.RandomState(5)
    params, box_params = NIA.sample_bev_image_augmentation(step, a)
    angle, scale = b.uniform(-0.3925, 0.3925), b.uniform(0.95, 1.05)
    dx, dy = b.rand() < 0.5, b.rand() < 0.5
    assert params == dict(angle=angle, scale=scale, trans=None, flip_h=bool(dy), flip_v=bool(dx))
    assert box_params == dict(params, angle=-angle)
    same, same_box = NIA.sample_bev_image_augmentation(dict(step, reverse_angle=False), a)
    assert same == same_box
    from projects.mmdet3d_plugin import native_aug as NA
    assert set(params) == NA._PARAM_KEYS
    NA.augment_lidar2img(np.eye(4), params)   # the dict is of the form the existing helper takes


@pytest.mark.parametrize("flip", [False, True])
@pytest.mark.parametrize("rotate", [0.0, 5.4, -90.0])
def test_train_image_lidar2img(flip, rotate):
    """the pixel of a projected point, resized, cropped, mirrored and rotated, is its projection through the result"""
    NIA = _nia()
    K = np.array([[1266.4, 0.0, 816.2], [0.0, 1266.4, 491.5], [0.0, 0.0, 1.0]])
    E = np.array([[0.0, -1.0, 0.0, 0.5], [0.0, 0.0, -1.0, 1.5], [1.0, 0.0, 0.0, -2.0], [0.0, 0.0, 0.0, 1.0]])
    K0, E0 = K.copy(), E.copy()
    resize, crop = 1.1, (37, 215, 1637, 855)
    L = NIA.train_image_lidar2img(K, E, resize, crop, flip, rotate)
    assert np.array_equal(K, K0) and np.array_equal(E, E0) and L.shape == (4, 4)
    w, h = crop[2] - crop[0], crop[3] - crop[1]
    th = rotate / 180 * math.pi
    for p in ([12.0, 3.0, 1.0], [30.0, -7.5, 0.2], [8.0, 1.0, -1.0]):
        cam = E @ np.array(p + [1.0])
        u, v = (K @ cam[:3])[:2] / cam[2]
        u, v = u * resize - crop[0], v * resize - crop[1]
        if flip:
            u = w - u
        du, dv = u - w / 2, v - h / 2
        u, v = math.cos(th) * du + math.sin(th) * dv + w / 2, -math.sin(th) * du + math.cos(th) * dv + h / 2
        q = L @ np.array(p + [1.0])
        assert abs(q[0] / q[2] - u) <= 1e-9 * max(1.0, abs(u)) and abs(q[1] / q[2] - v) <= 1e-9 * max(1.0, abs(v))
        assert q[2] == cam[2]
    K4 = np.eye(4)
    K4[:3, :3] = K
    assert np.array_equal(NIA.train_image_lidar2img(K4, E, resize, crop, flip, rotate), L)
    if not flip and rotate == 0.0:
        from projects.mmdet3d_plugin import native_img as NI
        assert np.allclose(L, NI.resize_crop_lidar2img(K, E, resize, crop), rtol=0, atol=1e-9)
    with pytest.raises(ValueError):
        NIA.train_image_lidar2img(K[:2], E, resize, crop, flip, rotate)


def _box(cx, cy, cz, s):
    return np.array([[cx + dx * s, cy + dy * s, cz + dz * s] for dx in (-1, 1) for dy in (-1, 1) for dz in (-1, 1)], float)


def test_paste_plan_on_a_hand_built_scene():
    """camera at the origin looking along +z, focal length 100, principal point (50, 40), frame 80 x 100"""
    NIA = _nia()
    L = np.array([[100.0, 0, 50, 0], [0, 100.0, 40, 0], [0, 0, 1, 0], [0, 0, 0, 1]])
    near = _box(0.0, 0.0, 5.0, 1.0)        # depth 4..6
    far = _box(0.5, 0.1, 20.0, 2.0)        # depth 18..22
    behind = _box(0.0, 0.0, -5.0, 1.0)     # all depths negative
    straddle = _box(0.0, 0.0, 0.5, 1.0)    # some corners behind the camera
    thin = _box(0.0, 0.0, 100.0, 0.7)      # projects to about 1.4 pixels: int width 1
    mid = _box(-1.0, 0.5, 10.0, 1.0)       # a sampled box, depth 9..11
    corners = np.stack([near, far, behind, straddle, thin, mid])
    plan = NIA.paste_plan(corners, L[None], (80, 100), 1)
    assert len(plan) == 1 and plan[0].dtype == np.int32

    def rect(c):
        uv = c[:, :2] / c[:, 2:3] * 100.0 + np.array([50.0, 40.0])
        lo, hi = uv.min(0), uv.max(0)
        r = [int(lo[0]), int(lo[1]), int(hi[0]), int(hi[1])]
        return [min(max(r[0], 0), 99), min(max(r[1], 0), 79), min(max(r[2], 0), 99), min(max(r[3], 0), 79)]

    assert plan[0].tolist() == [rect(far) + [-1], rect(mid) + [0], rect(near) + [-1]]   # far to near
    assert rect(thin)[2] - rect(thin)[0] == 1
    assert rect(near) == [25, 15, 75, 65]
    unordered = NIA.paste_plan(corners, L[None], (80, 100), 1, by_depth=False)
    assert unordered[0].tolist() == [rect(near) + [-1], rect(far) + [-1], rect(mid) + [0]]
    # equal depths keep the stable ascending order, reversed
    twins = np.stack([near, near + np.array([0.5, 0, 0]), mid])
    assert [r[4] for r in NIA.paste_plan(twins, L[None], (80, 100), 2)[0].tolist()] == [1, 0, -1]
    none = NIA.paste_plan(np.stack([behind]), np.stack([L, L]), (80, 100), 0)
    assert [p.shape for p in none] == [(0, 5), (0, 5)]
    bad = L.copy()
    bad[0, 0] = np.inf
    with pytest.raises(ValueError):
        NIA.paste_plan(corners, bad[None], (80, 100), 1)
    for args in ((corners[:, :7], L[None], (80, 100), 1), (corners, L, (80, 100), 1), (corners, L[None], (80, 100), 9),
                 (corners, L[None], (0, 100), 1)):
        with pytest.raises(ValueError):
            NIA.paste_plan(*args)


# ---- config plans ------------------------------------------------------------------------------------------------
def _conf(rand_flip):
    return dict(resize_lim=(0.94, 1.25), final_dim=(640, 1600), bot_pct_lim=(0.0, 0.0), rot_lim=(0.0, 0.0), H=900, W=1600,
                rand_flip=rand_flip)


BEV = dict(rot_range=[-0.3925, 0.3925], scale_ratio_range=[0.95, 1.05], reverse_angle=False, flip_dx_ratio=0.0,
           flip_dy_ratio=0.0)
GM = dict(use_h=True, use_w=True, rotate=1, offset=False, ratio=0.5, mode=1, prob=0.7)


def _plan(rand_flip, **kw):
    base = dict(data_aug_conf=_conf(rand_flip), pic_wise=False, mean=(103.530, 116.280, 123.675),
                std=(57.375, 57.120, 58.395), to_rgb=False, size_divisor=32, image_paste=False, mixup_rate=-1.0,
                paste_by_depth=True, modal_mask=None, bev_image_step=None, grid_mask=None)
    base.update(kw)
    return base


T = "CMTCoop_TUMTraf"
REF_PLANS = {
    f"{T}/camera/coop/cmt_camera_vov_1600x640_cbgs_a9coop_pretrained.py": _plan(False, bev_image_step=BEV),
    f"{T}/camera/infra/cmt_camera_vov_1600x640_cbgs_a9coop_infrastructure_pretrained.py": _plan(False, bev_image_step=BEV),
    f"{T}/camera/vehicle/cmt_camera_vov_1600x640_cbgs_a9coop_vehicle_pretrained.py": _plan(False, bev_image_step=BEV),
    f"{T}/fusion/coop/cmt_voxel0075_vov_1600x640_cbgs_a9coop_pretrained.py":
        _plan(False, image_paste=True, mixup_rate=0.5, grid_mask=GM),
    f"{T}/fusion/infra/cmt_voxel0075_vov_1600x640_cbgs_a9coop_infrastructure_pretrained.py":
        _plan(False, image_paste=True, mixup_rate=0.5, grid_mask=GM),
    f"{T}/fusion/vehicle/cmt_voxel0075_vov_1600x640_cbgs_a9coop_vehicle_pretrained.py":
        _plan(False, image_paste=True, mixup_rate=0.5, grid_mask=GM),
    f"{T}/lidar/coop/cmt_lidar_voxel0075_cbgs_a9coop_pretrained.py": None,
    f"{T}/lidar/infra/cmt_lidar_voxel0075_cbgs_a9coop_infrastructure_pretrained.py": None,
    f"{T}/lidar/vehicle/cmt_lidar_voxel0075_cbgs_a9coop_vehicle_pretrained.py": None,
    "CMT_Nuscenes/camera/cmt_camera_vov_1600x640_cbgs.py": _plan(True, bev_image_step=dict(BEV, reverse_angle=True)),
    "CMT_Nuscenes/fusion/cmt_voxel0075_vov_1600x640_cbgs.py":
        _plan(True, image_paste=True, mixup_rate=0.5, modal_mask="train", grid_mask=GM),
    "CMT_Nuscenes/fusion/cmt_voxel0100_r50_800x320_cbgs.py": "r50",
    "CMT_Nuscenes/lidar/cmt_lidar_voxel0075_cbgs.py": None,
}


@pytest.mark.parametrize("name", sorted(REF_PLANS))
def test_image_train_plan_from_reference_config(name):
    if not os.path.isdir(REF_CONFIGS):
        pytest.skip("reference checkout not present")
    NIA = _nia()
    from projects.mmdet3d_plugin.config import load_config
    plan = NIA.image_train_plan_from_config(load_config(os.path.join(REF_CONFIGS, name)))
    want = REF_PLANS[name]
    if want == "r50":   # the 800 x 320 config: its own sizes and limits, the same steps as the 1600 x 640 one
        assert plan["data_aug_conf"]["final_dim"] == (320, 800) and plan["data_aug_conf"]["rand_flip"] is True
        assert plan["image_paste"] is True and plan["mixup_rate"] == 0.5 and plan["modal_mask"] == "train"
        assert plan["grid_mask"] == GM and plan["bev_image_step"] is None and plan["size_divisor"] == 32
        return
    if want is not None:
        assert {k: tuple(v) if isinstance(v, (list, tuple)) else v for k, v in plan["data_aug_conf"].items()} == want["data_aug_conf"]
        plan = dict(plan, data_aug_conf=want["data_aug_conf"])
    assert plan == want


def _cfg(steps, model=None):
    return dict(data=dict(train=dict(type="CBGSDataset", dataset=dict(pipeline=steps))), model=model or {})


def test_image_train_plan_from_a_plain_dict():
    NIA = _nia()
    steps = [dict(type="UnifiedObjectSample", sample_2d=True, sample_method="by_order", mixup_rate=0.25, db_sampler={}),
             dict(type="ModalMask3D", mode="test", mask_modal="points"),
             dict(type="ResizeCropFlipImage", data_aug_conf=_conf(True), training=True, pic_wise=True),
             dict(type="NormalizeMultiviewImage", mean=[1, 2, 3], std=[4, 5, 6]),
             dict(type="PadMultiViewImage", size_divisor=16)]
    plan = NIA.image_train_plan_from_config(_cfg(steps, dict(use_grid_mask=True)))
    assert plan == dict(data_aug_conf=_conf(True), pic_wise=True, mean=(1, 2, 3), std=(4, 5, 6), to_rgb=True,
                        size_divisor=16, image_paste=True, mixup_rate=0.25, paste_by_depth=False, modal_mask="points",
                        bev_image_step=None, grid_mask=GM)
    assert NIA.image_train_plan_from_config(_cfg([dict(type="LoadPointsFromFile")])) is None
    with pytest.raises(NotImplementedError):
        NIA.image_train_plan_from_config(_cfg([dict(steps[0], modify_points=True)] + steps[1:]))
    with pytest.raises(ValueError):
        NIA.image_train_plan_from_config(_cfg(steps[:3]))
    with pytest.raises(ValueError):
        NIA.image_train_plan_from_config(_cfg(steps[:4] + [dict(type="PadMultiViewImage", size=(640, 1600))]))
    with pytest.raises(ValueError):
        NIA.image_train_plan_from_config(_cfg([dict(steps[2], training=False)] + steps[3:]))


# ---- wrapper argument checks -------------------------------------------------------------------------------------
def test_wrapper_argument_errors():
    NIA = _nia()
    fr = torch.zeros((2, 8, 9, 3), dtype=torch.uint8)
    ok = dict(resize_dims=(9, 8), crop=(0, 0, 6, 5), flip=False, rotate=0)
    gm = dict(d=4, l=2, st_h=1, st_w=3, use_h=True, use_w=True, mode=1)
    bad_aug = [
        ((fr.float(), [ok, ok]), {}),
        ((fr[0], [ok, ok]), {}),
        ((fr[:, :, :, :2], [ok, ok]), {}),
        ((fr.permute(0, 2, 1, 3), [ok, ok]), {}),
        ((torch.zeros((17, 2, 2, 3), dtype=torch.uint8), [ok] * 17), {}),
        ((fr, [ok]), {}),
        ((fr, [ok, dict(ok, crop=(0, 0, 7, 5))]), {}),
        ((fr, [ok, dict(ok, crop=(3, 0, 3, 5))]), {}),
        ((fr, [ok, dict(ok, resize_dims=(0, 8))]), {}),
        ((fr, [ok, dict(ok, resize_dims=(1 << 30, 8))]), {}),
        ((fr, [ok, dict(ok, crop=(1 << 30, 0, (1 << 30) + 6, 5))]), {}),
        ((fr, [ok, dict(ok, rotate=float("nan"))]), {}),
        ((fr, [ok, ok]), dict(size=(4, 8))),
        ((fr, [ok, ok]), dict(size_divisor=0)),
        ((fr, [ok, ok]), dict(std=[1.0, 0.0, 1.0])),
        ((fr, [ok, ok]), dict(zero=[True])),
        ((fr, [ok, ok]), dict(grid_mask=dict(gm, d=1))),
        ((fr, [ok, ok]), dict(grid_mask=dict(gm, l=4))),
        ((fr, [ok, ok]), dict(grid_mask=dict(gm, l=0))),
        ((fr, [ok, ok]), dict(grid_mask=dict(gm, st_h=4))),
        ((fr, [ok, ok]), dict(grid_mask=dict(gm, st_w=-1))),
        ((fr, [ok, ok]), dict(grid_mask=dict(gm, mode=2))),
        ((fr, [ok, ok]), dict(grid_mask=dict(d=4, l=2))),
        ((fr, [ok, ok]), dict(out=torch.zeros((2, 3, 32, 31)))),
        ((fr, [ok, ok]), {}),                                               # CPU tensors: no CPU path
    ]
    for args, kw in bad_aug:
        with pytest.raises(ValueError):
            NIA.augment_images(*args, **kw)
    x = torch.zeros((2, 3, 8, 9))
    for args in ((x.double(), gm), (x[0], gm), (x.permute(0, 1, 3, 2), gm), (x, dict(gm, d=0)), (x, dict(gm, l=9)), (x, gm)):
        with pytest.raises(ValueError):
            NIA.grid_mask_(*args)
    r = np.array([[0, 0, 4, 4, 0]], np.int32)
    p = [np.zeros((2, 2, 3), np.uint8)]
    bad_paste = [
        ((fr.float(), [r, r], p), {}),
        ((fr[0], [r, r], p), {}),
        ((fr.permute(0, 2, 1, 3), [r, r], p), {}),
        ((fr, [r], p), {}),
        ((fr, [r, r], p), dict(mixup_rate=1.5)),
        ((fr, [r, r], p), dict(mixup_rate=float("nan"))),
        ((fr, [r, r.astype(np.float32)], p), {}),
        ((fr, [r, r[:, :4]], p), {}),
        ((fr, [r, np.array([[0, 0, 10, 4, 0]])], p), {}),
        ((fr, [r, np.array([[0, 0, 4, 9, 0]])], p), {}),
        ((fr, [r, np.array([[-1, 0, 4, 4, 0]])], p), {}),
        ((fr, [r, np.array([[5, 0, 4, 4, 0]])], p), {}),
        ((fr, [r, np.array([[0, 0, 4, 4, 1]])], p), {}),
        ((fr, [r, np.array([[0, 0, 4, 4, -2]])], p), {}),
        ((fr, [r, np.tile(r, (257, 1))], p), {}),
        ((fr, [r, r], [np.zeros((2, 2, 4), np.uint8)]), {}),
        ((fr, [r, r], [np.zeros((2, 2, 3), np.float32)]), {}),
        ((torch.zeros((17, 2, 2, 3), dtype=torch.uint8), [r] * 17, p), {}),
        ((fr, [r, r], p), {}),                                              # CPU tensors: no CPU path
    ]
    for args, kw in bad_paste:
        with pytest.raises(ValueError):
            NIA.paste_images(*args, **kw)
    with pytest.raises(NotImplementedError):
        NIA.paste_images(fr, [r, r], p, modify_points=True)
    with pytest.raises(ValueError):
        NIA.sample_image_augmentation(dict(CONF, final_dim=(0, 1600)), np.random.RandomState(0))
    with pytest.raises(ValueError):
        NIA.warp_inverse(4, 4, float("inf"))


def test_grid_mask_module_host_side():
    from projects.mmdet3d_plugin.models.utils.grid_mask import GridMask
    for kw in (dict(rotate=2), dict(offset=True)):
        with pytest.raises(NotImplementedError):
            GridMask(True, True, **kw)
    gm = GridMask(True, True, rotate=1, offset=False, ratio=0.5, mode=1, prob=0.7)
    gm.set_prob(5, 20)
    assert gm.prob == 0.7 * 5 / 20 and gm.st_prob == 0.7
    x = torch.ones((1, 3, 8, 8))
    gm.eval()
    assert gm(x) is x                      # untouched outside training, on any device
    gm.train()
    gm.prob = -1.0
    assert gm(x) is x                      # rand() > prob


# ---- ABI ---------------------------------------------------------------------------------------------------------
def _lib():
    from projects.mmdet3d_plugin import native
    if not native.available():
        pytest.skip("libcmt_hip.so not built")
    return native, native.lib()


def test_imgaug_abi():
    native, L = _lib()
    assert L.cmt_abi_version() == 25
    for key, cls in (("img_augment", native.ImgAugmentArgs), ("grid_mask", native.GridMaskArgs),
                     ("img_paste", native.ImgPasteArgs)):
        assert native.STRUCTS[key] is cls
        assert getattr(L, f"cmt_{key}_args_size")() == ctypes.sizeof(cls), key
    assert native.IMG_AUG_MAX == 16 and native.PASTE_MAX_RECTS == 256
    assert ctypes.sizeof(native.PasteRect) == 20 and ctypes.sizeof(native.PastePatch) == 16
    for name in ("cmt_img_augment", "cmt_grid_mask", "cmt_img_paste"):
        assert getattr(L, name)(None, None) == 1001   # CMT_EINVAL
        assert name in L.cmt_last_error().decode()


def _aug_args(native, **kw):
    a = native.ImgAugmentArgs()
    a.N, a.Hs, a.Ws, a.to_rgb = 2, 8, 9, 0
    a.w, a.h, a.Hp, a.Wp = 6, 5, 8, 8
    for c in range(3):
        a.mean[c], a.inv_std[c] = 0.0, 1.0
    for n in range(2):
        im = a.img[n]
        im.Hr, im.Wr, im.x0, im.y0 = 8, 9, 0, 0
        im.iM[:] = [1.0, 0.0, 0.0, 0.0, 1.0, 0.0]
    a.src, a.dst = ctypes.c_void_p(4096), ctypes.c_void_p(8192)   # never dereferenced: every case is rejected
    for k, v in kw.items():
        if k.startswith("img1_"):
            if k == "img1_iM":
                a.img[1].iM[v[0]] = v[1]
            else:
                setattr(a.img[1], k[5:], v)
        elif k.startswith("grid_"):
            setattr(a.grid, k[5:], v)
        else:
            setattr(a, k, v)
    return a


GRID_OK = dict(grid_d=4, grid_l=2, grid_st_h=1, grid_st_w=3)


@pytest.mark.parametrize("bad", [
    dict(src=None), dict(dst=None), dict(N=0), dict(N=17), dict(Hs=0), dict(Ws=-1), dict(w=0), dict(h=0), dict(Hp=4),
    dict(Wp=5), dict(Hs=1 << 30), dict(Wp=1 << 30), dict(Hp=1 << 29, Wp=1 << 29), dict(dst=ctypes.c_void_p(8194)),
    dict(mean=(ctypes.c_float * 3)(0.0, float("nan"), 0.0)), dict(img1_Hr=0), dict(img1_Wr=1 << 30), dict(img1_x0=1 << 30),
    dict(img1_y0=-(1 << 30)), dict(img1_iM=(2, float("nan"))), dict(img1_iM=(4, float("inf"))), dict(img1_iM=(0, 1048576.0)),
    dict(img1_iM=(5, -1048576.0)), dict(grid_d=-1), dict(GRID_OK, grid_d=1, grid_l=0), dict(GRID_OK, grid_l=0),
    dict(GRID_OK, grid_l=4), dict(GRID_OK, grid_st_h=4), dict(GRID_OK, grid_st_h=-1), dict(GRID_OK, grid_st_w=4),
    dict(GRID_OK, grid_d=1 << 30)], ids=lambda d: "-".join(d) if isinstance(d, dict) else None)
def test_img_augment_rejects(bad):
    native, L = _lib()
    assert L.cmt_img_augment(ctypes.byref(_aug_args(native, **bad)), None) == 1001
    assert b"cmt_img_augment" in L.cmt_last_error()


def _gm_args(native, **kw):
    a = native.GridMaskArgs()
    a.planes, a.h, a.w = 6, 8, 9
    a.grid.d, a.grid.l, a.grid.st_h, a.grid.st_w = 4, 2, 1, 3
    a.x = ctypes.c_void_p(8192)
    for k, v in kw.items():
        if k.startswith("grid_"):
            setattr(a.grid, k[5:], v)
        else:
            setattr(a, k, v)
    return a


@pytest.mark.parametrize("bad", [dict(x=None), dict(x=ctypes.c_void_p(8193)), dict(planes=0), dict(h=0), dict(w=-2),
                                 dict(h=1 << 30), dict(planes=1 << 40), dict(grid_d=0), dict(grid_d=1), dict(grid_l=0),
                                 dict(grid_l=4), dict(grid_st_h=4), dict(grid_st_w=-1)], ids=lambda d: "-".join(d))
def test_grid_mask_rejects(bad):
    native, L = _lib()
    assert L.cmt_grid_mask(ctypes.byref(_gm_args(native, **bad)), None) == 1001
    assert b"cmt_grid_mask" in L.cmt_last_error()


def _paste_args(native, rect_rows, patch_rows, counts=(1, 0), **kw):
    """host tables for 2 cameras of 8 x 9; the device pointers are never dereferenced: every case is rejected"""
    a = native.ImgPasteArgs()
    a.N, a.Hs, a.Ws, a.n_patches = 2, 8, 9, len(patch_rows)
    table = (native.PasteRect * (2 * native.PASTE_MAX_RECTS))()
    for i, r in enumerate(rect_rows):
        table[i] = native.PasteRect(*r)
    ptab = (native.PastePatch * max(len(patch_rows), 1))()
    for i, p in enumerate(patch_rows):
        ptab[i] = native.PastePatch(*p)
    for i, c in enumerate(counts):
        a.count[i] = c
    a.mixup = -1.0
    a.rects, a.patches = ctypes.cast(table, ctypes.c_void_p), ctypes.cast(ptab, ctypes.c_void_p)
    a.rects_dev, a.patches_dev, a.patch_bytes = ctypes.c_void_p(4096), ctypes.c_void_p(8192), ctypes.c_void_p(12288)
    a.patch_bytes_size = 12
    a.frames = ctypes.c_void_p(16384)
    for k, v in kw.items():
        setattr(a, k, v)
    a._keep = (table, ptab)
    return a


OKR, OKP = [(0, 0, 4, 4, 0)], [(0, 2, 2)]


@pytest.mark.parametrize("rects,patches,kw", [
    (OKR, OKP, dict(frames=None)), (OKR, OKP, dict(N=0)), (OKR, OKP, dict(N=17)), (OKR, OKP, dict(Hs=0)),
    (OKR, OKP, dict(Ws=1 << 30)), (OKR, OKP, dict(n_patches=-1)), (OKR, OKP, dict(mixup=float("nan"))),
    (OKR, OKP, dict(mixup=1.25)), (OKR, OKP, dict(counts=(257, 0))), (OKR, OKP, dict(counts=(1, -1))),
    (OKR, OKP, dict(rects=None)), (OKR, OKP, dict(rects_dev=None)), (OKR, OKP, dict(patches=None)),
    (OKR, OKP, dict(patches_dev=None)), (OKR, OKP, dict(patch_bytes=None)), (OKR, OKP, dict(patch_bytes_size=11)),
    ([(0, 0, 10, 4, 0)], OKP, {}), ([(0, 0, 4, 9, 0)], OKP, {}), ([(-1, 0, 4, 4, 0)], OKP, {}), ([(0, -1, 4, 4, 0)], OKP, {}),
    ([(5, 0, 4, 4, 0)], OKP, {}), ([(0, 5, 4, 4, 0)], OKP, {}), ([(0, 0, 4, 4, 1)], OKP, {}), ([(0, 0, 4, 4, -2)], OKP, {}),
    (OKR, [(0, -1, 2)], {}), (OKR, [(0, 2, 1 << 15)], {}), (OKR, [(-1, 2, 2)], {}), (OKR, [(1, 2, 2)], {}),
    (OKR, [(13, 0, 0)], {})])
def test_img_paste_rejects(rects, patches, kw):
    native, L = _lib()
    kw = dict(kw)
    counts = kw.pop("counts", (1, 0))
    assert L.cmt_img_paste(ctypes.byref(_paste_args(native, rects, patches, counts, **kw)), None) == 1001
    assert b"cmt_img_paste" in L.cmt_last_error()


def test_img_paste_with_nothing_to_paste_launches_nothing():
    """empty lists and empty rectangles are legal and return before any device work"""
    native, L = _lib()
    assert L.cmt_img_paste(ctypes.byref(_paste_args(native, [], [], (0, 0))), None) == 0
    assert L.cmt_img_paste(ctypes.byref(_paste_args(native, [(3, 3, 3, 7, -1)], [], (1, 0))), None) == 0
