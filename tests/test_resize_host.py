"""Host side of the fused resize (cmt_img_resize_prepare): known answers of the numpy oracle tests/_resize_ref.py
that the GPU test is held to, the plan / lidar2img / config helpers of native_img, the ABI mirror and the
argument errors.  No GPU needed.

The oracle's distance from a float64 bilinear with the same taps is held strictly below 1.0 grey level at five
shapes.  Its parts: each coefficient rounding moves a sample by at most 255 / 4096 = 0.06 per axis, ``>> 4`` loses
less than 1 / 128, each of the two ``>> 16`` less than 0.25 (both downwards) and the final rounding at most 0.5;
the parts can add up to a little over 1.0 in principle, the largest distance seen at these shapes is 0.783.
"""
import ctypes
import os

import numpy as np
import pytest
import torch

import _resize_ref as R

REF_CONFIGS = "/root/reference/projects/configs"
SHAPES = [((1200, 1920), (900, 1600)), ((900, 1600), (450, 800)), ((37, 53), (29, 47)), ((24, 40), (31, 57)),
          ((33, 45), (33, 45))]


def _img(H, W, seed, n=1):
    return np.random.default_rng(seed).integers(0, 256, (n, H, W, 3), dtype=np.uint8)


# ---- the oracle's known answers ----------------------------------------------------------------------------------
def test_identity():
    src = _img(33, 45, 0, n=2)
    assert np.array_equal(R.resize_u8(src, 33, 45), src)


def test_exact_half_is_the_rounded_mean_of_four():
    src = _img(36, 64, 1)
    s = src.astype(np.int64)
    want = (s[:, 0::2, 0::2] + s[:, 0::2, 1::2] + s[:, 1::2, 0::2] + s[:, 1::2, 1::2] + 2) >> 2
    assert np.array_equal(R.resize_u8(src, 18, 32), want.astype(np.uint8))


def test_constants_are_preserved():
    """all 256 values, down (1.3333 / 1.2) and up (0.42 / 0.7): coefficient pairs sum to 2048"""
    src = np.broadcast_to(np.arange(256, dtype=np.uint8)[:, None, None, None], (256, 12, 18, 3))
    for Hr, Wr in ((9, 15), (29, 26)):
        out = R.resize_u8(src, Hr, Wr)
        assert np.array_equal(out, np.broadcast_to(np.arange(256, dtype=np.uint8)[:, None, None, None], out.shape))


@pytest.mark.parametrize("S,Rz", [(a, b) for (hs, ws), (hr, wr) in SHAPES for a, b in ((hs, hr), (ws, wr))])
@pytest.mark.parametrize("horizontal", [True, False])
def test_coefficient_pairs_sum_to_2048(S, Rz, horizontal):
    s0, s1, c0, c1 = R.axis_coefs(S, Rz, horizontal)
    assert np.all(c0 + c1 == R.COEF) and c0.min() >= 0 and c1.min() >= 0
    assert s0.min() >= 0 and s1.max() <= S - 1 and np.all((s1 == s0 + 1) | (s1 == s0))
    if horizontal:
        assert np.all(c1[s1 == s0] == 0)   # a clamped horizontal tap carries no weight


@pytest.mark.parametrize("src_hw,dst_hw", SHAPES)
def test_within_one_grey_level_of_float64_bilinear(src_hw, dst_hw):
    src = _img(*src_hw, seed=src_hw[0] + dst_hw[1])
    err = np.abs(R.resize_u8(src, *dst_hw).astype(np.float64) - R.resize_f64(src, *dst_hw)).max()
    print(f"resize {src_hw} -> {dst_hw}: max |fixed point - float64 bilinear| = {err:.4f} grey levels (bound < 1.0)")
    assert err < 1.0


def test_border_taps():
    """2.5 x upscale of 14 columns: the first and last resized columns copy the border pixel, rows only clamp"""
    src = _img(9, 14, 2)
    out = R.resize_u8(src, 22, 35)
    s0, s1, a0, a1 = R.axis_coefs(14, 35, True)
    assert s0[0] == 0 and a0[0] == 2048 and s0[-1] == 13 and a0[-1] == 2048 and (a1 == 0).sum() >= 2
    y0, y1, b0, b1 = R.axis_coefs(9, 22, False)
    assert y0[0] == 0 and y1[0] == 0 and y0[-1] == 8 and y1[-1] == 8
    assert np.array_equal(out[:, 0, 0], src[:, 0, 0]) and np.array_equal(out[:, -1, -1], src[:, -1, -1])


def test_reference_window_and_pad():
    src = _img(6, 7, 3, n=2)
    mean, std = [103.530, 116.280, 123.675], [57.375, 57.120, 58.395]
    out = R.reference(src, (7, 6), (-2, -1, 12, 9), 10, 13, mean, std, False)
    inv32 = (1.0 / np.asarray(std, np.float32).astype(np.float64)).astype(np.float32)
    outside = (np.float32(0) - np.asarray(mean, np.float32)) * inv32
    assert out.dtype == np.float32 and out.shape == (2, 3, 10, 13)
    assert np.array_equal(out[0, :, 0, 0], outside) and np.array_equal(out[1, :, 8, 11], outside)
    assert np.all(out[:, :, 9:] == 0) and np.all(out[:, :, :, 12:] == 0)
    inside = (src[0, 0, 0].astype(np.float32) - np.asarray(mean, np.float32)) * inv32
    assert np.array_equal(out[0, :, 1, 2], inside)
    gone = R.reference(src, (7, 6), (20, 20, 4, 4), 4, 4, mean, std, True)   # a window that misses the image
    assert np.all(gone[:, :, :4, :4] == outside[None, :, None, None])


def test_against_cv2():
    cv2 = pytest.importorskip("cv2")
    for (hs, ws), (hr, wr) in SHAPES[1:]:
        src = _img(hs, ws, 7)[0]
        assert np.array_equal(cv2.resize(src, (wr, hr), interpolation=cv2.INTER_LINEAR), R.resize_u8(src[None], hr, wr)[0])


# ---- native_img's host helpers -----------------------------------------------------------------------------------
def test_resize_crop_plan():
    from projects.mmdet3d_plugin import native_img as NI
    assert NI.resize_crop_plan((900, 1600), (640, 1600)) == (1.0, (1600, 900), (0, 260, 1600, 900))
    assert NI.resize_crop_plan((900, 1600), (320, 800)) == (0.5, (800, 450), (0, 130, 800, 450))
    resize, dims, crop = NI.resize_crop_plan((188, 320), (128, 320))
    assert (resize, crop) == NI.test_crop((188, 320), (128, 320)) and dims == (320, 188)
    assert NI.resize_crop_plan((900, 1600), (640, 1600), bot_pct_lim=(0.0, 0.2))[2] == (0, 170, 1600, 810)
    with pytest.raises(ValueError):
        NI.resize_crop_plan((0, 1600), (640, 1600))
    with pytest.raises(NotImplementedError):   # the integer-crop helper is unchanged
        NI.test_crop((900, 1600), (320, 800))


def test_resize_crop_lidar2img():
    from projects.mmdet3d_plugin import native_img as NI
    K = np.array([[1266.4, 0.0, 816.2], [0.0, 1266.4, 491.5], [0.0, 0.0, 1.0]])
    E = np.array([[0.0, -1.0, 0.0, 0.5], [0.0, 0.0, -1.0, 1.5], [1.0, 0.0, 0.0, -2.0], [0.0, 0.0, 0.0, 1.0]])
    got = NI.resize_crop_lidar2img(K, E, 0.5, (0, 130, 800, 450))
    hand = np.array([[633.2, 0.0, 408.1, 0.0], [0.0, 633.2, 245.75 - 130.0, 0.0], [0.0, 0.0, 1.0, 0.0],
                     [0.0, 0.0, 0.0, 1.0]]) @ E
    assert got.dtype == np.float64 and np.array_equal(got, hand)
    assert K[0, 0] == 1266.4 and K[1, 2] == 491.5   # the caller's matrix is not modified
    crop = (7, 260, 1607, 900)
    assert np.array_equal(NI.resize_crop_lidar2img(K, E, 1.0, crop), NI.crop_lidar2img(K, E, crop))
    K4 = np.eye(4)
    K4[:3, :3] = K
    assert np.array_equal(NI.resize_crop_lidar2img(K4, E, 0.5, crop), NI.resize_crop_lidar2img(K, E, 0.5, crop))
    with pytest.raises(ValueError):
        NI.resize_crop_lidar2img(np.eye(2), E, 1.0, crop)


PLANS = {
    "CMTCoop_TUMTraf/camera/coop/cmt_camera_vov_1600x640_cbgs_a9coop_pretrained.py": 1.0,
    "CMTCoop_TUMTraf/camera/infra/cmt_camera_vov_1600x640_cbgs_a9coop_infrastructure_pretrained.py": 1.0,
    "CMTCoop_TUMTraf/camera/vehicle/cmt_camera_vov_1600x640_cbgs_a9coop_vehicle_pretrained.py": 1.0,
    "CMTCoop_TUMTraf/fusion/coop/cmt_voxel0075_vov_1600x640_cbgs_a9coop_pretrained.py": 1.0,
    "CMTCoop_TUMTraf/fusion/infra/cmt_voxel0075_vov_1600x640_cbgs_a9coop_infrastructure_pretrained.py": 1.0,
    "CMTCoop_TUMTraf/fusion/vehicle/cmt_voxel0075_vov_1600x640_cbgs_a9coop_vehicle_pretrained.py": 1.0,
    "CMTCoop_TUMTraf/lidar/coop/cmt_lidar_voxel0075_cbgs_a9coop_pretrained.py": None,
    "CMTCoop_TUMTraf/lidar/infra/cmt_lidar_voxel0075_cbgs_a9coop_infrastructure_pretrained.py": None,
    "CMTCoop_TUMTraf/lidar/vehicle/cmt_lidar_voxel0075_cbgs_a9coop_vehicle_pretrained.py": None,
    "CMT_Nuscenes/camera/cmt_camera_vov_1600x640_cbgs.py": 1.0,
    "CMT_Nuscenes/fusion/cmt_voxel0075_vov_1600x640_cbgs.py": 1.0,
    "CMT_Nuscenes/fusion/cmt_voxel0100_r50_800x320_cbgs.py": 0.5,
    "CMT_Nuscenes/lidar/cmt_lidar_voxel0075_cbgs.py": None,
}


@pytest.mark.parametrize("name", sorted(PLANS))
def test_image_plan_from_reference_config(name):
    if not os.path.isdir(REF_CONFIGS):
        pytest.skip("reference checkout not present")
    from projects.mmdet3d_plugin import native_img as NI
    from projects.mmdet3d_plugin.config import load_config
    plan = NI.image_plan_from_config(load_config(os.path.join(REF_CONFIGS, name)))
    if PLANS[name] is None:
        assert plan is None
        return
    assert plan["resize"] == PLANS[name] and plan["size_divisor"] == 32 and plan["to_rgb"] is False
    assert plan["mean"] == NI.IMG_MEAN and plan["std"] == NI.IMG_STD
    if PLANS[name] == 1.0:
        assert plan["resize_dims"] == (1600, 900) and plan["crop"] == (0, 260, 1600, 900)
    else:
        assert plan["resize_dims"] == (800, 450) and plan["crop"] == (0, 130, 800, 450)


def test_image_plan_from_a_plain_dict():
    from projects.mmdet3d_plugin import native_img as NI
    aug = dict(H=1200, W=1920, final_dim=(640, 1600), bot_pct_lim=(0.0, 0.0))
    steps = [dict(type="LoadPointsFromFile"),
             dict(type="MultiScaleFlipAug3D", transforms=[
                 dict(type="ResizeCropFlipImageCoop", data_aug_conf=aug, training=False),
                 dict(type="NormalizeMultiviewImageCoop", mean=[1.0, 2.0, 3.0], std=[4.0, 5.0, 6.0], to_rgb=True),
                 dict(type="PadMultiViewImageCoop", size_divisor=16)])]
    plan = NI.image_plan_from_config(dict(data=dict(test=dict(pipeline=steps))))
    assert plan == dict(resize=1600 / 1920, resize_dims=(1600, int(1200 * (1600 / 1920))),
                        crop=(0, int(1200 * (1600 / 1920)) - 640, 1600, int(1200 * (1600 / 1920))), mean=(1.0, 2.0, 3.0),
                        std=(4.0, 5.0, 6.0), to_rgb=True, size_divisor=16)
    assert NI.image_plan_from_config(dict(data=dict(test=dict(pipeline=steps[:1])))) is None
    steps[1]["transforms"][0]["training"] = True
    with pytest.raises(ValueError, match="training"):
        NI.image_plan_from_config(dict(data=dict(test=dict(pipeline=steps))))


# ---- ABI and errors ----------------------------------------------------------------------------------------------
def _lib():
    from projects.mmdet3d_plugin import native
    if not native.available():
        pytest.skip("libcmt_hip.so not built")
    return native, native.lib()


def _resize_args(native, **kw):
    a = native.ImgResizeArgs()
    a.N, a.Hs, a.Ws, a.to_rgb, a.Hr, a.Wr = 1, 8, 8, 0, 6, 6
    a.x0, a.y0, a.w, a.h, a.Hp, a.Wp = 0, 0, 6, 6, 8, 8
    for c in range(3):
        a.mean[c], a.inv_std[c] = 0.0, 1.0
    a.src, a.dst = ctypes.c_void_p(4096), ctypes.c_void_p(8192)   # never dereferenced: every case is rejected
    for k, v in kw.items():
        setattr(a, k, v)
    return a


def test_img_resize_abi():
    native, L = _lib()
    assert L.cmt_abi_version() == 25
    assert L.cmt_img_resize_args_size() == ctypes.sizeof(native.ImgResizeArgs)
    assert native.STRUCTS["img_resize"] is native.ImgResizeArgs


@pytest.mark.parametrize("bad", [dict(Hr=0), dict(Wr=-3), dict(N=0), dict(Ws=0), dict(w=0), dict(Hp=5), dict(Wp=5),
                                 dict(src=None), dict(dst=ctypes.c_void_p(8194)), dict(x0=1 << 30), dict(Hr=1 << 30),
                                 dict(N=1 << 20, Hp=1 << 12, Wp=1 << 12, h=6, w=6)],
                         ids=lambda d: "-".join(d))
def test_img_resize_rejects(bad):
    native, L = _lib()
    assert L.cmt_img_resize_prepare(ctypes.byref(_resize_args(native, **bad)), None) == 1001
    assert b"cmt_img_resize_prepare" in L.cmt_last_error()
    assert L.cmt_img_resize_prepare(None, None) == 1001


def test_prepare_images_resize_errors():
    from projects.mmdet3d_plugin import native_img as NI
    ok = torch.zeros((2, 8, 8, 3), dtype=torch.uint8)
    for dims in ((0, 6), (6, -1), (6,), (1 << 30, 6)):
        with pytest.raises(ValueError, match="resize_dims"):
            NI.prepare_images(ok, resize_dims=dims)
    with pytest.raises(ValueError, match="below the crop"):
        NI.prepare_images(ok, resize_dims=(12, 10), size=(9, 12))
    with pytest.raises(ValueError, match="empty crop"):
        NI.prepare_images(ok, resize_dims=(12, 10), crop=(4, 4, 4, 8))
    with pytest.raises(ValueError, match="device"):
        NI.prepare_images(ok, resize_dims=(12, 10))
    with pytest.raises(ValueError, match="uint8"):
        NI.prepare_images(ok.float(), resize_dims=(12, 10))


def test_cli_ida_size_argument():
    import importlib.util
    from conftest import PKG
    spec = importlib.util.spec_from_file_location("cmt_test_cli_ida", os.path.join(PKG, "tools", "test.py"))
    cli = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(cli)
    base = ["cmtcoop_fusion_tumtraf", "--synthetic", "--detector", "--out", "x.json"]
    assert cli.parse_args(base).ida_size is None
    assert cli.parse_args(base + ["--frame-size", "1200", "1920", "--ida-size", "900", "1600"]).ida_size == [900, 1600]
