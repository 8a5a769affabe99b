"""Host-side checks of the detector layer: the registry builds CmtDetector / CmtCoopDetector from the
reference's configs and from the package's, the state-dict keys are the reference's, the cmt_img_prepare
entry checks its arguments before touching a device, and the image-pipeline helpers restate the reference's
test-time crop.  Nothing here needs a GPU."""
import ctypes
import os

import numpy as np
import pytest
import torch

from test_reference_configs import NAMES, REF_CONFIGS, _need_checkout

SMALL = dict(num_query=64, num_layers=2, grid_size=[256, 256, 40], spec_name="V-19-eSE")
PTS = ("pts_middle_encoder", "pts_backbone", "pts_neck")
IMG = ("img_backbone", "img_neck")
R50 = "CMT_Nuscenes/fusion/cmt_voxel0100_r50_800x320_cbgs.py"


def _small(name):
    from projects.mmdet3d_plugin import build_detector
    from projects.mmdet3d_plugin import synthetic as S
    cfg = S.make_detector_cfg(name, **SMALL)
    return build_detector(cfg), cfg


# ---- reference configs --------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", [n for n in NAMES if n != R50])
def test_reference_model_builds(name):
    _need_checkout()
    from projects.mmdet3d_plugin import build_detector
    from projects.mmdet3d_plugin.config import load_config
    from projects.mmdet3d_plugin.models.detectors import CmtCoopDetector, CmtDetector
    cfg = load_config(os.path.join(REF_CONFIGS, name))["model"]
    model = build_detector(cfg)
    assert type(model).__name__ == cfg["type"]
    lidar, camera = "/camera/" not in name, "/lidar/" not in name

    def check_branches(det):
        kids = dict(det.named_children())
        for k in PTS + ("pts_voxel_layer", "pts_voxel_encoder"):
            assert (k in kids) == lidar, (k, sorted(kids))
        for k in IMG:
            assert (k in kids) == camera, (k, sorted(kids))

    if cfg["type"] == "CmtCoopDetector":
        assert isinstance(model, CmtCoopDetector)
        agents = [a for a in ("vehicle_model", "infrastructure_model") if cfg.get(a)]
        assert agents and sorted(dict(model.named_children())) == sorted(agents + ["pts_bbox_head"])
        for a in agents:
            agent = getattr(model, a)
            assert type(agent) is CmtDetector and not agent.with_pts_bbox
            check_branches(agent)
    else:
        assert isinstance(model, CmtDetector) and model.with_pts_bbox
        check_branches(model)
    assert type(model.pts_bbox_head).__name__ == cfg["pts_bbox_head"]["type"]
    assert model.pts_bbox_head.test_cfg == cfg["test_cfg"]["pts"]


def test_r50_config_names_resnet():
    _need_checkout()
    from projects.mmdet3d_plugin import build_detector
    from projects.mmdet3d_plugin.config import load_config
    cfg = load_config(os.path.join(REF_CONFIGS, R50))["model"]
    with pytest.raises((NotImplementedError, KeyError), match="ResNet"):
        build_detector(cfg)


def test_registry_names():
    from projects.mmdet3d_plugin import registry as R
    assert "CmtDetector" in R.DETECTORS and "CmtCoopDetector" in R.DETECTORS
    assert "HardSimpleVFE" in R.VOXEL_ENCODERS
    assert R.build_model is R.build_detector
    vfe = R.build_voxel_encoder(dict(type="HardSimpleVFE", num_features=5))
    assert not list(vfe.state_dict())
    vox = torch.arange(24, dtype=torch.float32).view(2, 2, 6)
    vox[1, 1] = 0
    got = vfe(vox, torch.tensor([2, 1]), None)
    assert torch.equal(got, torch.stack([vox[0, :, :5].mean(0), vox[1, 0, :5]]))


# ---- state-dict keys ------------------------------------------------------------------------------------------
def _branch_keys(cfg):
    from projects.mmdet3d_plugin import registry as R
    build = dict(img_backbone=R.build_backbone, img_neck=R.build_neck, pts_middle_encoder=R.build_middle_encoder,
                 pts_backbone=R.build_backbone, pts_neck=R.build_neck)
    return {k: set(build[k](cfg[k]).state_dict()) for k in IMG + PTS}


def _head_keys(cfg):
    from projects.mmdet3d_plugin import build_head
    head = dict(cfg["pts_bbox_head"], train_cfg=None, test_cfg=cfg["test_cfg"]["pts"])
    return set(build_head(head).state_dict())


def test_fusion_detector_keys():
    model, cfg = _small("cmt_fusion_nus")
    keys = set(model.state_dict())
    branches = dict(_branch_keys(cfg), pts_bbox_head=_head_keys(cfg))
    for prefix, want in branches.items():
        got = {k[len(prefix) + 1:] for k in keys if k.startswith(prefix + ".")}
        assert want and got == want, prefix
    assert all(k.split(".")[0] in branches for k in keys)


def test_coop_detector_keys():
    model, cfg = _small("cmtcoop_fusion_tumtraf")
    keys = set(model.state_dict())
    seen = set()
    for agent in ("vehicle_model", "infrastructure_model"):
        for prefix, want in _branch_keys(cfg[agent]).items():
            full = f"{agent}.{prefix}."
            got = {k[len(full):] for k in keys if k.startswith(full)}
            assert want and got == want, full
            seen |= {full + k for k in got}
    head = {k[len("pts_bbox_head."):] for k in keys if k.startswith("pts_bbox_head.")}
    assert head == _head_keys(cfg)
    assert seen | {"pts_bbox_head." + k for k in head} == keys


def test_merged_checkpoint_loads():
    from projects.mmdet3d_plugin.checkpoint import load_detector_checkpoint, merge_coop_checkpoints
    coop, _ = _small("cmtcoop_fusion_tumtraf")
    sd_v = _small("cmt_fusion_nus")[0].state_dict()
    torch.manual_seed(1)
    single_i = _small("cmt_fusion_nus")[0]
    with torch.no_grad():
        single_i.pts_middle_encoder.conv_input[0].weight.normal_()
    sd_i = single_i.state_dict()
    merged = merge_coop_checkpoints(vehicle=sd_v, infrastructure=sd_i)
    assert merged and set(merged) <= set(coop.state_dict())
    missing, unexpected = load_detector_checkpoint(coop, {"state_dict": merged, "meta": {}}, strict=False)
    assert not unexpected
    assert missing and all(k.startswith("pts_bbox_head.task_heads.") for k in missing)
    # the converter writes the sparse kernels in the other layout; they arrive in this package's
    w = coop.infrastructure_model.pts_middle_encoder.conv_input[0].weight
    assert torch.equal(w, single_i.pts_middle_encoder.conv_input[0].weight)
    k = next(k for k in sd_v if k.startswith("img_backbone.") and k.endswith("weight"))
    assert torch.equal(coop.state_dict()["vehicle_model." + k], sd_v[k])
    # a bare state dict of the detector itself loads strictly
    assert load_detector_checkpoint(coop, coop.state_dict()) == ([], [])


def test_detector_cfg_geometry():
    from projects.mmdet3d_plugin import synthetic as S
    cfg = S.make_detector_cfg("cmt_fusion_nus", **SMALL)
    pcr = cfg["pts_voxel_layer"]["point_cloud_range"]
    assert pcr == pytest.approx([-9.6, -9.6, -5.0, 9.6, 9.6, 3.0])
    assert cfg["pts_middle_encoder"]["sparse_shape"] == [41, 256, 256]
    assert cfg["pts_bbox_head"]["bbox_coder"]["pc_range"] == pcr and cfg["test_cfg"]["pts"]["pc_range"] == pcr
    assert cfg["test_cfg"]["pts"]["grid_size"] == [256, 256, 40]
    full = S.make_detector_cfg("cmtcoop_lidar_tumtraf")
    assert full["type"] == "CmtCoopDetector" and "img_backbone" not in full["vehicle_model"]
    assert full["vehicle_model"]["pts_middle_encoder"]["sparse_shape"] == [41, 1440, 1440]
    assert full["vehicle_model"]["pts_voxel_layer"]["point_cloud_range"] == [-72.0, -72.0, -8, 72.0, 72.0, 0]
    fr = S.synthetic_frames(2, 5, 7, seed=3)
    assert fr.dtype == torch.uint8 and tuple(fr.shape) == (2, 5, 7, 3) and torch.equal(fr, S.synthetic_frames(2, 5, 7, 3))


# ---- ABI --------------------------------------------------------------------------------------------------------
def _prep_args(native, **kw):
    a = native.ImgPrepareArgs()
    a.N, a.Hs, a.Ws, a.to_rgb, a.x0, a.y0, a.w, a.h, a.Hp, a.Wp = 2, 9, 14, 0, 3, 2, 7, 5, 8, 8
    for c in range(3):
        a.mean[c], a.inv_std[c] = 100.0, 0.017
    a.src, a.dst = ctypes.c_void_p(4096), ctypes.c_void_p(8192)   # never dereferenced: the checks fail first
    for k, v in kw.items():
        setattr(a, k, v)
    return a


def test_img_prepare_abi():
    from projects.mmdet3d_plugin import native
    L = native.lib()
    assert L.cmt_abi_version() == 25 and native.ABI_VERSION == 25
    assert L.cmt_img_prepare_args_size() == ctypes.sizeof(native.ImgPrepareArgs)


@pytest.mark.parametrize("bad", [dict(src=None), dict(dst=None), dict(Hp=4), dict(Wp=6), dict(N=0), dict(w=0),
                                 dict(h=0), dict(Hs=0), dict(x0=-2 ** 30), dict(N=2 ** 30, Hp=2 ** 20, Wp=2 ** 20)],
                         ids=lambda d: "_".join(f"{k}={v}" for k, v in d.items()))
def test_img_prepare_rejects(bad):
    from projects.mmdet3d_plugin import native
    L = native.lib()
    rc = L.cmt_img_prepare(ctypes.byref(_prep_args(native, **bad)), None)
    assert rc == 1001, rc   # CMT_EINVAL
    assert b"cmt_img_prepare" in L.cmt_last_error()
    assert L.cmt_img_prepare(None, None) == 1001


# ---- host helpers -------------------------------------------------------------------------------------------------
def test_test_crop():
    from projects.mmdet3d_plugin import native_img as NI
    assert NI.test_crop((900, 1600), (640, 1600)) == (1.0, (0, 260, 1600, 900))
    assert NI.test_crop((188, 320), (128, 320)) == (1.0, (0, 60, 320, 188))
    with pytest.raises(NotImplementedError):
        NI.test_crop((900, 1600), (320, 800))


def test_crop_lidar2img():
    from projects.mmdet3d_plugin import native_img as NI
    from projects.mmdet3d_plugin import synthetic as S
    rng = np.random.default_rng(0)
    K = np.array([[1266.4, 0.0, 816.2], [0.0, 1266.4, 491.5], [0.0, 0.0, 1.0]])
    E = S.camera_lidar2img(20.0, f=1.0, cx=0.0, cy=0.0)   # unit intrinsics: the rigid lidar -> camera transform
    K4 = np.eye(4)
    K4[:3, :3] = K
    crop = (0, 260, 1600, 900)
    old, new = K4 @ E, NI.crop_lidar2img(K, E, crop)
    assert new.dtype == np.float64 and np.array_equal(NI.crop_lidar2img(K4, E, crop), new)
    assert K[1, 2] == 491.5   # the caller's matrix is not modified
    pts = np.concatenate([rng.uniform(5, 40, (50, 1)), rng.uniform(-5, 5, (50, 2)), np.ones((50, 1))], 1)
    pts = pts @ np.array([[np.cos(0.35), np.sin(0.35), 0, 0], [-np.sin(0.35), np.cos(0.35), 0, 0], [0, 0, 1, 0], [0, 0, 0, 1]])
    a, b = pts @ old.T, pts @ new.T
    keep = a[:, 2] > 1.0
    assert keep.sum() >= 10
    u0, v0 = a[keep, 0] / a[keep, 2], a[keep, 1] / a[keep, 2]
    u1, v1 = b[keep, 0] / b[keep, 2], b[keep, 1] / b[keep, 2]
    assert np.abs(u1 - (u0 - crop[0])).max() <= 1e-9 and np.abs(v1 - (v0 - crop[1])).max() <= 1e-9
    shifted = NI.crop_lidar2img(K, E, (7, 260, 1607, 900))
    c = pts @ shifted.T
    assert np.abs(c[keep, 0] / c[keep, 2] - (u0 - 7)).max() <= 1e-9


def test_norm_constants_two_step_error():
    """the float32 subtract-then-multiply form over every byte and channel of the configs' constants stays
    within 1.74e-7 of the float64 quotient: where the kernel test's 1e-6 bound comes from"""
    from projects.mmdet3d_plugin import native_img as NI
    mean32, inv32 = NI.norm_constants(NI.IMG_MEAN, NI.IMG_STD)
    assert mean32.dtype == np.float32 and inv32.dtype == np.float32
    x = np.arange(256, dtype=np.float32)[:, None]
    two = (x - mean32) * inv32
    ref = (x.astype(np.float64) - mean32.astype(np.float64)) / np.asarray(NI.IMG_STD, np.float32).astype(np.float64)
    assert two.dtype == np.float32 and np.abs(two - ref).max() <= 1.74e-7
    assert np.abs(ref).max() < 4.0   # largest |value| about 2.64: every result lies below 4, where one ulp is 2.4e-7


# ---- wrapper and detector errors ---------------------------------------------------------------------------------
def test_prepare_images_errors():
    from projects.mmdet3d_plugin import native_img as NI
    ok = torch.zeros((2, 8, 8, 3), dtype=torch.uint8)
    with pytest.raises(ValueError, match="uint8"):
        NI.prepare_images(ok.float())
    with pytest.raises(ValueError, match="contiguous"):
        NI.prepare_images(torch.zeros((2, 8, 3, 8), dtype=torch.uint8).permute(0, 1, 3, 2))
    with pytest.raises(ValueError, match="device"):
        NI.prepare_images(ok)
    with pytest.raises(ValueError):
        NI.prepare_images(torch.zeros((2, 8, 8, 4), dtype=torch.uint8))
    with pytest.raises(ValueError):
        NI.prepare_images(torch.zeros((8, 8, 3), dtype=torch.uint8))


def test_detector_argument_errors():
    from projects.mmdet3d_plugin import build_detector
    from projects.mmdet3d_plugin import synthetic as S
    model, cfg = _small("cmt_lidar_nus")
    model.eval()
    pts = torch.zeros((4, 5))
    with pytest.raises(TypeError, match="points must be a list"):
        model(return_loss=False, points=pts, img_metas=[[{}]])
    with pytest.raises(TypeError, match="img_metas must be a list"):
        model.forward_test(points=[[pts]], img_metas={})
    with pytest.raises(TypeError, match="img must be a list"):
        model.forward_test(points=[[pts]], img_metas=[[{}]], img=pts)
    with pytest.raises(NotImplementedError, match="inference only"):
        model.forward_train(points=[pts], img_metas=[{}])
    with pytest.raises(NotImplementedError, match="forward_train"):
        model(points=[pts], img_metas=[{}])   # return_loss defaults to True, as in mmdet
    coop_cfg = S.make_detector_cfg("cmtcoop_lidar_tumtraf", **SMALL)
    coop = build_detector(coop_cfg).eval()
    with pytest.raises(TypeError, match="vehicle_points must be a list"):
        coop.forward_test(vehicle_points=pts, img_metas=[[{}]])
    with pytest.raises(NotImplementedError):
        coop(return_loss=True, img_metas=[{}])
    with pytest.raises(NotImplementedError):
        build_detector(dict(coop_cfg, coop_fusion_neck=dict(type="Anything")))
    with pytest.raises(NotImplementedError):
        build_detector(dict(cfg, pts_fusion_layer=dict(type="Anything")))
    model.check_input_range()   # no forward ran: nothing to report
    coop.check_input_range()
