"""CmtDetector / CmtCoopDetector on the GPU at the head tests' small shapes: a 256 x 256 x 40 voxel grid
(32 x 32 BEV), frames prepared to 128 x 320, VoVNet V-19-eSE, 64 queries, 2 decoder layers, 2 000 points per
sample inside the shrunken range, jittered weights and BN statistics in every branch.

The detector is plumbing: it owns no parameter and no kernel.  So ``extract_feat`` must equal, bit for bit,
the modules called by hand in this process (voxelize_batch -> SparseEncoder -> SECOND -> SECONDFPN, and
VoVNet -> CPFPN), and ``simple_test`` must equal ``head(...)`` + ``get_bboxes`` on those features.  Every
module is bitwise repeatable, so equality is the bound; there is no tolerance here."""
import importlib.util
import json
import os

import pytest
import torch

from conftest import PKG

pytestmark = pytest.mark.gpu

SMALL = dict(num_query=64, num_layers=2, grid_size=[256, 256, 40], spec_name="V-19-eSE")
HW = (128, 320)
NPTS = 2000


def _image_only(cfg):
    for k in [k for k in cfg if k.startswith("pts_") and k != "pts_bbox_head"]:
        del cfg[k]
    cfg["pts_bbox_head"]["type"] = "CmtImageHead"


def _build(dev, name, modify=None, seed=0):
    from projects.mmdet3d_plugin import build_detector
    from projects.mmdet3d_plugin import synthetic as S
    cfg = S.make_detector_cfg(name, **SMALL)
    if modify is not None:
        modify(cfg)
    torch.manual_seed(seed)
    model = build_detector(cfg)
    model.init_weights()
    S._jitter_(model, torch.Generator().manual_seed(seed + 1))
    return model.eval().to(dev), cfg


def _points(dev, cfg, B, seed):
    from projects.mmdet3d_plugin import synthetic as S
    pcr = cfg["pts_voxel_layer"]["point_cloud_range"]
    return [S.synthetic_points(NPTS, pcr, seed=seed + i, device=dev) for i in range(B)]


def _images(dev, n, seed):
    from projects.mmdet3d_plugin import native_img as NI
    from projects.mmdet3d_plugin import synthetic as S
    img = NI.prepare_images(S.synthetic_frames(n, HW[0], HW[1], seed=seed, device=dev))
    assert tuple(img.shape) == (n, 3) + HW
    return img


def _metas(B, yaws, prefix="", seed=0):
    from projects.mmdet3d_plugin import synthetic as S
    return S.synthetic_metas(B, yaws=yaws, pad_shape=HW + (3,), prefix=prefix, seed=seed)


def _pts_by_hand(det, pts):
    from projects.mmdet3d_plugin.mmcv_custom.ops.voxel.spconv_voxelize import voxelize_batch
    feats, _, coors = voxelize_batch(det.pts_voxel_layer, pts, num_features=5)
    x = det.pts_middle_encoder(feats, coors, len(pts))
    return det.pts_neck(det.pts_backbone(x))


def _img_by_hand(det, img4):
    return det.img_neck(list(det.img_backbone(img4).values()))


def _same_maps(got, want):
    assert len(got) == len(want) and len(want) >= 1
    for g, w in zip(got, want):
        assert g.dtype == w.dtype and g.shape == w.shape and torch.equal(g, w)
        assert torch.isfinite(w).all() and float(w.abs().max()) > 0


def _same_results(results, bbox_list, B):
    assert isinstance(results, list) and len(results) == B == len(bbox_list)
    for res, (boxes, scores, labels) in zip(results, bbox_list):
        assert list(res) == ["pts_bbox"] and sorted(res["pts_bbox"]) == ["boxes_3d", "labels_3d", "scores_3d"]
        r = res["pts_bbox"]
        for t in r.values():
            assert torch.is_tensor(t) and t.device.type == "cpu"
        assert r["boxes_3d"].shape[0] == r["scores_3d"].shape[0] == r["labels_3d"].shape[0] > 0
        assert r["boxes_3d"].shape[1] == 9
        assert torch.equal(r["boxes_3d"], boxes.cpu()) and torch.equal(r["scores_3d"], scores.cpu())
        assert torch.equal(r["labels_3d"], labels.cpu())


def test_fusion_detector(dev):
    from projects.mmdet3d_plugin import synthetic as S
    from projects.mmdet3d_plugin.models.detectors import CmtDetector
    B, V = 2, 2
    det, cfg = _build(dev, "cmt_fusion_nus")
    assert type(det) is CmtDetector
    pts, img4 = _points(dev, cfg, B, 10), _images(dev, B * V, 20)
    metas = _metas(B, S.NUS_YAWS[:V], seed=30)
    with torch.no_grad():
        want_pts, want_img = _pts_by_hand(det, pts), _img_by_hand(det, img4)
        img_feats, pts_feats = det.extract_feat(pts, img4, metas)
        _same_maps(pts_feats, want_pts)
        _same_maps(img_feats, want_img)
        assert tuple(pts_feats[0].shape) == (B, 512, 32, 32) and tuple(img_feats[0].shape) == (B * V, 256, 8, 20)
        assert all(tuple(m["input_shape"]) == HW for m in metas)
        want = det.pts_bbox_head.get_bboxes(det.pts_bbox_head(want_pts, want_img, metas), metas)
        res4 = det.simple_test(pts, metas, img=img4)
        _same_results(res4, want, B)
        # the image as the data pipeline collates it: [B, N, 3, H, W]
        metas5 = _metas(B, S.NUS_YAWS[:V], seed=30)
        res5 = det.simple_test(pts, metas5, img=img4.view(B, V, 3, *HW))
        _same_results(res5, want, B)
        assert all(tuple(m["input_shape"]) == HW for m in metas5)
        # mmdet's entry: the outer lists are test-time augmentations
        res = det(return_loss=False, points=[pts], img_metas=[metas], img=[img4.view(B, V, 3, *HW)])
        _same_results(res, want, B)
    det.check_input_range()


def test_coop_detector(dev):
    from projects.mmdet3d_plugin import synthetic as S
    from projects.mmdet3d_plugin.models.detectors import CmtCoopDetector
    B = 1
    det, cfg = _build(dev, "cmtcoop_fusion_tumtraf")
    assert type(det) is CmtCoopDetector
    body = cfg["vehicle_model"]
    pv, pi = _points(dev, body, B, 40), _points(dev, body, B, 50)
    iv, ii = _images(dev, 1, 60), _images(dev, 3, 70)
    metas = _metas(B, S.VEHICLE_YAWS, prefix="vehicle_", seed=80)
    metas[0].update(_metas(B, S.INFRA_YAWS, prefix="infrastructure_", seed=90)[0])
    head = det.pts_bbox_head
    with torch.no_grad():
        wv_pts, wv_img = _pts_by_hand(det.vehicle_model, pv), _img_by_hand(det.vehicle_model, iv)
        wi_pts, wi_img = _pts_by_hand(det.infrastructure_model, pi), _img_by_hand(det.infrastructure_model, ii)
        gv_img, gv_pts = det.extract_vehicular_feat(pv, iv[None], metas)
        gi_img, gi_pts = det.extract_infrastructure_feat(pi, ii[None], metas)
        _same_maps(gv_pts, wv_pts)
        _same_maps(gv_img, wv_img)
        _same_maps(gi_pts, wi_pts)
        _same_maps(gi_img, wi_img)
        assert not torch.equal(wv_pts[0], wi_pts[0])   # the agents carry their own weights and inputs
        assert tuple(metas[0]["input_shape"]) == HW
        want = head.get_bboxes(head(wv_pts, wi_pts, wv_img, wi_img, metas), metas)
        res = det.simple_test(pv, pi, metas, vehicle_img=iv[None], infrastructure_img=ii[None])
        _same_results(res, want, B)
        res = det(return_loss=False, vehicle_points=[pv], vehicle_img=[iv[None]], infrastructure_points=[pi],
                  infrastructure_img=[ii[None]], img_metas=[metas])
        _same_results(res, want, B)
        # the vehicle agent absent: its features reach the head as [None]
        want_i = head.get_bboxes(head([None], wi_pts, [None], wi_img, metas), metas)
        res_i = det.simple_test(None, pi, metas, vehicle_img=None, infrastructure_img=ii[None])
        _same_results(res_i, want_i, B)
        assert not torch.equal(res_i[0]["pts_bbox"]["scores_3d"], res[0]["pts_bbox"]["scores_3d"])
    det.check_input_range()


def test_lidar_detector(dev):
    B = 2
    det, cfg = _build(dev, "cmt_lidar_nus")
    assert not det.with_img_backbone
    pts = _points(dev, cfg, B, 100)
    metas = [dict() for _ in range(B)]
    with torch.no_grad():
        want_pts = _pts_by_hand(det, pts)
        img_feats, pts_feats = det.extract_feat(pts, None, metas)
        assert img_feats is None
        _same_maps(pts_feats, want_pts)
        assert not torch.equal(want_pts[0][0], want_pts[0][1])
        want = det.pts_bbox_head.get_bboxes(det.pts_bbox_head(want_pts, [None], metas), metas)
        _same_results(det.simple_test(pts, metas), want, B)
        _same_results(det(return_loss=False, points=[pts], img_metas=[metas]), want, B)
    det.check_input_range()


def test_camera_detector(dev):
    from projects.mmdet3d_plugin import synthetic as S
    B, V = 1, 2
    det, cfg = _build(dev, "cmt_fusion_nus", modify=_image_only)
    assert type(det.pts_bbox_head).__name__ == "CmtImageHead" and not det.with_pts_backbone
    assert not any(k.startswith("pts_") and not k.startswith("pts_bbox_head.") for k in det.state_dict())
    img4 = _images(dev, B * V, 110)
    metas = _metas(B, S.NUS_YAWS[:V], seed=120)
    with torch.no_grad():
        want_img = _img_by_hand(det, img4)
        img_feats, pts_feats = det.extract_feat(None, img4[None], metas)
        assert pts_feats is None
        _same_maps(img_feats, want_img)
        want = det.pts_bbox_head.get_bboxes(det.pts_bbox_head([None], want_img, metas), metas)
        _same_results(det.simple_test(None, metas, img=img4[None]), want, B)
    det.check_input_range()


def test_cli_detector(dev, tmp_path):
    """tools/test.py --detector in this process: uint8 frames 188 x 320 are cropped to rows 60..188"""
    from projects.mmdet3d_plugin import native_img as NI
    assert NI.test_crop((188, 320), (128, 320)) == (1.0, (0, 60, 320, 188))
    spec = importlib.util.spec_from_file_location("cmt_test_cli_det", os.path.join(PKG, "tools", "test.py"))
    cli = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(cli)
    out = tmp_path / "f.json"
    rc = cli.main(["cmt_fusion_nus", "--synthetic", "--detector", "--num-query", "32", "--num-layers", "1",
                   "--grid", "32", "32", "--frame-size", "188", "320", "--points", "1000", "--out", str(out)])
    assert rc == 0
    data = json.loads(out.read_text())
    assert data["config"] == "cmt_fusion_nus" and len(data["frames"]) == 1
    fr = data["frames"][0]
    n = len(fr["scores_3d"])
    assert n > 0 and len(fr["boxes_3d"]) == n == len(fr["labels_3d"]) and len(fr["boxes_3d"][0]) == 9
    assert fr["voxels"][0]["voxels"] > 0 and fr["voxels"][0]["points_kept"] == 1000
