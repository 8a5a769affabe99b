"""CmtCoopDetector: two headless CmtDetector agents (vehicle, infrastructure) and one cooperative head.

Restates, for inference, the reference's models/detectors/cmt_coop.py: each agent extracts its own image
and point features, and the CmtHeadCoop decodes both agents' memories and max-fuses them.  Both agents get
the frame's whole ``img_metas``; the head selects each agent's entries by key prefix (``vehicle_`` /
``infrastructure_``).  A missing agent or modality reaches the head as ``[None]`` (cmt_coop.py:552-561).
State-dict keys: ``vehicle_model.*``, ``infrastructure_model.*`` (each with CmtDetector's keys) and
``pts_bbox_head.*`` -- what ``merge_coop_checkpoints`` writes.  Training and ``aug_test`` are not built (see
cmt.py); ``show_results`` writes PNG pictures of both agents' clouds (core/visualizer).
"""
import copy

import torch.nn as nn

from ...registry import DETECTORS, build_head, build_model
from .cmt import (_TRAIN_MSG, _pts_cfg, bbox3d2result, check_children_range, check_test_lists, detector_forward)

__all__ = ["CmtCoopDetector"]


@DETECTORS.register_module()
class CmtCoopDetector(nn.Module):
    def __init__(self, vehicle_model=None, infrastructure_model=None, coop_fusion_neck=None, pts_bbox_head=None,
                 train_cfg=None, test_cfg=None, pretrained=None, init_cfg=None):
        super().__init__()
        if vehicle_model:
            self.vehicle_model = build_model(vehicle_model)
        if infrastructure_model:
            self.infrastructure_model = build_model(infrastructure_model)
        self.coop_fusion_neck = None
        if coop_fusion_neck:
            raise NotImplementedError("CmtCoopDetector coop_fusion_neck: not implemented in the reference either "
                                      "(cmt_coop.py:52-55); the agents are fused in the head")
        if pretrained is not None and not isinstance(pretrained, dict):
            raise ValueError(f"pretrained should be a dict, got {type(pretrained)}")
        if pts_bbox_head:
            head = copy.deepcopy(dict(pts_bbox_head))
            head.update(train_cfg=_pts_cfg(train_cfg), test_cfg=_pts_cfg(test_cfg))
            self.pts_bbox_head = build_head(head)
        self.train_cfg, self.test_cfg = train_cfg, test_cfg
        self.pretrained, self.init_cfg = pretrained, init_cfg

    def init_weights(self):
        for m in self.children():
            if hasattr(m, "init_weights"):
                m.init_weights()

    with_vehicle_model = property(lambda self: getattr(self, "vehicle_model", None) is not None)
    with_infrastructure_model = property(lambda self: getattr(self, "infrastructure_model", None) is not None)
    with_pts_bbox = property(lambda self: getattr(self, "pts_bbox_head", None) is not None)

    def extract_vehicular_feat(self, vehicle_points, vehicle_img, vehicle_img_metas):
        """-> (img_feats, pts_feats) of the vehicle agent ((None, None) without one)"""
        if not self.with_vehicle_model:
            return None, None
        return self.vehicle_model.extract_feat(points=vehicle_points, img=vehicle_img, img_metas=vehicle_img_metas)

    def extract_infrastructure_feat(self, infrastructure_points, infrastructure_img, infrastructure_img_metas):
        if not self.with_infrastructure_model:
            return None, None
        return self.infrastructure_model.extract_feat(points=infrastructure_points, img=infrastructure_img,
                                                      img_metas=infrastructure_img_metas)

    def coop_simple_test_pts(self, vehicle_pts_feats, infrastructure_pts_feats, vehicle_img_feats,
                             infrastructure_img_feats, img_metas, rescale=False):
        if vehicle_pts_feats is None:
            vehicle_pts_feats = [None]
        if infrastructure_pts_feats is None:
            infrastructure_pts_feats = [None]
        if vehicle_img_feats is None:
            vehicle_img_feats = [None]
        if infrastructure_img_feats is None:
            infrastructure_img_feats = [None]
        outs = self.pts_bbox_head(vehicle_pts_feats, infrastructure_pts_feats, vehicle_img_feats,
                                  infrastructure_img_feats, img_metas)
        bbox_list = self.pts_bbox_head.get_bboxes(outs, img_metas, rescale=rescale)
        return [bbox3d2result(b, s, l) for b, s, l in bbox_list]

    def simple_test(self, vehicle_points, infrastructure_points, img_metas, vehicle_img=None,
                    infrastructure_img=None, rescale=False):
        v_img, v_pts = self.extract_vehicular_feat(vehicle_points, vehicle_img, img_metas)
        i_img, i_pts = self.extract_infrastructure_feat(infrastructure_points, infrastructure_img, img_metas)
        bbox_list = [dict() for _ in range(len(img_metas))]
        if self.with_pts_bbox:
            bbox_pts = self.coop_simple_test_pts(v_pts, i_pts, v_img, i_img, img_metas, rescale=rescale)
            for result, pts_bbox in zip(bbox_list, bbox_pts):
                result["pts_bbox"] = pts_bbox
        return bbox_list

    def forward_test(self, vehicle_points=None, vehicle_img=None, infrastructure_points=None,
                     infrastructure_img=None, img_metas=None, **kwargs):
        """the outer lists are test-time augmentations; the first entry of each is run"""
        if vehicle_points is None:
            vehicle_points = [None]
        if infrastructure_points is None:
            infrastructure_points = [None]
        if vehicle_img is None:
            vehicle_img = [None]
        if infrastructure_img is None:
            infrastructure_img = [None]
        check_test_lists([(vehicle_points, "vehicle_points"), (vehicle_img, "vehicle_img"),
                          (infrastructure_points, "infrastructure_points"),
                          (infrastructure_img, "infrastructure_img"), (img_metas, "img_metas")])
        return self.simple_test(vehicle_points[0], infrastructure_points[0], img_metas[0],
                                vehicle_img=vehicle_img[0], infrastructure_img=infrastructure_img[0], **kwargs)

    def forward_train(self, *args, **kwargs):
        raise NotImplementedError(_TRAIN_MSG.format(type(self).__name__))

    def forward(self, return_loss=True, **kwargs):
        return detector_forward(self, return_loss, kwargs)

    def check_input_range(self):
        check_children_range(self)

    def show_results(self, data, result, out_dir, show=False, score_thr=None, gt_bboxes=None):
        """the reference's signature (cmt_coop.py:637); see core/visualizer.show_results for what is written"""
        from ...core.visualizer import show_results
        return show_results(self, data, result, out_dir, show=show, score_thr=score_thr, gt_bboxes=gt_bboxes)
