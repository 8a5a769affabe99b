"""CmtDetector: raw points and prepared images to boxes through the native stages.

Restates, for inference, the reference's models/detectors/cmt.py (CmtDetector over mmdet3d's
MVXTwoStageDetector): voxelize + HardSimpleVFE -> SparseEncoder -> SECOND -> SECONDFPN for the points,
VoVNet -> CPFPN for the images, then the CMT head and its box decode.  The detector itself is plumbing:
it owns no parameter and launches no kernel of its own, so its outputs equal, bit for bit, the modules
called by hand.  Differences from the reference, all of scope:

* the feature extractors are inference only (their modules raise in training mode with autograd on), so
  ``forward_train`` raises; the head trains through its own ``forward_train`` / ``Trainer``;
* GridMask is the identity outside training (grid_mask.py:86), so ``use_grid_mask`` is accepted and no
  GridMask is built;
* with a ``HardSimpleVFE`` encoder the per-voxel mean comes out of the voxelizer's own kernel
  (``voxelize_batch``); any other encoder module is called on the padded voxels;
* the batch size handed to the middle encoder is ``len(points)``, not ``coors[-1, 0] + 1`` (cmt.py:81): the
  same number unless the last sample has no voxel, and no host read;
* a cloud may be the padded buffer of ``native_pts.prepare_points`` (kept rows first, NaN rows after them) as it
  is: the voxelizer drops non-finite points and keeps input order, so the result equals the trimmed cloud's bit
  for bit and the count never has to reach the host;
* ``show_results`` writes PNG pictures drawn on the device (core/visualizer: the top view, and camera overlays when
  the data carries uint8 frames), not mmdet3d's ``.obj`` files, and ``show=True`` raises (there is no display);
* ``aug_test`` is not built.

State-dict keys are the reference's: ``img_backbone.*``, ``img_neck.*``, ``pts_middle_encoder.*``,
``pts_backbone.*``, ``pts_neck.*``, ``pts_bbox_head.*``; the voxel layer, the VFE and the detector add none.
"""
import copy

import torch
import torch.nn as nn

from ...mmcv_custom.ops.voxel.spconv_voxelize import SPConvVoxelization, voxelize_batch
from ...registry import (DETECTORS, build_backbone, build_head, build_middle_encoder, build_neck,
                         build_voxel_encoder)
from ..voxel_encoders import HardSimpleVFE

__all__ = ["CmtDetector", "bbox3d2result", "detector_forward", "check_test_lists"]

_TRAIN_MSG = ("{}: the feature extractors (voxelizer, SparseEncoder, SECOND, SECONDFPN, VoVNet, CPFPN) are inference "
              "only, so the detector does not train end to end; the head trains through its own forward_train / "
              "Trainer on precomputed features, as before")


def bbox3d2result(bboxes, scores, labels):
    """mmdet3d.core.bbox3d2result: one sample's boxes, scores and labels as CPU tensors"""
    return dict(boxes_3d=bboxes.to("cpu"), scores_3d=scores.cpu(), labels_3d=labels.cpu())


def detector_forward(model, return_loss, kwargs):
    """mmdet's BaseDetector.forward dispatch"""
    if return_loss:
        return model.forward_train(**kwargs)
    return model.forward_test(**kwargs)


def check_test_lists(pairs):
    """forward_test's argument check: every entry is the outer test-time-augmentation list"""
    for var, name in pairs:
        if not isinstance(var, list):
            raise TypeError("{} must be a list, but got {}".format(name, type(var)))


def _pts_cfg(cfg):
    if not cfg:
        return None
    return cfg["pts"] if isinstance(cfg, dict) else cfg.pts


def check_children_range(model):
    """check_input_range() of every direct sub-module that has one (the RangeFlagMixin extractors, the head,
    an agent detector); every flag is read and cleared before the first error is raised"""
    first = None
    for m in model.children():
        fn = getattr(m, "check_input_range", None)
        if fn is None:
            continue
        try:
            fn()
        except ValueError as e:
            first = first or e
    if first is not None:
        raise first


@DETECTORS.register_module()
class CmtDetector(nn.Module):
    def __init__(self, use_grid_mask=False, pts_voxel_layer=None, pts_voxel_encoder=None, pts_middle_encoder=None,
                 pts_backbone=None, pts_neck=None, img_backbone=None, img_neck=None, pts_bbox_head=None,
                 train_cfg=None, test_cfg=None, pretrained=None, init_cfg=None, **kwargs):
        super().__init__()
        extra = sorted(k for k, v in kwargs.items() if v is not None)
        if extra:
            raise NotImplementedError(f"CmtDetector: {extra} of MVXTwoStageDetector have no native path (no reference "
                                      "config sets them)")
        if img_backbone and img_backbone.get("type") == "ResNet":
            raise NotImplementedError("CmtDetector img_backbone type 'ResNet' (the r50 800 x 320 config) is not built: "
                                      "the native image backbone is VoVNet")
        self.use_grid_mask = bool(use_grid_mask)
        if pts_voxel_layer:
            self.pts_voxel_layer = SPConvVoxelization(**pts_voxel_layer)
        if pts_voxel_encoder:
            self.pts_voxel_encoder = build_voxel_encoder(pts_voxel_encoder)
        if pts_middle_encoder:
            self.pts_middle_encoder = build_middle_encoder(pts_middle_encoder)
        if pts_backbone:
            self.pts_backbone = build_backbone(pts_backbone)
        if pts_neck is not None:
            self.pts_neck = build_neck(pts_neck)
        if img_backbone:
            self.img_backbone = build_backbone(img_backbone)
        if img_neck is not None:
            self.img_neck = build_neck(img_neck)
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

    # ---- what is there -----------------------------------------------------------------------------------
    def _has(self, name):
        return getattr(self, name, None) is not None

    with_img_backbone = property(lambda self: self._has("img_backbone"))
    with_img_neck = property(lambda self: self._has("img_neck"))
    with_pts_backbone = property(lambda self: self._has("pts_backbone"))
    with_pts_neck = property(lambda self: self._has("pts_neck"))
    with_voxel_encoder = property(lambda self: self._has("pts_voxel_encoder"))
    with_middle_encoder = property(lambda self: self._has("pts_middle_encoder"))
    with_pts_bbox = property(lambda self: self._has("pts_bbox_head"))

    # ---- features ----------------------------------------------------------------------------------------
    def extract_img_feat(self, img, img_metas):
        """img [B, N, C, H, W] or [B*N, C, H, W] -> the neck's tuple of maps (None without image or backbone)"""
        if not self.with_img_backbone or img is None:
            return None
        input_shape = img.shape[-2:]
        for m in img_metas:
            m.update(input_shape=input_shape)
        if img.dim() == 5 and img.size(0) == 1:
            img = img.squeeze(0)
        elif img.dim() == 5 and img.size(0) > 1:
            B, N, C, H, W = img.size()
            img = img.view(B * N, C, H, W)
        feats = self.img_backbone(img.float())
        if isinstance(feats, dict):
            feats = list(feats.values())
        if self.with_img_neck:
            feats = self.img_neck(feats)
        return feats

    @torch.no_grad()
    def voxelize(self, points):
        """list of [N_i, F] clouds -> (features, num_points [M], coors [M, 4] = (sample, z, y, x)).  With a
        HardSimpleVFE encoder ``features`` is already its output, the per-voxel mean [M, num_features] of the
        voxelizer's kernel; otherwise the padded voxels [M, max_points, F] for the encoder module."""
        if not self._has("pts_voxel_layer"):
            raise RuntimeError("CmtDetector has no pts_voxel_layer")
        enc = getattr(self, "pts_voxel_encoder", None)
        if isinstance(enc, HardSimpleVFE):
            return voxelize_batch(self.pts_voxel_layer, points, num_features=enc.num_features)
        voxels, nums, coors = [], [], []
        for i, pts in enumerate(points):
            v, c, n = self.pts_voxel_layer(pts)
            voxels.append(v)
            nums.append(n)
            coors.append(nn.functional.pad(c, (1, 0), mode="constant", value=i))
        return torch.cat(voxels, 0), torch.cat(nums, 0), torch.cat(coors, 0)

    def extract_pts_feat(self, pts, img_feats, img_metas):
        """list of clouds -> the neck's ``[bev]`` (None without points)"""
        if pts is None:
            return None
        if not (self.with_voxel_encoder and self.with_middle_encoder and self.with_pts_backbone):
            raise RuntimeError("CmtDetector got points but has no point branch (pts_voxel_encoder, pts_middle_encoder "
                               "and pts_backbone)")
        feats, nums, coors = self.voxelize(pts)
        if not isinstance(self.pts_voxel_encoder, HardSimpleVFE):
            feats = self.pts_voxel_encoder(feats, nums, coors)
        x = self.pts_middle_encoder(feats, coors, len(pts))
        x = self.pts_backbone(x)
        if self.with_pts_neck:
            x = self.pts_neck(x)
        return x

    def extract_feat(self, points, img, img_metas):
        img_feats = self.extract_img_feat(img, img_metas)
        pts_feats = self.extract_pts_feat(points, img_feats, img_metas)
        return img_feats, pts_feats

    # ---- test --------------------------------------------------------------------------------------------
    def simple_test_pts(self, x, x_img, img_metas, rescale=False):
        outs = self.pts_bbox_head(x, x_img, img_metas)
        bbox_list = self.pts_bbox_head.get_bboxes(outs, img_metas, rescale=rescale)
        return [bbox3d2result(b, s, l) for b, s, l in bbox_list]

    def simple_test(self, points, img_metas, img=None, rescale=False):
        img_feats, pts_feats = self.extract_feat(points, img=img, img_metas=img_metas)
        if pts_feats is None:
            pts_feats = [None]
        if img_feats is None:
            img_feats = [None]
        bbox_list = [dict() for _ in range(len(img_metas))]
        if self.with_pts_bbox:
            for result, pts_bbox in zip(bbox_list, self.simple_test_pts(pts_feats, img_feats, img_metas, rescale)):
                result["pts_bbox"] = pts_bbox
        return bbox_list

    def forward_test(self, points=None, img_metas=None, img=None, **kwargs):
        """the outer lists are test-time augmentations; the first entry of each is run"""
        if points is None:
            points = [None]
        if img is None:
            img = [None]
        check_test_lists([(points, "points"), (img, "img"), (img_metas, "img_metas")])
        return self.simple_test(points[0], img_metas[0], img[0], **kwargs)

    def forward_train(self, *args, **kwargs):
        raise NotImplementedError(_TRAIN_MSG.format(type(self).__name__))

    def forward(self, return_loss=True, **kwargs):
        return detector_forward(self, return_loss, kwargs)

    def check_input_range(self):
        check_children_range(self)

    def show_results(self, data, result, out_dir, show=False, score_thr=None):
        """the reference's signature (coop_base.py:31); see core/visualizer.show_results for what is written"""
        from ...core.visualizer import show_results
        return show_results(self, data, result, out_dir, show=show, score_thr=score_thr)
