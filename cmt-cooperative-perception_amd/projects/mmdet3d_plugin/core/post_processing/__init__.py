"""Box-level post-processing on the device: late fusion of several agents' detections and the NMS settings of a
``test_cfg``.

``fuse_detections`` is the box-level baseline of cooperative perception: every agent's detector runs on its own,
the box sets are brought into one frame and duplicates are suppressed by rotated IoU, the higher-scoring box of a
duplicate staying as it is (no merging).  The body is cmt_box_concat -> cmt_box_nms -> one gather; nothing is read
back, the outputs are padded to capacity and carry a device count.
"""
import math

import torch

__all__ = ["fuse_detections", "nms_from_test_cfg"]


def fuse_detections(results, *, iou_thr, poses=None, class_aware=True, score_thr=None, max_num=None, z_origin=0.5):
    """``results``: per agent (boxes fp32 [n_k, >= 7], scores fp32 [n_k], labels int32 [n_k][, count]) on one HIP
    device, as ``cmt_box_decode`` or ``get_bboxes`` give them (``z_origin`` 0.5 for the former's gravity-centre z,
    0 for the latter's bottom z); ``poses[k]``: None or a host 4 x 4 matrix that brings agent k into the common
    frame.  ``class_aware``: only boxes of one class suppress each other.  ``score_thr``: boxes below it take no
    part (None: every real box).  ``max_num``: at most that many boxes, the best first.
    -> (boxes [cap, cols], scores [cap], labels int32 [cap], source int32 [cap], count int32 [1]): the fused boxes
    in descending score in the first ``count`` rows (then zeros, score -inf, label -1, source -1), ``source`` the
    agent a box came from; cap = sum n_k, or ``max_num`` if that is smaller."""
    from ... import native_iou as NI
    boxes, scores, labels, source, _ = NI.concat_detections(results, poses)
    # the padding rows of the candidate set carry score -inf: any finite threshold drops them
    thr = -torch.finfo(torch.float32).max if score_thr is None else float(score_thr)
    if math.isnan(thr) or thr == -math.inf:
        raise ValueError("score_thr must be finite (the padding rows carry -inf) or None")
    keep_idx, count = NI.nms_rotated(boxes, scores, iou_thr, labels=labels if class_aware else None, score_thr=thr,
                                     z_origin=z_origin)
    if max_num is not None:
        if int(max_num) < 0:
            raise ValueError(f"max_num must not be negative, got {max_num}")
        keep_idx = keep_idx[:int(max_num)]
        count = count.clamp(max=int(max_num))
    kept = keep_idx >= 0
    idx = keep_idx.clamp(min=0).long()
    ob = torch.where(kept[:, None], boxes.index_select(0, idx), boxes.new_zeros(()))
    os_ = torch.where(kept, scores.index_select(0, idx), scores.new_full((), -math.inf))
    ol = torch.where(kept, labels.index_select(0, idx), labels.new_full((), -1))
    osrc = torch.where(kept, source.index_select(0, idx), source.new_full((), -1))
    return ob, os_, ol, osrc, count


def nms_from_test_cfg(test_cfg):
    """The rotated-NMS settings of a head's ``test_cfg`` (or a model's, with its ``pts`` entry): None for
    ``nms_type`` None or 'circle' (circle NMS is not implemented), for 'rotate' dict(iou_thr = nms_thr,
    use_rotate_nms)."""
    if isinstance(test_cfg, dict) and "pts" in test_cfg and "nms_type" not in test_cfg:
        test_cfg = test_cfg["pts"]
    if not isinstance(test_cfg, dict):
        raise ValueError("test_cfg must be a dict")
    kind = test_cfg.get("nms_type")
    if kind in (None, "circle"):
        return None
    if kind != "rotate":
        raise ValueError(f"unknown nms_type {kind!r} (None, 'circle' or 'rotate')")
    if "nms_thr" not in test_cfg:
        raise ValueError("nms_type 'rotate' needs nms_thr")
    return dict(iou_thr=float(test_cfg["nms_thr"]), use_rotate_nms=bool(test_cfg.get("use_rotate_nms", True)))
