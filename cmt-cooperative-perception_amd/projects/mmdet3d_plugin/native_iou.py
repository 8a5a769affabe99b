"""Rotated-box overlap on the device: cmt_box_iou, cmt_box_nms and cmt_box_concat (include/cmt_hip.h).

``box_iou`` gives the pairwise (or row-by-row) BEV and 3D IoU of two box sets, ``nms_rotated`` the greedy rotated
NMS of one set, ``concat_detections`` the candidate set of late fusion: the boxes of several agents, each through
its own rigid transform, in one padded set.  Everything stays on the device: no call here reads a result back.

Like native_track.py: argument checks raise ValueError before the device check, tensors must live on a HIP device,
there is no CPU fallback.
"""
import ctypes
import math

import torch

from . import native as N
from ._argcheck import count_word as _count, nonneg, pose_arguments, same_device, strided_rows, tensor
from .native import _check, _p, _stream, lib

__all__ = ["NMS_MAX", "CONCAT_MAX", "box_iou", "nms_rotated", "nms_workspace", "concat_detections"]

NMS_MAX, CONCAT_MAX = N.NMS_MAX, N.CONCAT_MAX


def _z_origin(z):
    z = float(z)
    if z not in (0.0, 0.5):
        raise ValueError(f"z_origin must be 0 (z is the bottom) or 0.5 (z is the gravity centre), got {z}")
    return z


def _on_device(dev, **ts):
    same_device(dev, "the box overlap calls need tensors", **ts)


def box_iou(a, b, *, mode="bev", z_origin=0.5, aligned=False, n_a=None, n_b=None, out=None):
    """cmt_box_iou.  ``a`` fp32 [N, >= 7], ``b`` fp32 [M, >= 7] (x y z dx dy dz yaw; rows may be views with a row
    stride).  ``mode``: 'bev' or '3d' returns one fp32 [N, M] tensor, 'both' the pair (bev, iou3d); with
    ``aligned`` (N == M) the tensors are [N], row i against row i.  ``n_a`` / ``n_b``: None or device int32 counts
    of the valid rows; elements beyond them are not written (a fresh output is zero there).  ``out``: a tensor (or
    for 'both' a pair) to write into, [N, >= M] with unit column stride ([N] when aligned)."""
    if mode not in ("bev", "3d", "both"):
        raise ValueError(f"mode must be 'bev', '3d' or 'both', got {mode!r}")
    n, lda = strided_rows(a, "a", 7)
    m, ldb = strided_rows(b, "b", 7)
    z_origin = _z_origin(z_origin)
    if aligned and n != m:
        raise ValueError(f"aligned needs as many rows in a as in b, got {n} and {m}")
    _count(n_a, "n_a"), _count(n_b, "n_b")
    want = 2 if mode == "both" else 1
    if out is None:
        outs = [torch.zeros((n,) if aligned else (n, m), dtype=torch.float32, device=a.device) for _ in range(want)]
    else:
        outs = list(out) if isinstance(out, (tuple, list)) else [out]
        if len(outs) != want:
            raise ValueError(f"mode {mode!r} writes {want} tensor(s), out has {len(outs)}")
    ldo = m
    for k, o in enumerate(outs):
        if aligned:
            tensor(o, "out", torch.float32, (n,))
        else:
            rows, ld = strided_rows(o, "out", m, rows=n)
            if rows != n:
                raise ValueError(f"out must have {n} rows, got {rows}")
            if k and ld != ldo:
                raise ValueError("the two outputs must have the same row stride")
            ldo = ld
    _on_device(a.device, b=b, n_a=n_a, n_b=n_b, **{f"out{k}": o for k, o in enumerate(outs)})
    if n == 0 or m == 0:      # nothing to compute: empty tensors have no address to pass
        lib()
        return (outs[0], outs[1]) if want == 2 else outs[0]
    g = N.BoxIouArgs()
    g.N, g.M, g.lda, g.ldb, g.aligned, g.z_origin, g.ldo = n, m, lda, ldb, int(bool(aligned)), z_origin, max(ldo, m)
    g.a, g.b, g.n_a, g.n_b = _p(a), _p(b), _p(n_a), _p(n_b)
    if mode == "bev":
        g.bev = _p(outs[0])
    elif mode == "3d":
        g.iou3d = _p(outs[0])
    else:
        g.bev, g.iou3d = _p(outs[0]), _p(outs[1])
    _check(lib().cmt_box_iou(ctypes.byref(g), _stream()), "cmt_box_iou")
    return (outs[0], outs[1]) if want == 2 else outs[0]


def nms_workspace(n, device):
    """the workspace of ``nms_rotated`` for ``n`` rows: an int64 tensor (8-byte aligned), never initialised"""
    nbytes = int(lib().cmt_box_nms_workspace_bytes(int(n)))
    if nbytes < 0:
        raise ValueError(f"rotated NMS takes 0..{NMS_MAX} rows, got {n}")
    return torch.empty((nbytes + 7) // 8, dtype=torch.int64, device=device)


def nms_rotated(boxes, scores, iou_thr, *, labels=None, count=None, score_thr=-math.inf, z_origin=0.5, use_3d=False,
                work=None, keep=None):
    """cmt_box_nms -> (keep_idx int32 [N]: the kept rows in descending score, then -1; keep_count int32 [1]), both
    on the device.  ``labels`` int32 [N]: only rows of equal label suppress each other (class-aware).  ``count``:
    None or a device int32, the valid rows.  Rows below ``score_thr`` or with a NaN score do not take part.
    ``use_3d``: suppress by the 3D IoU instead of the BEV IoU.  ``work``: the tensor of ``nms_workspace(N, device)``
    (allocated when None).  ``keep``: an optional uint8 or int32 [N] tensor that receives the 0 / 1 flags."""
    n, ld = strided_rows(boxes, "boxes", 7)
    if n > NMS_MAX:
        raise ValueError(f"rotated NMS takes at most {NMS_MAX} rows, got {n}")
    scores = tensor(scores, "scores", torch.float32, (n,))
    if labels is not None:
        labels = tensor(labels, "labels", torch.int32, (n,))
    _count(count, "count")
    iou_thr, score_thr, z_origin = nonneg(iou_thr, "iou_thr"), float(score_thr), _z_origin(z_origin)
    if math.isnan(score_thr):
        raise ValueError("score_thr must not be NaN")
    if keep is not None:
        if not torch.is_tensor(keep) or keep.dtype not in (torch.uint8, torch.int32):
            raise ValueError("keep must be a uint8 or int32 tensor")
        tensor(keep, "keep", keep.dtype, (n,))
    dev = boxes.device
    _on_device(dev, scores=scores, labels=labels, count=count, work=work, keep=keep)
    need = int(lib().cmt_box_nms_workspace_bytes(n))
    if work is None:
        work = nms_workspace(n, dev)
    elif not torch.is_tensor(work) or not work.is_contiguous() or work.numel() * work.element_size() < need \
            or work.data_ptr() % 8:
        raise ValueError(f"work must be a contiguous, 8-byte aligned tensor of at least {need} bytes (nms_workspace)")
    keep_idx = torch.empty(n, dtype=torch.int32, device=dev)
    keep_count = torch.empty(1, dtype=torch.int32, device=dev)
    g = N.BoxNmsArgs()
    g.N, g.ld, g.use_3d, g.keep_dtype = n, ld, int(bool(use_3d)), int(keep is not None and keep.dtype == torch.int32)
    g.iou_thr, g.score_thr, g.z_origin = iou_thr, score_thr, z_origin
    g.boxes, g.scores, g.labels, g.count = _p(boxes), _p(scores), _p(labels), _p(count)
    g.keep_idx, g.keep, g.keep_count = _p(keep_idx), _p(keep), _p(keep_count)
    g.workspace, g.workspace_bytes = _p(work), work.numel() * work.element_size()
    _check(lib().cmt_box_nms(ctypes.byref(g), _stream()), "cmt_box_nms")
    return keep_idx, keep_count


def transform_arguments(pose):
    """A 4 x 4 (or 3 x 4) rigid transform -> its 12 floats, row-major [R|t]"""
    return pose_arguments(pose)[0]


def concat_detections(sources, poses=None, *, cols=None):
    """cmt_box_concat.  ``sources``: up to 8 tuples (boxes fp32 [n_k, >= 7], scores fp32 [n_k], labels int32 [n_k]
    [, count: None or a device int32]); ``poses``: None or per source None or a HOST 4 x 4 matrix that brings the
    source into the common frame (position, yaw and, from 9 columns on, the velocity go through it).  ``cols``:
    the columns carried (default: the fewest any source has, at most 16).
    -> (boxes [sum n_k, cols], scores, labels, source int32: the agent of every row, count int32 [1] = sum n_k).
    Row i of source k lands at [n_0 + .. + n_(k-1) + i]; rows beyond a source's count get score -inf and label -1,
    which ``nms_rotated`` drops through any finite ``score_thr``.  One launch, no host read."""
    sources = list(sources)
    K = len(sources)
    if not 1 <= K <= CONCAT_MAX:
        raise ValueError(f"concat_detections takes 1..{CONCAT_MAX} sources, got {K}")
    if poses is None:
        poses = [None] * K
    if len(poses) != K:
        raise ValueError(f"poses has {len(poses)} entries for {K} sources")
    g = N.BoxConcatArgs()
    keepalive, total, dev, width = [], 0, None, 16
    for k, src in enumerate(sources):
        if not isinstance(src, (tuple, list)) or len(src) not in (3, 4):
            raise ValueError(f"source {k} must be (boxes, scores, labels[, count])")
        boxes, scores, labels = src[:3]
        count = src[3] if len(src) == 4 else None
        n, ld = strided_rows(boxes, f"boxes of source {k}", 7)
        scores = tensor(scores, f"scores of source {k}", torch.float32, (n,))
        labels = tensor(labels, f"labels of source {k}", torch.int32, (n,))
        _count(count, f"count of source {k}")
        dev = boxes.device if dev is None else dev
        _on_device(dev, boxes=boxes, scores=scores, labels=labels, count=count)
        width = min(width, int(boxes.shape[1]))
        g.n[k], g.ld[k] = n, ld
        g.boxes[k], g.scores[k], g.labels[k] = boxes.data_ptr(), scores.data_ptr(), labels.data_ptr()
        g.count[k] = None if count is None else count.data_ptr()
        if poses[k] is not None:
            g.has_transform[k] = 1
            for t, v in enumerate(transform_arguments(poses[k])):
                g.transform[k][t] = v
        keepalive.append((boxes, scores, labels, count))
        total += n
    cols = width if cols is None else int(cols)
    if not 7 <= cols <= width:
        raise ValueError(f"cols must be 7..{width} (the narrowest source, at most 16), got {cols}")
    ob = torch.empty((total, cols), dtype=torch.float32, device=dev)
    os_ = torch.empty(total, dtype=torch.float32, device=dev)
    ol = torch.empty(total, dtype=torch.int32, device=dev)
    osrc = torch.empty(total, dtype=torch.int32, device=dev)
    oc = torch.empty(1, dtype=torch.int32, device=dev)
    g.K, g.cols, g.ld_out = K, cols, cols
    g.out_boxes, g.out_scores, g.out_labels, g.out_source, g.out_count = _p(ob), _p(os_), _p(ol), _p(osrc), _p(oc)
    _check(lib().cmt_box_concat(ctypes.byref(g), _stream()), "cmt_box_concat")
    return ob, os_, ol, osrc, oc
