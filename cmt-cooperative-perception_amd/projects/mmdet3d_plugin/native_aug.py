"""The training side of the point pipeline on the device: cmt_points_in_boxes, cmt_pts_augment and
cmt_boxes_augment (include/cmt_hip.h) and the host helpers that restate the reference's choices around them.

``augment_points`` takes one cloud (the padded pair ``prepare_points`` returns, or plain rows), the objects a
database sampler chose (their points and boxes) and the parameters one sample drew, and returns the detector's
training ``points``: remove_points_in_boxes, the concatenation, GlobalRotScaleTransAll[Coop], CustomRandomFlip3D,
PointsRangeFilter[Coop] and PointShuffle[Coop] in two launches with no host read.  The result is padded like
``prepare_points``': kept rows first, the rest NaN, plus a device count, and goes to ``voxelize_batch`` as it is.
``augment_boxes`` applies the same parameters to the annotations (with ObjectRangeFilter, ObjectNameFilter and
limit_yaw) and can write the head's gravity-centre layout for ``head.forward_train``.  ``points_in_boxes`` is the
inside test on its own; it gives the evaluator its ``gt_num_pts``.

The database sampler (the in-memory database, its collision test and the gather of the chosen objects) is
native_gtdb.py; its files stay with the caller.  ``unified_sample``'s image pasting and the image side of the
training pipeline are native_imgaug.py.

Like native_pts.py: argument checks raise ValueError before the device check, tensors must live on a HIP device,
there is no CPU fallback and no wrapper synchronises with the host.
"""
import ctypes
import math

import numpy as np
import torch

from . import native as N
from ._argcheck import count_word as _count_word, rows as _rows, same_device, tensor
from .native import _check, _p, _stream, lib
from .native_pts import PointsWorkspace, _pipeline_steps

__all__ = ["MAX_PASTE_BOXES", "MAX_ANNOTATIONS", "tile_rows", "box_chunk", "workspace_bytes", "points_in_boxes",
           "augment_points", "augment_boxes", "sample_augmentation", "augment_lidar2img", "train_plan_from_config"]

MAX_PASTE_BOXES = N.AUG_MAX_BOXES
MAX_ANNOTATIONS = N.AUG_MAX_ANN
_PARAM_KEYS = {"angle", "scale", "trans", "flip_h", "flip_v"}
_DEFAULT_WS = PointsWorkspace()


def tile_rows():
    """slots (points) per workgroup tile of cmt_pts_augment and cmt_points_in_boxes"""
    return int(lib().cmt_pts_augment_tile_rows())


def box_chunk():
    """boxes staged per pass of cmt_points_in_boxes"""
    return int(lib().cmt_points_in_boxes_chunk())


def workspace_bytes(n_in):
    return int(lib().cmt_pts_augment_workspace_bytes(int(n_in)))


def rotation_matrix(angle):
    """R of BasePoints.rotate(angle): counter-clockwise about z, p' = R p; float64"""
    c, s = math.cos(float(angle)), math.sin(float(angle))
    return np.array([[c, -s, 0.0], [s, c, 0.0], [0.0, 0.0, 1.0]])


def _fill_xform(xf, params, point_cloud_range):
    """the checked parameters of one sample -> cmt_aug_xform.  A step is switched on iff its parameter is present
    (not None): angle 0, scale 1 and a zero translation still multiply and add, as the reference does."""
    if not isinstance(params, dict):
        raise ValueError(f"params must be a dict with keys among {sorted(_PARAM_KEYS)}, got {type(params)}")
    unknown = set(params) - _PARAM_KEYS
    if unknown:
        raise ValueError(f"params: unknown keys {sorted(unknown)}")
    angle, scale, trans = params.get("angle"), params.get("scale"), params.get("trans")
    if angle is not None:
        a = float(angle)
        if not math.isfinite(a):
            raise ValueError(f"params['angle'] must be finite, got {angle!r}")
        xf.has_rot = 1
        xf.rot32[:] = rotation_matrix(a).astype(np.float32).ravel().tolist()
        xf.angle32 = a
    if scale is not None:
        s = float(np.float32(scale))
        if not math.isfinite(s):
            raise ValueError(f"params['scale'] must be finite, got {scale!r}")
        xf.has_scale, xf.scale = 1, s
    if trans is not None:
        t = np.asarray(trans, dtype=np.float32).reshape(-1)
        if t.shape != (3,) or not np.isfinite(t).all():
            raise ValueError(f"params['trans'] must be 3 finite values, got {trans!r}")
        xf.has_trans = 1
        xf.trans32[:] = t.tolist()
    xf.flip_h, xf.flip_v = int(bool(params.get("flip_h"))), int(bool(params.get("flip_v")))
    if point_cloud_range is not None:
        rng = np.asarray(point_cloud_range, dtype=np.float32).reshape(-1)
        if rng.shape != (6,) or not np.isfinite(rng).all() or not (rng[:3] < rng[3:]).all():
            raise ValueError(f"point_cloud_range must be 6 finite values with min < max, got {point_cloud_range!r}")
        xf.has_range = 1
        xf.range[:] = rng.tolist()


def _on_device(dev, **tensors):
    same_device(dev, "tensors must live", **tensors)


def points_in_boxes(points, boxes, count=None, want=("box_of_point", "count_per_box")):
    """cmt_points_in_boxes -> the tensors named in ``want``, in its order (one name: that tensor alone).

    ``points``: fp32 [N, F], F 3..8 (columns 0..2 are read); ``count``: None or a device int32, rows at or beyond it
    belong to no box (the padded pair of ``prepare_points`` / ``augment_points``); ``boxes``: fp32 [M, 7 | 9] LiDAR
    boxes (x, y, z_bottom, dx, dy, dz, yaw, ...).  ``box_of_point`` int32 [N]: the lowest index of a containing box,
    -1 for none; ``count_per_box`` int32 [M]: the points inside each box (``points_in_rbbox(...).sum(0)``), which is
    the evaluator's ``gt_num_pts``.  No host read."""
    single = isinstance(want, str)
    names = (want,) if single else tuple(want)
    if not names or any(n not in ("box_of_point", "count_per_box") for n in names) or len(set(names)) != len(names):
        raise ValueError(f"want must name box_of_point and / or count_per_box, got {want!r}")
    points = _rows(points, "points", range(3, 9))
    boxes = _rows(boxes, "boxes", (7, 9))
    count = _count_word(count)
    n, m = int(points.shape[0]), int(boxes.shape[0])
    if n >= 2 ** 31 or m >= 2 ** 24:
        raise ValueError("at most 2^31 - 1 points and 2^24 - 1 boxes")
    dev = points.device
    _on_device(dev, boxes=boxes, count=count)
    out = {}
    if "box_of_point" in names:
        out["box_of_point"] = torch.empty(n, dtype=torch.int32, device=dev)
    if "count_per_box" in names:
        out["count_per_box"] = torch.empty(m, dtype=torch.int32, device=dev)
    a = N.PointsInBoxesArgs()
    a.N, a.M, a.F, a.D = n, m, int(points.shape[1]), int(boxes.shape[1])
    a.points, a.count_in, a.boxes = _p(points), _p(count), _p(boxes)
    a.box_of_point, a.count_per_box = _p(out.get("box_of_point")), _p(out.get("count_per_box"))
    _check(lib().cmt_points_in_boxes(ctypes.byref(a), _stream()), "cmt_points_in_boxes")
    return out[names[0]] if single else tuple(out[k] for k in names)


def augment_points(points, params, *, count=None, paste_points=None, paste_boxes=None, paste_first=False,
                   point_cloud_range=None, shuffle=None, out=None, workspace=None):
    """cmt_pts_augment for one cloud -> (points_padded [n_in, F] fp32, count [1] int32), both on the device, with
    n_in = len(points) + len(paste_points): rows [0, count) are the augmented cloud, rows [count, n_in) NaN.

    ``points``: fp32 [n, F], F 3..8, with the optional device ``count`` (rows at or beyond it are dropped).
    ``params``: dict with any of ``angle`` (radians, counter-clockwise), ``scale``, ``trans`` (3 values), ``flip_h``,
    ``flip_v`` as ``sample_augmentation`` draws them; an absent or None entry switches its step off.  The coop
    sample calls this twice with the same ``params``.
    ``paste_points`` fp32 [n_paste, F] / ``paste_boxes`` fp32 [K, 7 | 9] (columns 0..6 are used), K <= 128: the
    sampled objects.  Rows of ``points`` inside a paste box are removed; the paste rows are concatenated in front
    (``paste_first``: ObjectSample[Coop]) or behind (UnifiedObjectSample[Coop]).
    ``point_cloud_range``: None or the 6 values of PointsRangeFilter[Coop], applied after the transform.
    ``shuffle``: None (keep the order), True or a torch.Generator (PointShuffle: a random permutation of all n_in
    rows drawn on the device; restricted to the kept rows it is a uniform shuffle of them), or an int32 [n_in]
    order tensor (slot j visits row order[j] of the concatenation; an entry outside [0, n_in) drops the slot).
    ``out`` / ``workspace``: as ``prepare_points``."""
    points = _rows(points, "points", range(3, 9))
    F, n_src = int(points.shape[1]), int(points.shape[0])
    count = _count_word(count)
    if (paste_points is None) != (paste_boxes is None):
        raise ValueError("paste_points and paste_boxes come together")
    n_paste = K = 0
    if paste_points is not None:
        paste_points = _rows(paste_points, "paste_points", (F,))
        paste_boxes = _rows(paste_boxes, "paste_boxes", (7, 9))
        n_paste, K = int(paste_points.shape[0]), int(paste_boxes.shape[0])
        if K > MAX_PASTE_BOXES:
            raise ValueError(f"at most {MAX_PASTE_BOXES} paste boxes, got {K}")
    n_in = n_src + n_paste
    if n_in >= 2 ** 31:
        raise ValueError("n_in must be below 2^31")
    a = N.PtsAugmentArgs()
    _fill_xform(a.xf, params, point_cloud_range)
    order = None
    if torch.is_tensor(shuffle):
        order = tensor(shuffle, "an order tensor", torch.int32, (n_in,))
    elif not (shuffle is None or isinstance(shuffle, (bool, torch.Generator))):
        raise ValueError(f"shuffle must be None, a bool, a torch.Generator or an int32 order tensor, got {type(shuffle)}")
    dev = points.device
    _on_device(dev, count=count, paste_points=paste_points, paste_boxes=paste_boxes, order=order)
    if out is not None:
        if (not torch.is_tensor(out) or out.dtype != torch.float32 or tuple(out.shape) != (n_in, F)
                or not out.is_contiguous() or out.device != dev):
            raise ValueError(f"out must be a contiguous fp32 {(n_in, F)} tensor on the points' device")
    need = workspace_bytes(n_in)
    if workspace is None:
        workspace = _DEFAULT_WS
    if isinstance(workspace, PointsWorkspace):
        ws = workspace.get(need, dev)
    else:
        ws = workspace
        if (not torch.is_tensor(ws) or ws.dtype != torch.int32 or not ws.is_contiguous() or ws.device != dev
                or ws.numel() * 4 < need):
            raise ValueError(f"workspace must be a contiguous int32 tensor of at least {need} bytes on the points' device")
    if isinstance(shuffle, torch.Generator):
        if shuffle.device.type == "cpu":
            order = torch.randperm(n_in, generator=shuffle, dtype=torch.int32).to(dev, non_blocking=True)
        else:
            order = torch.randperm(n_in, generator=shuffle, dtype=torch.int32, device=dev)
    elif shuffle is True:
        order = torch.randperm(n_in, dtype=torch.int32, device=dev)
    if K and paste_boxes.shape[1] != 7:
        paste_boxes = paste_boxes[:, :7].contiguous()
    dst = out if out is not None else torch.empty((n_in, F), dtype=torch.float32, device=dev)
    cnt = torch.empty(1, dtype=torch.int32, device=dev)
    a.n_src, a.n_paste, a.F, a.K, a.paste_first = n_src, n_paste, F, K, int(bool(paste_first))
    a.src, a.count_in, a.paste, a.paste_boxes, a.order = _p(points), _p(count), _p(paste_points), _p(paste_boxes), _p(order)
    a.dst, a.count, a.workspace, a.workspace_bytes = _p(dst), _p(cnt), _p(ws), ws.numel() * 4
    _check(lib().cmt_pts_augment(ctypes.byref(a), _stream()), "cmt_pts_augment")
    return dst, cnt


def augment_boxes(boxes, labels, params, *, paste_boxes=None, paste_labels=None, point_cloud_range=None, num_classes,
                  gravity=False):
    """cmt_boxes_augment -> (boxes_out [n, D] fp32, labels_out [n] int64, count [1] int32) on the device, with
    n = len(boxes) + len(paste_boxes): rows [0, count) are the kept annotations in input order, the rest NaN / -1.

    ``boxes`` fp32 [n, 7 | 9] / ``labels`` int64 [n]: the ground truth; ``paste_boxes`` / ``paste_labels``: the
    sampled objects, appended behind it as every object sampler does.  ``params``: as ``augment_points``.
    ``point_cloud_range``: None or 6 values, ObjectRangeFilter's strict BEV test on the centre.  ``num_classes``:
    ObjectNameFilter, a label outside [0, num_classes) drops the box.  The yaw is wrapped by limit_yaw(0.5, 2 pi).
    ``gravity=True`` moves z from the bottom to the gravity centre: the [n, 9] rows ``head.forward_train`` takes."""
    boxes = _rows(boxes, "boxes", (7, 9))
    D = int(boxes.shape[1])
    if not torch.is_tensor(labels) or labels.dtype != torch.int64 or tuple(labels.shape) != (boxes.shape[0],):
        raise ValueError(f"labels must be an int64 [{boxes.shape[0]}] tensor")
    if (paste_boxes is None) != (paste_labels is None):
        raise ValueError("paste_boxes and paste_labels come together")
    if paste_boxes is not None:
        paste_boxes = _rows(paste_boxes, "paste_boxes", (D,))
        if (not torch.is_tensor(paste_labels) or paste_labels.dtype != torch.int64
                or tuple(paste_labels.shape) != (paste_boxes.shape[0],)):
            raise ValueError(f"paste_labels must be an int64 [{paste_boxes.shape[0]}] tensor")
    num_classes = int(num_classes)
    if num_classes < 0:
        raise ValueError(f"num_classes must not be negative, got {num_classes}")
    n = int(boxes.shape[0]) + (int(paste_boxes.shape[0]) if paste_boxes is not None else 0)
    if n > MAX_ANNOTATIONS:
        raise ValueError(f"at most {MAX_ANNOTATIONS} boxes, got {n}")
    a = N.BoxesAugmentArgs()
    _fill_xform(a.xf, params, point_cloud_range)
    dev = boxes.device
    _on_device(dev, labels=labels, paste_boxes=paste_boxes, paste_labels=paste_labels)
    if paste_boxes is not None:
        boxes, labels = torch.cat([boxes, paste_boxes], 0), torch.cat([labels, paste_labels], 0)
    labels = labels.contiguous()
    out_boxes = torch.empty((n, D), dtype=torch.float32, device=dev)
    out_labels = torch.empty(n, dtype=torch.int64, device=dev)
    cnt = torch.empty(1, dtype=torch.int32, device=dev)
    a.n, a.D, a.num_classes, a.gravity = n, D, num_classes, int(bool(gravity))
    a.boxes, a.labels, a.out_boxes, a.out_labels, a.count = _p(boxes), _p(labels), _p(out_boxes), _p(out_labels), _p(cnt)
    _check(lib().cmt_boxes_augment(ctypes.byref(a), _stream()), "cmt_boxes_augment")
    return out_boxes, out_labels, cnt


# ---- host side ---------------------------------------------------------------------------------------------------
def sample_augmentation(plan, rng):
    """One sample's parameters from ``rng`` (a numpy RandomState) in the reference's order of draws:
    GlobalRotScaleTransAll[Coop] draws ``uniform(*rot_range)``, ``uniform(*scale_ratio_range)`` and
    ``normal(scale=translation_std, size=3)`` (std as float32, as the reference builds it), CustomRandomFlip3D then
    ``rand() < flip_ratio_bev_horizontal`` and ``rand() < flip_ratio_bev_vertical``.  A step that ``plan`` (from
    ``train_plan_from_config``) does not have consumes no draw: its ``angle`` / ``scale`` / ``trans`` is None, its
    flips False.  With the reference's seed the numbers are the reference's."""
    out = dict(angle=None, scale=None, trans=None, flip_h=False, flip_v=False)
    if plan.get("rot_range") is not None:
        out["angle"] = float(rng.uniform(plan["rot_range"][0], plan["rot_range"][1]))
        out["scale"] = float(rng.uniform(plan["scale_ratio_range"][0], plan["scale_ratio_range"][1]))
        out["trans"] = rng.normal(scale=np.array(plan["translation_std"], dtype=np.float32), size=3).T
    if plan.get("flip_ratio_bev_horizontal") is not None:
        out["flip_h"] = bool(rng.rand() < plan["flip_ratio_bev_horizontal"])
        out["flip_v"] = bool(rng.rand() < plan["flip_ratio_bev_vertical"])
    return out


def augment_lidar2img(mats, params):
    """The lidar2img / lidar2cam update of GlobalRotScaleTransAll[Coop] and CustomRandomFlip3D for one 4 x 4 matrix
    or a stack: ``L @ inv(R4) @ inv(S4) @ inv(T4) @ F4`` in the reference's order, so that the augmented matrix
    projects an augmented point where the original projected the original point.  Host float64 throughout.
    Stated deviation: the reference multiplies the R and S steps in float32 torch (and so rounds the matrices to
    float32 on the way); this keeps float64.  The inputs are not modified."""
    m = np.asarray(mats, dtype=np.float64)
    if m.shape[-2:] != (4, 4):
        raise ValueError(f"4 x 4 matrices required, got {m.shape}")
    unknown = set(params) - _PARAM_KEYS
    if unknown:
        raise ValueError(f"params: unknown keys {sorted(unknown)}")
    out = m
    if params.get("angle") is not None:
        r4 = np.eye(4)
        r4[:3, :3] = rotation_matrix(params["angle"])
        out = out @ np.linalg.inv(r4)
    if params.get("scale") is not None:
        s = float(params["scale"])
        out = out @ np.linalg.inv(np.diag([s, s, s, 1.0]))
    if params.get("trans") is not None:
        t4 = np.eye(4)
        t4[:3, 3] = np.asarray(params["trans"], dtype=np.float64).reshape(3)
        out = out @ np.linalg.inv(t4)
    f4 = np.diag([-1.0 if params.get("flip_v") else 1.0, -1.0 if params.get("flip_h") else 1.0, 1.0, 1.0])
    return out @ f4


_SAMPLERS = ("ObjectSample", "ObjectSampleCoop", "UnifiedObjectSample", "UnifiedObjectSampleCoop")
_PASTE_FIRST = ("ObjectSample", "ObjectSampleCoop")   # points.cat([sampled_points, points])
_GRST = ("GlobalRotScaleTrans", "GlobalRotScaleTransCoop", "GlobalRotScaleTransAll", "GlobalRotScaleTransAllCoop")
_FLIP = ("RandomFlip3D", "CustomRandomFlip3D")


def train_plan_from_config(cfg):
    """The training-side point and box pipeline of a config dict (config.load_config): ``data.train`` (through
    CBGSDataset's ``dataset``), its [Unified]ObjectSample[Coop], GlobalRotScaleTrans[All][Coop],
    [Custom]RandomFlip3D, PointsRangeFilter[Coop], ObjectRangeFilter, ObjectNameFilter and PointShuffle[Coop] steps ->
    dict(sampler, paste_first, image_paste, rot_range, scale_ratio_range, translation_std,
    flip_ratio_bev_horizontal, flip_ratio_bev_vertical, point_cloud_range, object_range, num_classes, shuffle).

    ``sampler`` is the object sampler's type or None; ``paste_first`` tells where it concatenates the sampled points;
    ``image_paste`` reports ``sample_2d`` (the image pasting of ``unified_sample``, which is not performed here).
    The three transform entries are None without a GlobalRotScaleTrans step, the two flip ratios None without a
    flip step, the ranges None without their filters, ``num_classes`` None without ObjectNameFilter.
    Steps that are not built raise NotImplementedError naming them: ``shift_height``, ``ModalMask3D(mode='train')``,
    ``GlobalRotScaleTransImage``, and a flip step that follows the 2D flip (``sync_2d`` of mmdet3d's RandomFlip3D)."""
    train = cfg["data"]["train"]
    while isinstance(train, dict) and "pipeline" not in train and "dataset" in train:
        train = train["dataset"]   # CBGSDataset and other wrappers
    steps = list(_pipeline_steps(train["pipeline"]))
    plan = dict(sampler=None, paste_first=False, image_paste=False, rot_range=None, scale_ratio_range=None,
                translation_std=None, flip_ratio_bev_horizontal=None, flip_ratio_bev_vertical=None,
                point_cloud_range=None, object_range=None, num_classes=None, shuffle=False)
    for st in steps:
        kind = st.get("type")
        if kind == "ModalMask3D" and st.get("mode", "test") == "train":
            raise NotImplementedError("ModalMask3D(mode='train') is not built")
        if kind == "GlobalRotScaleTransImage":
            raise NotImplementedError("GlobalRotScaleTransImage is not built")
        if kind in _SAMPLERS:
            plan.update(sampler=kind, paste_first=kind in _PASTE_FIRST, image_paste=bool(st.get("sample_2d", False)))
        elif kind in _GRST:
            if st.get("shift_height", False):
                raise NotImplementedError(f"{kind}(shift_height=True) is not built")
            rot = st.get("rot_range", [-0.78539816, 0.78539816])
            rot = [-rot, rot] if isinstance(rot, (int, float)) else list(rot)
            std = st.get("translation_std", [0, 0, 0])
            std = [std] * 3 if isinstance(std, (int, float)) else list(std)
            plan.update(rot_range=[float(v) for v in rot],
                        scale_ratio_range=[float(v) for v in st.get("scale_ratio_range", [0.95, 1.05])],
                        translation_std=[float(v) for v in std])
        elif kind in _FLIP:
            if kind == "RandomFlip3D" and st.get("sync_2d", True):
                raise NotImplementedError("RandomFlip3D(sync_2d=True) follows the image flip and is not built")
            plan.update(flip_ratio_bev_horizontal=float(st.get("flip_ratio_bev_horizontal", 0.0)),
                        flip_ratio_bev_vertical=float(st.get("flip_ratio_bev_vertical", 0.0)))
        elif kind in ("PointsRangeFilter", "PointsRangeFilterCoop"):
            plan["point_cloud_range"] = [float(v) for v in st["point_cloud_range"]]
        elif kind == "ObjectRangeFilter":
            plan["object_range"] = [float(v) for v in st["point_cloud_range"]]
        elif kind == "ObjectNameFilter":
            plan["num_classes"] = len(st["classes"])
        elif kind in ("PointShuffle", "PointShuffleCoop"):
            plan["shuffle"] = True
    return plan
