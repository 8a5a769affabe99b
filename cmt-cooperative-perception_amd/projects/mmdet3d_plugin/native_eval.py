"""Detection evaluation on the device: the ctypes binding of cmt_det_eval_* (include/cmt_hip.h, csrc/deteval.hip).

``det_eval`` takes predictions (boxes, scores, labels, sample indices) and ground truth that live on the device
and returns the per-prediction match results and the per-(class, threshold) curves, AP and TP errors of the
contract in cmt_hip.h: keys -> three stable ``torch.sort`` calls (plumbing) -> match -> curves, all on the current
stream with no host read.  ``det_eval_iou`` is the same with the IoU match (cmt_det_eval_match_iou) in place of the
centre distance and the interpolated APs (cmt_det_eval_ap_interp) behind the curves.  ``core/evaluation`` wraps both
into metrics dictionaries.

Like native_sparse.py: argument checks raise ValueError before the device check, tensors must live on a HIP device,
there is no CPU path.
"""
import ctypes
import math

import torch

from ._argcheck import count_word, rows, same_device, tensor
from .native import DetIouArgs, _check, _i64, _int, _p, _stream, _vp, lib

__all__ = ["MAX_CLASSES", "MAX_THRESHOLDS", "MAX_SAMPLES", "MAX_PER_SAMPLE", "NELEM", "DetEvalArgs", "DetIouArgs",
           "eval_lib", "workspace_bytes", "check_config", "check_iou_config", "det_eval", "det_eval_iou", "IOU_MODES"]

IOU_MODES = {"bev": 0, "3d": 1}   # cmt_det_iou_args.mode

MAX_CLASSES = 32       # cmt_hip.h CMT_DET_MAX_CLASSES
MAX_THRESHOLDS = 8     # cmt_hip.h CMT_DET_MAX_THRESHOLDS
NELEM = 101            # cmt_hip.h CMT_DET_NELEM
MAX_SAMPLES = 1 << 24
MAX_PER_SAMPLE = 1024  # predictions per sample the evaluator accepts
ERR_NAMES = ("trans_err", "vel_err", "scale_err", "orient_err")   # the order of err[] and of the curves 3..6
_dbl = ctypes.c_double


class DetEvalArgs(ctypes.Structure):
    _fields_ = [("N", _i64), ("G", _i64),
                ("S", _int), ("C", _int), ("T", _int), ("tp_index", _int), ("first_ind", _int), ("reserved", _int),
                ("range", _dbl * MAX_CLASSES), ("yaw_period", _dbl * MAX_CLASSES), ("dist_th", _dbl * MAX_THRESHOLDS),
                ("min_precision", _dbl),
                ("pred_box", _vp), ("pred_score", _vp), ("pred_label", _vp), ("pred_sample", _vp),
                ("gt_box", _vp), ("gt_label", _vp), ("gt_sample", _vp), ("gt_num_pts", _vp),
                ("n_pred", _vp), ("n_gt", _vp),
                ("key_class", _vp), ("key_sample", _vp), ("key_gt", _vp),
                ("sk_class", _vp), ("si_class", _vp), ("sk_sample", _vp), ("si_sample", _vp), ("sk_gt", _vp),
                ("si_gt", _vp),
                ("tp", _vp), ("match_gt", _vp), ("err", _vp), ("npos", _vp),
                ("md", _vp), ("ap", _vp), ("tp_err", _vp),
                ("workspace", _vp), ("workspace_bytes", _i64)]


_READY = False


def eval_lib():
    """libcmt_hip.so with the cmt_det_eval_* signatures set and the struct mirror checked (no device needed)"""
    global _READY
    L = lib()
    if not _READY:
        P = ctypes.POINTER(DetEvalArgs)
        L.cmt_det_eval_args_size.argtypes, L.cmt_det_eval_args_size.restype = [], _i64
        L.cmt_det_eval_workspace_bytes.argtypes = [_i64, _i64, _int, _int, _int]
        L.cmt_det_eval_workspace_bytes.restype = _i64
        for name in ("cmt_det_eval_keys", "cmt_det_eval_match", "cmt_det_eval_curves"):
            fn = getattr(L, name)
            fn.argtypes, fn.restype = [P, _vp], _int
        for name in ("cmt_det_eval_match_iou", "cmt_det_eval_ap_interp"):
            getattr(L, name).argtypes = [P, ctypes.POINTER(DetIouArgs), _vp]
        got = L.cmt_det_eval_args_size()
        if got != ctypes.sizeof(DetEvalArgs):
            raise RuntimeError(f"cmt_det_eval_args: library struct is {got} bytes, the ctypes mirror "
                               f"{ctypes.sizeof(DetEvalArgs)} (stale binding)")
        _READY = True
    return L


def _check_dims(N, G, S, C, T):
    if not 0 <= N < 2 ** 31 or not 0 <= G < 2 ** 31:
        raise ValueError(f"N and G must be in [0, 2^31), got {N} and {G}")
    if not 1 <= S <= MAX_SAMPLES:
        raise ValueError(f"S must be in [1, 2^24], got {S}")
    if not 1 <= C <= MAX_CLASSES:
        raise ValueError(f"at most {MAX_CLASSES} classes (and at least one), got {C}")
    if not 1 <= T <= MAX_THRESHOLDS:
        raise ValueError(f"at most {MAX_THRESHOLDS} distance thresholds (and at least one), got {T}")


def workspace_bytes(N, G, S, C, T):
    _check_dims(N, G, S, C, T)
    return int(eval_lib().cmt_det_eval_workspace_bytes(N, G, S, C, T))


def check_config(class_range, yaw_period, dist_ths, dist_th_tp, min_recall, min_precision):
    """the checked configuration -> (ranges, periods, thresholds, tp_index, first_ind, min_precision)"""
    rng = [float(v) for v in class_range]
    per = [float(v) for v in yaw_period]
    ths = [float(v) for v in dist_ths]
    if len(rng) != len(per):
        raise ValueError(f"{len(rng)} class ranges but {len(per)} yaw periods")
    _check_dims(0, 0, 1, len(rng), len(ths))
    for name, vals in (("class_range", rng), ("yaw_period", per), ("dist_ths", ths)):
        if any(not math.isfinite(v) or v <= 0 for v in vals):
            raise ValueError(f"{name} must be finite and positive, got {vals}")
    if float(dist_th_tp) not in ths:
        raise ValueError(f"dist_th_tp {dist_th_tp} is not one of dist_ths {ths}")
    if not 0 <= min_precision < 1:
        raise ValueError(f"min_precision must be in [0, 1), got {min_precision}")
    if not 0 <= min_recall <= 1:
        raise ValueError(f"min_recall must be in [0, 1], got {min_recall}")
    first_ind = round(100 * min_recall) + 1
    if not 1 <= first_ind <= 100:
        raise ValueError(f"min_recall {min_recall} leaves no recall bin (first index {first_ind})")
    return rng, per, ths, ths.index(float(dist_th_tp)), first_ind, float(min_precision)


def det_eval(pred_boxes, pred_scores, pred_labels, pred_samples, gt_boxes, gt_labels, gt_samples, gt_num_pts, *,
             num_samples, class_range, yaw_period, dist_ths, dist_th_tp, min_recall=0.1, min_precision=0.1,
             n_pred=None, n_gt=None, out=None, workspace=None, events=None):
    """The contract of cmt_hip.h for N prediction rows and G ground-truth rows -> dict of device tensors:
    ``tp`` uint8 [T, N], ``match_gt`` int32 [T, N] (ground-truth row, -1: none), ``err`` float64 [T, 4, N] (trans, vel,
    scale, orient; NaN without a match), ``npos`` int32 [C], ``md`` float64 [C, T, 7, 101] (recall, precision,
    confidence, then the four error curves), ``ap`` float64 [C, T], ``tp_err`` float64 [C, 4].  Nothing is read
    back to the host.

    ``pred_boxes`` fp32 [N, 9], ``pred_scores`` fp32 [N], ``pred_labels`` / ``pred_samples`` int32 [N];
    ``gt_boxes`` fp32 [G, 9], ``gt_labels`` / ``gt_samples`` / ``gt_num_pts`` int32 [G].  ``n_pred`` / ``n_gt``: one
    device int32 each, the rows actually filled (default: all).  ``out``: a dict of the seven tensors to write into;
    ``workspace``: a uint8 tensor of at least ``workspace_bytes(N, G, S, C, T)`` bytes.  ``events``: a list that
    receives (phase name, start event, end event) for keys, sort, match and curves (for measurements)."""
    def config():
        return check_config(class_range, yaw_period, dist_ths, dist_th_tp, min_recall, min_precision), None

    return _det_eval(pred_boxes, pred_scores, pred_labels, pred_samples, gt_boxes, gt_labels, gt_samples, gt_num_pts,
                     num_samples, config, n_pred, n_gt, out, workspace, events)


def check_iou_config(class_range, yaw_period, iou_ths, iou_th_tp, mode, z_origin, min_recall, min_precision):
    """the checked IoU configuration -> (check_config's tuple with the IoU thresholds in place of the distances,
    (mode word, z_origin))"""
    ths = [float(v) for v in iou_ths]
    if not 1 <= len(ths) <= MAX_THRESHOLDS:
        raise ValueError(f"at most {MAX_THRESHOLDS} IoU thresholds (and at least one), got {len(ths)}")
    if any(not math.isfinite(v) or not 0 <= v < 1 for v in ths):
        raise ValueError(f"iou_ths must be in [0, 1), got {ths}")
    if float(iou_th_tp) not in ths:
        raise ValueError(f"iou_th_tp {iou_th_tp} is not one of iou_ths {ths}")
    if mode not in IOU_MODES:
        raise ValueError(f"mode must be 'bev' or '3d', got {mode!r}")
    if float(z_origin) not in (0.0, 0.5):
        raise ValueError(f"z_origin must be 0 or 0.5, got {z_origin}")
    # the base struct wants positive distances; the IoU match does not read them
    rng, per, _, _, first_ind, min_prec = check_config(class_range, yaw_period, [1.0] * len(ths), 1.0, min_recall,
                                                       min_precision)
    return (rng, per, ths, ths.index(float(iou_th_tp)), first_ind, min_prec), (IOU_MODES[mode], float(z_origin))


def det_eval_iou(pred_boxes, pred_scores, pred_labels, pred_samples, gt_boxes, gt_labels, gt_samples, gt_num_pts, *,
                 num_samples, class_range, yaw_period, iou_ths, iou_th_tp, mode="3d", z_origin=0.5, min_recall=0.1,
                 min_precision=0.1, n_pred=None, n_gt=None, out=None, workspace=None, events=None):
    """``det_eval`` with the IoU match of cmt_hip.h (cmt_det_eval_match_iou: the largest BEV or 3D IoU above
    ``iou_ths[t]``, the ground truth as the first box) in place of the centre distance: keys -> sorts -> match_iou ->
    curves -> ap_interp.  The same arguments and the same dict, plus ``match_iou`` fp32 [T, N] (NaN without a match)
    and ``ap_interp`` float64 [C, T, 2] (all-point AP, 40-point AP).  ``events`` also receives ap_interp."""
    def config():
        return check_iou_config(class_range, yaw_period, iou_ths, iou_th_tp, mode, z_origin, min_recall, min_precision)

    return _det_eval(pred_boxes, pred_scores, pred_labels, pred_samples, gt_boxes, gt_labels, gt_samples, gt_num_pts,
                     num_samples, config, n_pred, n_gt, out, workspace, events)


def _det_eval(pred_boxes, pred_scores, pred_labels, pred_samples, gt_boxes, gt_labels, gt_samples, gt_num_pts,
              num_samples, config, n_pred, n_gt, out, workspace, events):
    """the shared body.  ``config()`` -> (check_config's tuple, iou): iou None for the centre distance, or (mode word,
    z_origin) with the IoU thresholds in the tuple's threshold slot; it is called after the tensor checks"""
    N = int(rows(pred_boxes, "pred_boxes", (9,)).shape[0])
    G = int(rows(gt_boxes, "gt_boxes", (9,)).shape[0])
    for name, t, dt, n in (("pred_scores", pred_scores, torch.float32, N), ("pred_labels", pred_labels, torch.int32, N),
                           ("pred_samples", pred_samples, torch.int32, N), ("gt_labels", gt_labels, torch.int32, G),
                           ("gt_samples", gt_samples, torch.int32, G), ("gt_num_pts", gt_num_pts, torch.int32, G)):
        if rows(t, name, None, dt).shape[0] < n:
            raise ValueError(f"{name} is short: {t.shape[0]} rows for {n} boxes")
    count_word(n_pred, "n_pred"), count_word(n_gt, "n_gt")
    (rng, per, ths, tp_index, first_ind, min_prec), iou = config()
    S, C, T = int(num_samples), len(rng), len(ths)
    _check_dims(N, G, S, C, T)
    tensors = dict(pred_scores=pred_scores, pred_labels=pred_labels, pred_samples=pred_samples, gt_boxes=gt_boxes,
                   gt_labels=gt_labels, gt_samples=gt_samples, gt_num_pts=gt_num_pts, n_pred=n_pred, n_gt=n_gt)
    shapes = dict(tp=((T, N), torch.uint8), match_gt=((T, N), torch.int32), err=((T, 4, N), torch.float64),
                  npos=((C,), torch.int32), md=((C, T, 7, NELEM), torch.float64), ap=((C, T), torch.float64),
                  tp_err=((C, 4), torch.float64))
    base = tuple(shapes)
    if iou is not None:
        shapes.update(match_iou=((T, N), torch.float32), ap_interp=((C, T, 2), torch.float64))
    if out is not None:
        for k, (shape, dt) in shapes.items():
            tensors[f"out[{k!r}]"] = tensor(out.get(k), f"out[{k!r}]", dt, shape)
    if workspace is not None:
        if not torch.is_tensor(workspace) or workspace.dtype != torch.uint8 or not workspace.is_contiguous():
            raise ValueError("workspace must be a contiguous uint8 tensor")
        tensors["workspace"] = workspace
    dev = pred_boxes.device
    same_device(dev, "detection evaluation needs its tensors", **tensors)
    L = eval_lib()
    need = int(L.cmt_det_eval_workspace_bytes(N, G, S, C, T))
    if workspace is None:
        workspace = torch.empty(need, dtype=torch.uint8, device=dev)
    elif workspace.numel() < need or workspace.data_ptr() % 8:
        raise ValueError(f"workspace must hold at least {need} bytes and be 8-byte aligned")
    if out is None:
        out = {k: torch.empty(shape, dtype=dt, device=dev) for k, (shape, dt) in shapes.items()}

    a = DetEvalArgs()
    a.N, a.G, a.S, a.C, a.T, a.tp_index, a.first_ind = N, G, S, C, T, tp_index, first_ind
    a.range[:C], a.yaw_period[:C], a.min_precision = rng, per, min_prec
    a.dist_th[:T] = ths if iou is None else [1.0] * T   # validated, not read by the IoU match
    a.pred_box, a.pred_score, a.pred_label, a.pred_sample = _p(pred_boxes), _p(pred_scores), _p(pred_labels), _p(pred_samples)
    a.gt_box, a.gt_label, a.gt_sample, a.gt_num_pts = _p(gt_boxes), _p(gt_labels), _p(gt_samples), _p(gt_num_pts)
    a.n_pred, a.n_gt = _p(n_pred), _p(n_gt)
    keys = torch.empty(2 * N + G, dtype=torch.int64, device=dev)
    kc, ks, kg = keys[:N], keys[N:2 * N], keys[2 * N:]
    a.key_class, a.key_sample, a.key_gt = _p(kc), _p(ks), _p(kg)
    for k in base:
        setattr(a, k, _p(out[k]))
    if iou is not None:
        b = DetIouArgs()
        b.mode, b.z_origin = iou
        b.iou_th[:T] = ths
        b.match_iou, b.ap_interp = _p(out["match_iou"]), _p(out["ap_interp"])
    a.workspace, a.workspace_bytes = _p(workspace), workspace.numel()
    st = _stream()

    def mark():
        if events is None:
            return None
        e = torch.cuda.Event(enable_timing=True)
        e.record()
        return e

    e0 = mark()
    _check(L.cmt_det_eval_keys(ctypes.byref(a), st), "cmt_det_eval_keys")
    e1 = mark()
    # the sorts are plumbing: stable, so equal keys keep the order the key kernel laid out
    sk_c, si_c = torch.sort(kc, stable=True)
    sk_s, si_s = torch.sort(ks, stable=True)
    sk_g, si_g = torch.sort(kg, stable=True)
    a.sk_class, a.si_class, a.sk_sample, a.si_sample = _p(sk_c), _p(si_c), _p(sk_s), _p(si_s)
    a.sk_gt, a.si_gt = _p(sk_g), _p(si_g)
    e2 = mark()
    if iou is None:
        _check(L.cmt_det_eval_match(ctypes.byref(a), st), "cmt_det_eval_match")
    else:
        _check(L.cmt_det_eval_match_iou(ctypes.byref(a), ctypes.byref(b), st), "cmt_det_eval_match_iou")
    e3 = mark()
    _check(L.cmt_det_eval_curves(ctypes.byref(a), st), "cmt_det_eval_curves")
    e4 = mark()
    if iou is not None:
        _check(L.cmt_det_eval_ap_interp(ctypes.byref(a), ctypes.byref(b), st), "cmt_det_eval_ap_interp")
        e5 = mark()
    if events is not None:
        events.extend([("keys", e0, e1), ("sort", e1, e2), ("match", e2, e3), ("curves", e3, e4)])
        if iou is not None:
            events.append(("ap_interp", e4, e5))
    # the sorted arrays are read by the launches above: torch's caching allocator keeps their memory
    # stream-ordered, so dropping the references here is safe on this stream
    return out
