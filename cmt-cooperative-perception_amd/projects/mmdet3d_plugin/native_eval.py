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

from ._argcheck import count_word, rows, same_device, strided_rows, tensor
from .native import DetIouArgs, LsapArgs, _check, _i64, _int, _p, _stream, _vp, lib

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


# ---- tracking evaluation (cmt_mot_eval_*, csrc/moteval.hip) ------------------------------------------------------
MOT_MAX_CLASSES = 64        # cmt_hip.h CMT_MOT_MAX_CLASSES
MOT_MAX_THRESHOLDS = 64     # CMT_MOT_MAX_THRESHOLDS
MOT_MAX_GT_TRACKS = 65536   # CMT_MOT_MAX_GT_TRACKS
MOT_MAX_GT = 512            # CMT_MOT_MAX_GT: kept ground truth per (frame, class)
MOT_MAX_PRED = 2048         # CMT_MOT_MAX_PRED: active predictions per (frame, class)
MOT_MAX_CHAINS = 65535      # CMT_MOT_MAX_CHAINS: chains per call (cmt_lsap's problems per call)
MOT_RUN_PARTS = 64          # CMT_MOT_RUN_PARTS: the slices cmt_mot_eval_runs reports the longest runs of
MOT_MAX_SCENE_STEPS = 1 << 24
MOT_WORKSPACE = 256 << 20   # the default budget of a block of chains
MOT_COUNTERS = ("tp", "fp", "fn", "ids", "frag", "npred")   # the order of the six counters
MOT_METRICS = ("recall", "mota", "motp", "motar")           # the order of metrics[..., 4]
MOT_CLASS_SUM = ("amota", "amotp", "best", "mota", "motp", "recall", "tp", "fp", "fn", "ids", "frag", "thr")
_flt = ctypes.c_float

__all__ += ["MotEvalArgs", "mot_lib", "check_mot_config", "mot_recall_levels", "mot_eval", "MOT_COUNTERS", "MOT_METRICS",
            "MOT_CLASS_SUM", "MOT_WORKSPACE"]


class MotEvalArgs(ctypes.Structure):
    _fields_ = [("N", _i64), ("G", _i64),
                ("F", _int), ("S", _int), ("Fmax", _int), ("C", _int), ("R", _int), ("ld_pred", _int), ("ld_gt", _int),
                ("max_gt_tracks", _int),
                ("phase", _int), ("step", _int), ("chain0", _int), ("nchains", _int), ("Gmax", _int), ("Hmax", _int),
                ("range", _dbl * MOT_MAX_CLASSES), ("recall", _dbl * MOT_MAX_THRESHOLDS), ("dist_th", _flt * MOT_MAX_CLASSES),
                ("pred_box", _vp), ("pred_score", _vp), ("pred_label", _vp), ("pred_track", _vp), ("pred_frame", _vp),
                ("gt_box", _vp), ("gt_label", _vp), ("gt_frame", _vp), ("gt_inst", _vp),
                ("n_pred", _vp), ("n_gt", _vp), ("frame_tab", _vp),
                ("key_pred", _vp), ("key_gt", _vp), ("sk_pred", _vp), ("sk_gt", _vp),
                ("npos", _vp), ("run_max", _vp), ("tp_score", _vp), ("tp_key", _vp), ("sk_tp", _vp), ("si_tp", _vp),
                ("thr", _vp),
                ("chain_cnt1", _vp), ("chain_dist1", _vp), ("chain_cnt2", _vp), ("chain_dist2", _vp),
                ("state_m", _vp), ("state_lost", _vp), ("cost", _vp), ("desc", _vp), ("cols", _vp), ("smatch", _vp),
                ("match_q", _vp), ("match_g", _vp),
                ("counters", _vp), ("dist_sum", _vp), ("metrics", _vp), ("class_sum", _vp), ("counters1", _vp),
                ("dist_sum1", _vp)]


_MOT_CALLS = ("cmt_mot_eval_keys", "cmt_mot_eval_runs", "cmt_mot_eval_cost", "cmt_mot_eval_update",
              "cmt_mot_eval_thresholds", "cmt_mot_eval_summary")
_MOT_READY = False


def mot_lib():
    """libcmt_hip.so with the cmt_mot_eval_* signatures set and the struct mirror checked (no device needed)"""
    global _MOT_READY
    L = lib()
    if not _MOT_READY:
        L.cmt_mot_eval_args_size.argtypes, L.cmt_mot_eval_args_size.restype = [], _i64
        for name in _MOT_CALLS:
            fn = getattr(L, name)
            fn.argtypes, fn.restype = [ctypes.POINTER(MotEvalArgs), _vp], _int
        got = L.cmt_mot_eval_args_size()
        if got != ctypes.sizeof(MotEvalArgs):
            raise RuntimeError(f"cmt_mot_eval_args: library struct is {got} bytes, the ctypes mirror "
                               f"{ctypes.sizeof(MotEvalArgs)} (stale binding)")
        _MOT_READY = True
    return L


def mot_recall_levels(num_thresholds, min_recall):
    """the R recall levels of the contract in float64: r_k = min_recall + k (1 - min_recall) / (R - 1), r_0 = 1 for
    R = 1"""
    R = int(num_thresholds)
    if not 1 <= R <= MOT_MAX_THRESHOLDS:
        raise ValueError(f"num_thresholds must be in [1, {MOT_MAX_THRESHOLDS}], got {num_thresholds}")
    lo = float(min_recall)
    if not 0 < lo <= 1:
        raise ValueError(f"min_recall must be in (0, 1], got {min_recall}")
    return [1.0] if R == 1 else [lo + k * (1.0 - lo) / (R - 1) for k in range(R)]


def check_mot_config(class_range, dist_th, recall, max_gt_tracks):
    """the checked configuration -> (ranges, distance thresholds, recall levels, max_gt_tracks)"""
    rng = [float(v) for v in class_range]
    dth = [float(v) for v in dist_th]
    rec = [float(v) for v in recall]
    if not 1 <= len(rng) <= MOT_MAX_CLASSES:
        raise ValueError(f"at most {MOT_MAX_CLASSES} classes (and at least one), got {len(rng)}")
    if len(dth) != len(rng):
        raise ValueError(f"{len(rng)} class ranges but {len(dth)} distance thresholds")
    if not 1 <= len(rec) <= MOT_MAX_THRESHOLDS:
        raise ValueError(f"at most {MOT_MAX_THRESHOLDS} recall levels (and at least one), got {len(rec)}")
    for name, vals in (("class_range", rng), ("dist_th", dth)):
        if any(not math.isfinite(v) or v <= 0 for v in vals):
            raise ValueError(f"{name} must be finite and positive, got {vals}")
    if any(not 0 < v <= 1 for v in rec):
        raise ValueError(f"recall levels must be in (0, 1], got {rec}")
    if not 1 <= int(max_gt_tracks) <= MOT_MAX_GT_TRACKS:
        raise ValueError(f"max_gt_tracks must be in [1, {MOT_MAX_GT_TRACKS}], got {max_gt_tracks}")
    return rng, dth, rec, int(max_gt_tracks)


def _mot_chain_bytes(gmax, hmax, max_gt_tracks):
    """the workspace one chain of a block needs: the cost matrix and cmt_lsap's copy, the state, the lists"""
    return 8 * gmax * hmax + 5 * max_gt_tracks + 8 * hmax + 8 * gmax + 36


def mot_eval(pred_boxes, pred_scores, pred_labels, pred_tracks, pred_frames, gt_boxes, gt_labels, gt_frames, gt_inst,
             frame_table, *, num_scenes, max_steps, class_range, dist_th, recall, max_gt_tracks, n_pred=None, n_gt=None,
             workspace_bytes=MOT_WORKSPACE, alloc=None, events=None):
    """The tracking evaluation of cmt_hip.h (cmt_mot_eval_*) -> dict of device tensors: ``npos`` int32 [C], ``run_max``
    int32 [2], ``tp_score`` fp32 [G], ``thr`` fp32 [C, R], ``counters`` int64 [C, R, 6] (MOT_COUNTERS), ``dist_sum``
    float64 [C, R], ``metrics`` float64 [C, R, 4] (MOT_METRICS), ``class_sum`` float64 [C, 12] (MOT_CLASS_SUM),
    ``counters1`` int64 [C, 6] and ``dist_sum1`` float64 [C] (phase 1: every prediction active).

    ``pred_boxes`` fp32 [N, >= 2] (a row stride will do; columns 0 and 1 are read), ``pred_scores`` fp32 [N],
    ``pred_labels`` / ``pred_tracks`` / ``pred_frames`` int32 [N]; ``gt_boxes`` fp32 [G, >= 2], ``gt_labels`` /
    ``gt_frames`` / ``gt_inst`` int32 [G]; ``frame_table`` int32 [F, 2], the (scene, step) of every frame, on the
    device.  ``num_scenes`` S and ``max_steps`` Fmax (the longest scene) size the chains.  ``recall``: the levels
    (``mot_recall_levels``).  ``workspace_bytes``: the budget of one block of chains; the chains are split into blocks
    that fit it (at least one chain, at most 65535), and the result does not depend on the split.  ``alloc(name, shape,
    dtype)``: the allocator of every buffer (default ``torch.empty`` on the device).  ``events``: a list that receives
    (kernel name, start event, end event) per launch group.

    keys -> two sorts -> runs -> ONE host read (the longest runs, which size the matrices) -> per block and step cost,
    cmt_lsap, update -> a sort -> thresholds -> the same loop per achieved slot -> summary."""
    N, ld_pred = strided_rows(pred_boxes, "pred_boxes", 2)
    G, ld_gt = strided_rows(gt_boxes, "gt_boxes", 2)
    for name, t, dt, n in (("pred_scores", pred_scores, torch.float32, N), ("pred_labels", pred_labels, torch.int32, N),
                           ("pred_tracks", pred_tracks, torch.int32, N), ("pred_frames", pred_frames, torch.int32, N),
                           ("gt_labels", gt_labels, torch.int32, G), ("gt_frames", gt_frames, torch.int32, G),
                           ("gt_inst", gt_inst, torch.int32, G)):
        if rows(t, name, None, dt).shape[0] < n:
            raise ValueError(f"{name} is short: {t.shape[0]} rows for {n} boxes")
    rows(frame_table, "frame_table", (2,), torch.int32)
    count_word(n_pred, "n_pred"), count_word(n_gt, "n_gt")
    rng, dth, rec, mgt = check_mot_config(class_range, dist_th, recall, max_gt_tracks)
    F, S, Fmax, C, R = int(frame_table.shape[0]), int(num_scenes), int(max_steps), len(rng), len(rec)
    if not 0 <= N < 2 ** 31 or not 0 <= G < 2 ** 31:
        raise ValueError(f"N and G must be in [0, 2^31), got {N} and {G}")
    if F < 1 or S < 1 or Fmax < 1 or S * Fmax > MOT_MAX_SCENE_STEPS:
        raise ValueError(f"frames, num_scenes and max_steps must be at least 1 and num_scenes * max_steps at most 2^24, "
                         f"got {F}, {S}, {Fmax}")
    if S * C * R >= 2 ** 31:
        raise ValueError(f"num_scenes * classes * recall levels must be below 2^31, got {S * C * R}")
    if int(workspace_bytes) < 1:
        raise ValueError(f"workspace_bytes must be positive, got {workspace_bytes}")
    dev = pred_boxes.device
    same_device(dev, "tracking evaluation needs its tensors", pred_scores=pred_scores, pred_labels=pred_labels,
                pred_tracks=pred_tracks, pred_frames=pred_frames, gt_boxes=gt_boxes, gt_labels=gt_labels,
                gt_frames=gt_frames, gt_inst=gt_inst, frame_table=frame_table, n_pred=n_pred, n_gt=n_gt)
    L = mot_lib()
    if alloc is None:
        def alloc(name, shape, dtype):
            return torch.empty(shape, dtype=dtype, device=dev)
    i32, i64, f32, f64 = torch.int32, torch.int64, torch.float32, torch.float64
    run_parts = alloc("run_max", (2, MOT_RUN_PARTS), i32)
    out = dict(npos=alloc("npos", (C,), i32), tp_score=alloc("tp_score", (G,), f32),
               thr=alloc("thr", (C, R), f32), counters=alloc("counters", (C, R, 6), i64),
               dist_sum=alloc("dist_sum", (C, R), f64), metrics=alloc("metrics", (C, R, 4), f64),
               class_sum=alloc("class_sum", (C, 12), f64), counters1=alloc("counters1", (C, 6), i64),
               dist_sum1=alloc("dist_sum1", (C,), f64))
    key_pred, key_gt, tp_key = alloc("key_pred", (N,), i64), alloc("key_gt", (G,), i64), alloc("tp_key", (G,), i64)
    cc1, cd1 = alloc("chain_cnt1", (S * C, 6), i64), alloc("chain_dist1", (S * C,), f64)
    cc2, cd2 = alloc("chain_cnt2", (S * C * R, 6), i64), alloc("chain_dist2", (S * C * R,), f64)

    a = MotEvalArgs()
    a.N, a.G, a.F, a.S, a.Fmax, a.C, a.R, a.ld_pred, a.ld_gt, a.max_gt_tracks = N, G, F, S, Fmax, C, R, ld_pred, ld_gt, mgt
    a.range[:C], a.dist_th[:C], a.recall[:R] = rng, dth, rec
    a.pred_box, a.pred_score, a.pred_label = _p(pred_boxes), _p(pred_scores), _p(pred_labels)
    a.pred_track, a.pred_frame = _p(pred_tracks), _p(pred_frames)
    a.gt_box, a.gt_label, a.gt_frame, a.gt_inst = _p(gt_boxes), _p(gt_labels), _p(gt_frames), _p(gt_inst)
    a.n_pred, a.n_gt, a.frame_tab = _p(n_pred), _p(n_gt), _p(frame_table)
    a.key_pred, a.key_gt, a.tp_key = _p(key_pred), _p(key_gt), _p(tp_key)
    a.chain_cnt1, a.chain_dist1, a.chain_cnt2, a.chain_dist2 = _p(cc1), _p(cd1), _p(cc2), _p(cd2)
    for k, t in out.items():
        setattr(a, k, _p(t))
    a.run_max = _p(run_parts)
    st = _stream()

    def call(name, kernel):
        e0 = None
        if events is not None:
            e0 = torch.cuda.Event(enable_timing=True)
            e0.record()
        kernel()
        if events is not None:
            e1 = torch.cuda.Event(enable_timing=True)
            e1.record()
            events.append((name, e0, e1))

    def native(name):
        call(name[len("cmt_mot_eval_"):], lambda: _check(getattr(L, name)(ctypes.byref(a), st), name))

    native("cmt_mot_eval_keys")
    # the sorts are plumbing; the row is the key's low word, so no two kept keys are equal
    sorted_keys = []
    call("sort", lambda: sorted_keys.extend((torch.sort(key_pred)[0], torch.sort(key_gt)[0])))
    sk_pred, sk_gt = sorted_keys
    a.sk_pred, a.sk_gt = _p(sk_pred), _p(sk_gt)
    native("cmt_mot_eval_runs")
    out["run_max"] = run_parts.amax(dim=1)
    gmax, hmax = (int(v) for v in out["run_max"].cpu())   # the one host read: it sizes the matrices
    if gmax > MOT_MAX_GT or hmax > MOT_MAX_PRED:
        raise ValueError(f"a (frame, class) holds {gmax} ground-truth boxes and {hmax} predictions; at most {MOT_MAX_GT} and "
                         f"{MOT_MAX_PRED} are supported")
    gmax, hmax = max(gmax, 1), max(hmax, 1)
    block = max(1, min(MOT_MAX_CHAINS, int(workspace_bytes) // _mot_chain_bytes(gmax, hmax, mgt)))
    block = min(block, S * C * R)
    ws = dict(state_m=alloc("state_m", (block, mgt), i32), state_lost=alloc("state_lost", (block, mgt), torch.uint8),
              cost=alloc("cost", (block, gmax, hmax), f32), desc=alloc("desc", (block, 4), i64),
              cols=alloc("cols", (block, hmax), i32), smatch=alloc("smatch", (block, gmax), i32),
              match_q=alloc("match_q", (block, hmax), i32), match_g=alloc("match_g", (block, gmax), i32))
    status = alloc("status", (block,), i32)
    lsap_bytes = int(L.cmt_lsap_workspace_bytes(block, gmax, hmax))
    lsap_ws = alloc("lsap_workspace", (max(lsap_bytes, 4) // 4,), f32)
    for k, t in ws.items():
        setattr(a, k, _p(t))
    a.Gmax, a.Hmax = gmax, hmax
    la = LsapArgs()
    la.max_nq, la.max_ngt = gmax, hmax
    la.cost, la.desc = ws["cost"].data_ptr(), ws["desc"].data_ptr()
    la.match_q, la.ld_q, la.match_g, la.ld_g = ws["match_q"].data_ptr(), hmax, ws["match_g"].data_ptr(), gmax
    la.status, la.workspace, la.workspace_bytes = status.data_ptr(), lsap_ws.data_ptr(), lsap_bytes

    def phase(number, chains):
        a.phase = number
        for c0 in range(0, chains, block):
            a.chain0, a.nchains = c0, min(block, chains - c0)
            la.P, la.cost_elems = a.nchains, a.nchains * gmax * hmax
            for step in range(Fmax):
                a.step = step
                native("cmt_mot_eval_cost")
                call("lsap", lambda: _check(L.cmt_lsap(ctypes.byref(la), st), "cmt_lsap"))
                native("cmt_mot_eval_update")

    phase(1, S * C)
    sorted_tp = []
    call("sort", lambda: sorted_tp.extend(torch.sort(tp_key, stable=True)))
    a.sk_tp, a.si_tp = _p(sorted_tp[0]), _p(sorted_tp[1])
    native("cmt_mot_eval_thresholds")
    phase(2, S * C * R)
    native("cmt_mot_eval_summary")
    return out
