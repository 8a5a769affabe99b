"""nuScenes-style detection evaluation (AP per distance threshold, the four TP errors, NDS) for boxes on the device.

The arithmetic is the contract of ``cmt_det_eval_*`` in include/cmt_hip.h (csrc/deteval.hip), a restatement of the
evaluator the reference carries in its dataset class (a9coop_dataset.py: accumulate, cummean, calc_ap, calc_tp,
filter_eval_boxes, _evaluate_a9_nusc).  ``DetectionEvaluator`` collects frames in device buffers without a host
read; ``compute()`` runs sort -> match -> curves on the device and reads back C x T APs and C x 4 errors, the means
over them (nine classes, four numbers each) are float64 on the host.

``TrackingEvaluator`` scores tracked boxes (``native_track.Tracker``'s ids) against ground truth with instance ids:
CLEAR MOT counters per recall level and AMOTA / AMOTP (``cmt_mot_eval_*``, csrc/moteval.hip).

``IouDetectionEvaluator`` is the same collector scored by overlap (``cmt_det_eval_match_iou``: the largest BEV or 3D
IoU above a threshold, KITTI / VOC style) with the all-point and 40-point APs of ``cmt_det_eval_ap_interp`` next to the
101-point one.
"""
import math
from dataclasses import dataclass
from typing import Optional, Sequence

import numpy as np
import torch

from ... import native_eval as NE

__all__ = ["DetEvalConfig", "tumtraf_eval_config", "nuscenes_eval_config", "DetectionEvaluator", "summarize", "TUMTRAF_CLASSES",
           "TP_METRICS", "ERR_NAME_MAPPING", "IouEvalConfig", "tumtraf_iou_config", "IouDetectionEvaluator", "summarize_iou",
           "NO_RANGE", "MotEvalConfig", "tumtraf_mot_config", "nuscenes_mot_config", "summarize_mot", "TrackingEvaluator"]

TUMTRAF_CLASSES = ("CAR", "TRAILER", "TRUCK", "VAN", "PEDESTRIAN", "BUS", "MOTORCYCLE", "BICYCLE", "EMERGENCY_VEHICLE")
_TUMTRAF_RANGE = {"CAR": 50, "TRUCK": 50, "BUS": 50, "TRAILER": 50, "VAN": 50, "EMERGENCY_VEHICLE": 50,
                  "PEDESTRIAN": 40, "MOTORCYCLE": 40, "BICYCLE": 40}
TP_METRICS = ("trans_err", "scale_err", "orient_err", "vel_err")   # the reference's order in its dictionaries
ERR_NAME_MAPPING = {"trans_err": "mATE", "scale_err": "mASE", "orient_err": "mAOE", "vel_err": "mAVE"}
CURVE_NAMES = ("recall", "precision", "confidence") + NE.ERR_NAMES


@dataclass
class DetEvalConfig:
    """The evaluation constants.  ``class_range`` and ``yaw_period`` follow ``class_names``; ``gt_velocity_zero``
    replaces the ground truth's velocity by zero, as the reference's load_gt does."""
    class_names: Sequence[str]
    class_range: Sequence[float]
    yaw_period: Sequence[float]
    dist_ths: Sequence[float] = (0.5, 1.0, 2.0, 4.0)
    dist_th_tp: float = 2.0
    min_recall: float = 0.1
    min_precision: float = 0.1
    mean_ap_weight: float = 5.0
    max_boxes_per_sample: int = 500
    gt_velocity_zero: bool = False

    def __post_init__(self):
        self.class_names = tuple(self.class_names)
        if len(self.class_names) != len(tuple(self.class_range)):
            raise ValueError(f"{len(self.class_names)} class names but {len(tuple(self.class_range))} class ranges")
        NE.check_config(self.class_range, self.yaw_period, self.dist_ths, self.dist_th_tp,
                        self.min_recall, self.min_precision)
        if not 1 <= int(self.max_boxes_per_sample) <= NE.MAX_PER_SAMPLE:
            raise ValueError(f"max_boxes_per_sample must be in [1, {NE.MAX_PER_SAMPLE}], got {self.max_boxes_per_sample}")
        if not math.isfinite(self.mean_ap_weight) or self.mean_ap_weight < 0:
            raise ValueError(f"mean_ap_weight must be finite and >= 0, got {self.mean_ap_weight}")


def tumtraf_eval_config(class_names=TUMTRAF_CLASSES):
    """The reference's A9 / TUMTraf constants: class ranges 50 / 40 m, thresholds 0.5 / 1 / 2 / 4 m, TP errors at
    2 m, min recall = min precision = 0.1, mAP weight 5, at most 500 boxes per sample, period 2 pi for every class
    (none is called 'barrier'), ground-truth velocity zero."""
    names = tuple(class_names)
    unknown = [n for n in names if n not in _TUMTRAF_RANGE]
    if unknown:
        raise ValueError(f"no TUMTraf class range for {unknown}")
    return DetEvalConfig(class_names=names, class_range=[float(_TUMTRAF_RANGE[n]) for n in names],
                         yaw_period=[2 * math.pi] * len(names), gt_velocity_zero=True)


# nuScenes detection_cvpr_2019 class ranges (the devkit's public configuration file)
_NUSCENES_RANGE = {"car": 50, "truck": 50, "bus": 50, "trailer": 50, "construction_vehicle": 50, "pedestrian": 40,
                   "motorcycle": 40, "bicycle": 40, "traffic_cone": 30, "barrier": 30}


def nuscenes_eval_config(class_names):
    """The nuScenes detection constants: class ranges 50 / 40 / 30 m, the same thresholds, and a barrier's
    orientation known up to pi only.  The attribute error and the per-class ignored errors of the devkit are not
    part of this evaluator."""
    names = tuple(class_names)
    unknown = [n for n in names if n not in _NUSCENES_RANGE]
    if unknown:
        raise ValueError(f"no nuScenes class range for {unknown}")
    return DetEvalConfig(class_names=names, class_range=[float(_NUSCENES_RANGE[n]) for n in names],
                         yaw_period=[math.pi if n == "barrier" else 2 * math.pi for n in names])


def summarize(cfg, ap, tp_err):
    """The reference's metrics_summary from ap [C, T] and tp_err [C, 4] (columns trans, vel, scale, orient), in
    float64 on the host."""
    ap = np.asarray(ap, dtype=np.float64)
    tp_err = np.asarray(tp_err, dtype=np.float64)
    ths = [float(t) for t in cfg.dist_ths]
    col = {n: i for i, n in enumerate(NE.ERR_NAMES)}
    label_aps = {n: {t: float(ap[c, k]) for k, t in enumerate(ths)} for c, n in enumerate(cfg.class_names)}
    label_tp = {n: {m: float(tp_err[c, col[m]]) for m in TP_METRICS} for c, n in enumerate(cfg.class_names)}
    mean_dist_aps = {n: float(np.mean(list(d.values()))) for n, d in label_aps.items()}
    mean_ap = float(np.mean(list(mean_dist_aps.values())))
    tp_errors = {m: float(np.nanmean([label_tp[n][m] for n in cfg.class_names])) for m in TP_METRICS}
    tp_scores = {m: max(0.0, 1.0 - tp_errors[m]) for m in TP_METRICS}
    nd = float(cfg.mean_ap_weight * mean_ap + np.sum(list(tp_scores.values())))
    nd = nd / float(cfg.mean_ap_weight + len(tp_scores))
    return dict(label_aps=label_aps, mean_dist_aps=mean_dist_aps, mean_ap=mean_ap, label_tp_errors=label_tp,
                tp_errors=tp_errors, tp_scores=tp_scores, nd_score=nd)


class DetectionEvaluator:
    """Collects detections and ground truth frame by frame on the device and scores them.

    ``capacity_frames`` frames of at most ``cfg.max_boxes_per_sample`` predictions fit; the prediction buffers are
    allocated once, ``add`` copies into them on the device and reads nothing back."""

    config_type = DetEvalConfig

    def __init__(self, cfg, capacity_frames: int, device):
        if not isinstance(cfg, self.config_type):
            raise ValueError(f"cfg must be a {self.config_type.__name__}")
        if not 1 <= int(capacity_frames) <= NE.MAX_SAMPLES:
            raise ValueError(f"capacity_frames must be in [1, 2^24], got {capacity_frames}")
        self.cfg = cfg
        self.capacity_frames = int(capacity_frames)
        self.device = torch.device(device)
        rows = self.capacity_frames * int(cfg.max_boxes_per_sample)
        if rows >= 2 ** 31:
            raise ValueError("capacity_frames * max_boxes_per_sample must be below 2^31")
        self._rows = rows
        self._buf = None
        self.reset()

    def reset(self):
        self._frames = 0
        self._n = 0
        self._gt = []          # (boxes, labels, samples, num_pts) per frame
        self._gt_cat = None    # their concatenation, built by the first run after an add
        self._result = None

    def _alloc(self):
        if self._buf is None:
            d, n = self.device, self._rows
            self._buf = dict(box=torch.empty((n, 9), dtype=torch.float32, device=d),
                             score=torch.empty(n, dtype=torch.float32, device=d),
                             label=torch.empty(n, dtype=torch.int32, device=d),
                             sample=torch.empty(n, dtype=torch.int32, device=d))

    def add(self, boxes, scores, labels, count=None, gt_boxes=None, gt_labels=None, gt_num_pts=None):
        """One or more frames.  ``boxes`` [B, max_num, 9] / ``scores`` / ``labels`` [B, max_num] with the device
        ``count`` [B] of ``box_decode``, or the ``get_bboxes`` tuple of one frame ([n, 9], [n], [n], count None).
        ``gt_boxes`` / ``gt_labels``: one tensor per frame ([g, 9] and [g]; a bare tensor for one frame),
        ``gt_num_pts`` likewise or None (unknown: every box counts)."""
        if not (torch.is_tensor(boxes) and torch.is_tensor(scores) and torch.is_tensor(labels)):
            raise ValueError("boxes, scores and labels must be tensors")
        if boxes.dim() == 2:
            boxes, scores, labels = boxes[None], scores[None], labels[None]
        if boxes.dim() != 3 or boxes.shape[-1] != 9 or tuple(scores.shape) != tuple(boxes.shape[:2]) or \
                tuple(labels.shape) != tuple(boxes.shape[:2]):
            raise ValueError(f"boxes must be [B, n, 9] with scores and labels [B, n], got {tuple(boxes.shape)}, "
                             f"{tuple(scores.shape)}, {tuple(labels.shape)}")
        if boxes.dtype != torch.float32 or scores.dtype != torch.float32:
            raise ValueError("boxes and scores must be fp32")
        if labels.dtype not in (torch.int32, torch.int64):
            raise ValueError("labels must be int32 or int64")
        B, M = int(boxes.shape[0]), int(boxes.shape[1])
        if M > int(self.cfg.max_boxes_per_sample):
            raise ValueError(f"only <= {self.cfg.max_boxes_per_sample} boxes per sample allowed, got {M}")
        if count is not None and (not torch.is_tensor(count) or count.dtype != torch.int32 or count.numel() != B):
            raise ValueError(f"count must be int32 [{B}]")
        if gt_boxes is None or gt_labels is None:
            raise ValueError("gt_boxes and gt_labels are required")
        if torch.is_tensor(gt_boxes):
            gt_boxes, gt_labels = [gt_boxes], [gt_labels]
            gt_num_pts = None if gt_num_pts is None else [gt_num_pts]
        gt_boxes, gt_labels = list(gt_boxes), list(gt_labels)
        gt_num_pts = [None] * B if gt_num_pts is None else list(gt_num_pts)
        if not len(gt_boxes) == len(gt_labels) == len(gt_num_pts) == B:
            raise ValueError(f"{B} frames of predictions but {len(gt_boxes)} / {len(gt_labels)} / {len(gt_num_pts)} "
                             "of ground truth")
        for b, l, q in zip(gt_boxes, gt_labels, gt_num_pts):
            if not torch.is_tensor(b) or b.dim() != 2 or b.shape[1] != 9 or b.dtype != torch.float32:
                raise ValueError("every gt_boxes entry must be fp32 [g, 9]")
            if not torch.is_tensor(l) or tuple(l.shape) != (b.shape[0],) or l.dtype not in (torch.int32, torch.int64):
                raise ValueError("every gt_labels entry must be int [g]")
            if q is not None and (not torch.is_tensor(q) or tuple(q.shape) != (b.shape[0],) or
                                  q.dtype not in (torch.int32, torch.int64)):
                raise ValueError("every gt_num_pts entry must be int [g] or None")
        if self._frames + B > self.capacity_frames:
            raise ValueError(f"capacity of {self.capacity_frames} frames exceeded")
        tensors = [boxes, scores, labels] + gt_boxes + gt_labels + [q for q in gt_num_pts if q is not None]
        if count is not None:
            tensors.append(count)
        if any(not t.is_cuda for t in tensors):
            raise ValueError("the evaluator needs its tensors on a HIP device (no CPU path)")
        self._alloc()
        dev = self.device
        lab = labels.to(device=dev, dtype=torch.int32)
        if count is not None:   # rows at or beyond a frame's count do not exist: label -1
            live = torch.arange(M, device=dev, dtype=torch.int32)[None, :] < count.to(dev).reshape(B, 1)
            lab = torch.where(live, lab, torch.full_like(lab, -1))
        n0, n1 = self._n, self._n + B * M
        self._buf["box"][n0:n1].copy_(boxes.reshape(B * M, 9))
        self._buf["score"][n0:n1].copy_(scores.reshape(B * M))
        self._buf["label"][n0:n1].copy_(lab.reshape(B * M))
        frame = torch.arange(self._frames, self._frames + B, device=dev, dtype=torch.int32)
        self._buf["sample"][n0:n1].copy_(frame[:, None].expand(B, M).reshape(B * M))
        for i, (b, l, q) in enumerate(zip(gt_boxes, gt_labels, gt_num_pts)):
            g = int(b.shape[0])
            b = b.to(dev)
            if self.cfg.gt_velocity_zero:
                b = b.clone()
                b[:, 7:9] = 0
            num = torch.full((g,), -1, dtype=torch.int32, device=dev) if q is None else q.to(device=dev, dtype=torch.int32)
            self._gt.append((b.contiguous(), l.to(device=dev, dtype=torch.int32),
                             torch.full((g,), self._frames + i, dtype=torch.int32, device=dev), num))
        self._n, self._frames = n1, self._frames + B
        self._result = self._gt_cat = None

    # ---- results -------------------------------------------------------------------------------------

    def run(self, events=None):
        """sort -> match -> curves on the device -> the dict of device tensors of ``native_eval.det_eval``"""
        cfg = self.cfg
        self._result = NE.det_eval(*self._rows_on_device(), num_samples=self._frames, class_range=cfg.class_range,
                                   yaw_period=cfg.yaw_period, dist_ths=cfg.dist_ths, dist_th_tp=cfg.dist_th_tp,
                                   min_recall=cfg.min_recall, min_precision=cfg.min_precision, events=events)
        return self._result

    def _rows_on_device(self):
        """the eight tensors of ``native_eval.det_eval``: the filled prediction rows and the concatenated ground truth"""
        if self._frames == 0:
            raise ValueError("no frame was added")
        if self._gt_cat is None:
            self._gt_cat = tuple(torch.cat([g[k] for g in self._gt]).contiguous() for k in range(4))
        n, buf = self._n, self._buf
        return (buf["box"][:n], buf["score"][:n], buf["label"][:n], buf["sample"][:n]) + self._gt_cat

    def _thresholds(self):
        return self.cfg.dist_ths

    def compute(self):
        """The reference's metrics_summary: label_aps, mean_dist_aps, mean_ap, label_tp_errors, tp_errors,
        tp_scores, nd_score."""
        res = self.run()
        return summarize(self.cfg, res["ap"].cpu().numpy(), res["tp_err"].cpu().numpy())

    def detail(self):
        """The ``object/...`` dictionary of the reference's _evaluate_single (values rounded to four decimals,
        nds and map as they are)."""
        m = self.compute() if self._result is None else summarize(self.cfg, self._result["ap"].cpu().numpy(),
                                                                   self._result["tp_err"].cpu().numpy())
        detail = dict()
        for name in self.cfg.class_names:
            for k, v in m["label_aps"][name].items():
                detail["object/{}_ap_dist_{}".format(name, k)] = float("{:.4f}".format(v))
            for k, v in m["label_tp_errors"][name].items():
                detail["object/{}_{}".format(name, k)] = float("{:.4f}".format(v))
            for k, v in m["tp_errors"].items():
                detail["object/{}".format(ERR_NAME_MAPPING[k])] = float("{:.4f}".format(v))
        detail["object/nds"] = m["nd_score"]
        detail["object/map"] = m["mean_ap"]
        return detail

    def metric_data(self):
        """The seven 101-point curves per (class, threshold), keyed ``'<class>:<threshold>'`` as the reference's
        metrics_details.json."""
        res = self.run() if self._result is None else self._result
        md = res["md"].cpu().numpy()
        out = dict()
        for c, name in enumerate(self.cfg.class_names):
            for k, th in enumerate(self._thresholds()):
                out[name + ":" + str(float(th))] = {cn: md[c, k, i].tolist() for i, cn in enumerate(CURVE_NAMES)}
        return out


# ---- IoU-matched AP -------------------------------------------------------------------------------------------
NO_RANGE = 1.0e9   # class_range=None: no range filter (the contract wants a finite range; non-finite centres still drop)


@dataclass
class IouEvalConfig:
    """The constants of the IoU-matched evaluation (cmt_det_eval_match_iou in include/cmt_hip.h): a prediction
    matches the unclaimed ground truth of largest BEV or 3D IoU above ``iou_ths[t]``.  ``class_range`` None: no
    range filter; ``yaw_period`` None: 2 pi for every class."""
    class_names: Sequence[str]
    iou_ths: Sequence[float] = (0.1, 0.25, 0.5, 0.7)
    iou_th_tp: float = 0.5
    mode: str = "3d"
    z_origin: float = 0.5
    class_range: Optional[Sequence[float]] = None
    yaw_period: Optional[Sequence[float]] = None
    min_recall: float = 0.1
    min_precision: float = 0.1
    max_boxes_per_sample: int = 500
    gt_velocity_zero: bool = False

    def __post_init__(self):
        self.class_names = tuple(self.class_names)
        C = len(self.class_names)
        self.class_range = [NO_RANGE] * C if self.class_range is None else [float(v) for v in self.class_range]
        self.yaw_period = [2 * math.pi] * C if self.yaw_period is None else [float(v) for v in self.yaw_period]
        if len(self.class_range) != C:
            raise ValueError(f"{C} class names but {len(self.class_range)} class ranges")
        self.iou_ths = tuple(float(t) for t in self.iou_ths)
        NE.check_iou_config(self.class_range, self.yaw_period, self.iou_ths, self.iou_th_tp, self.mode, self.z_origin,
                            self.min_recall, self.min_precision)
        if not 1 <= int(self.max_boxes_per_sample) <= NE.MAX_PER_SAMPLE:
            raise ValueError(f"max_boxes_per_sample must be in [1, {NE.MAX_PER_SAMPLE}], got {self.max_boxes_per_sample}")


def tumtraf_iou_config(class_names=TUMTRAF_CLASSES, mode="3d"):
    """Plain defaults for the TUMTraf classes: 3D IoU thresholds 0.1 / 0.25 / 0.5 / 0.7, TP errors and the mean
    matched IoU at 0.5, boxes with the centre at half height, no range filter, ground-truth velocity zero.  These are
    settings of this package: they are not taken from, and have not been compared with, the TUMTraf devkit."""
    return IouEvalConfig(class_names=tuple(class_names), mode=mode, gt_velocity_zero=True)


def summarize_iou(cfg, ap, ap_interp, tp_err, mean_iou):
    """The metrics dictionary from ap [C, T] (the 101-point AP of the reused curves), ap_interp [C, T, 2] (all-point,
    40-point), tp_err [C, 4] (columns trans, vel, scale, orient; at ``iou_th_tp``) and the mean matched IoU [C] (NaN for
    a class without a match), in float64 on the host."""
    ap, ai = np.asarray(ap, dtype=np.float64), np.asarray(ap_interp, dtype=np.float64)
    tp_err, mean_iou = np.asarray(tp_err, dtype=np.float64), np.asarray(mean_iou, dtype=np.float64)
    col = {n: i for i, n in enumerate(NE.ERR_NAMES)}
    label_aps = {n: {t: dict(ap_all=float(ai[c, k, 0]), ap_r40=float(ai[c, k, 1]), ap_101=float(ap[c, k]))
                     for k, t in enumerate(cfg.iou_ths)} for c, n in enumerate(cfg.class_names)}
    mean_aps = {n: {m: float(np.mean([d[t][m] for t in cfg.iou_ths])) for m in ("ap_all", "ap_r40", "ap_101")}
                for n, d in label_aps.items()}
    label_tp = {n: {m: float(tp_err[c, col[m]]) for m in TP_METRICS} for c, n in enumerate(cfg.class_names)}
    out = dict(label_aps=label_aps, mean_aps=mean_aps)
    for m in ("all", "r40", "101"):
        out["map_" + m] = float(np.mean([mean_aps[n]["ap_" + m] for n in cfg.class_names]))
    out.update(label_tp_errors=label_tp,
               tp_errors={m: float(np.nanmean([label_tp[n][m] for n in cfg.class_names])) for m in TP_METRICS},
               label_mean_iou={n: float(mean_iou[c]) for c, n in enumerate(cfg.class_names)},
               iou_ths=list(cfg.iou_ths), iou_th_tp=float(cfg.iou_th_tp), mode=cfg.mode)
    return out


class IouDetectionEvaluator(DetectionEvaluator):
    """``DetectionEvaluator`` (the same ``add`` / ``reset`` and buffers) scored by overlap: per class and IoU threshold
    the all-point AP, the 40-point AP and the nuScenes-style 101-point AP, their means, the four TP errors and the
    mean matched IoU at ``cfg.iou_th_tp``."""
    config_type = IouEvalConfig

    def run(self, events=None):
        """sort -> IoU match -> curves -> interpolated APs -> the dict of ``native_eval.det_eval_iou``"""
        cfg = self.cfg
        self._result = NE.det_eval_iou(*self._rows_on_device(), num_samples=self._frames, class_range=cfg.class_range,
                                       yaw_period=cfg.yaw_period, iou_ths=cfg.iou_ths, iou_th_tp=cfg.iou_th_tp,
                                       mode=cfg.mode, z_origin=cfg.z_origin, min_recall=cfg.min_recall,
                                       min_precision=cfg.min_precision, events=events)
        return self._result

    def _thresholds(self):
        return self.cfg.iou_ths

    def _mean_matched_iou(self, res):
        """per class the mean of match_iou over the matches at iou_th_tp (float64 sums on the device; NaN: none)"""
        k = self.cfg.iou_ths.index(float(self.cfg.iou_th_tp))
        v, lab = res["match_iou"][k].double(), self._buf["label"][:self._n]
        hit = ~torch.isnan(v)
        sums = [torch.where(hit & (lab == c), v, torch.zeros_like(v)).sum() for c in range(len(self.cfg.class_names))]
        cnts = [(hit & (lab == c)).sum() for c in range(len(self.cfg.class_names))]
        s, n = torch.stack(sums).cpu().numpy(), torch.stack(cnts).cpu().numpy()
        return np.divide(s, n, out=np.full(len(s), np.nan), where=n != 0)

    def compute(self):
        res = self.run()
        return summarize_iou(self.cfg, res["ap"].cpu().numpy(), res["ap_interp"].cpu().numpy(),
                             res["tp_err"].cpu().numpy(), self._mean_matched_iou(res))

    def detail(self):
        """``object/<class>_<ap kind>_iou_<threshold>`` and the means, values rounded to four decimals"""
        m = self.compute()
        detail = dict()
        for name in self.cfg.class_names:
            for th, d in m["label_aps"][name].items():
                for k, v in d.items():
                    detail["object/{}_{}_iou_{}".format(name, k, th)] = float("{:.4f}".format(v))
        for k in ("map_all", "map_r40", "map_101"):
            detail["object/" + k] = m[k]
        return detail


# ---- tracking evaluation --------------------------------------------------------------------------------------


@dataclass
class MotEvalConfig:
    """The constants of the tracking evaluation (cmt_mot_eval_* in include/cmt_hip.h).  ``class_range`` and ``dist_th``
    (metres; one number for all classes or one per class) follow ``class_names``; ``num_thresholds`` recall levels
    from ``min_recall`` to 1; ``max_gt_tracks`` bounds the instance ids of a scene; at most ``max_boxes_per_frame``
    prediction rows per frame."""
    class_names: Sequence[str]
    class_range: Optional[Sequence[float]] = None
    dist_th: object = 2.0
    num_thresholds: int = 40
    min_recall: float = 0.1
    max_gt_tracks: int = 1024
    max_boxes_per_frame: int = 500

    def __post_init__(self):
        self.class_names = tuple(self.class_names)
        C = len(self.class_names)
        self.class_range = [NO_RANGE] * C if self.class_range is None else [float(v) for v in self.class_range]
        self.dist_th = [float(v) for v in self.dist_th] if isinstance(self.dist_th, (list, tuple)) else [float(self.dist_th)] * C
        if len(self.class_range) != C:
            raise ValueError(f"{C} class names but {len(self.class_range)} class ranges")
        NE.check_mot_config(self.class_range, self.dist_th, self.recall_levels(), self.max_gt_tracks)
        if int(self.max_boxes_per_frame) < 1:
            raise ValueError(f"max_boxes_per_frame must be at least 1, got {self.max_boxes_per_frame}")

    def recall_levels(self):
        return NE.mot_recall_levels(self.num_thresholds, self.min_recall)


def tumtraf_mot_config(class_names=TUMTRAF_CLASSES, **overrides):
    """The TUMTraf classes with the detection evaluator's class ranges (50 / 40 m), a 2 m match distance and 40 recall
    levels from 0.1.  These are settings of this package: they are not taken from, and have not been compared with,
    a TUMTraf tracking devkit."""
    names = tuple(class_names)
    unknown = [n for n in names if n not in _TUMTRAF_RANGE]
    if unknown:
        raise ValueError(f"no TUMTraf class range for {unknown}")
    return MotEvalConfig(class_names=names, class_range=[float(_TUMTRAF_RANGE[n]) for n in names], **overrides)


# nuScenes tracking_nips_2019 (the devkit's public configuration file): seven classes, 2 m, 40 levels from 0.1
NUSCENES_TRACKING_CLASSES = ("bicycle", "bus", "car", "motorcycle", "pedestrian", "trailer", "truck")
_NUSCENES_TRACKING_RANGE = {"car": 50, "truck": 50, "bus": 50, "trailer": 50, "pedestrian": 40, "motorcycle": 40,
                            "bicycle": 40}


def nuscenes_mot_config(class_names=NUSCENES_TRACKING_CLASSES, **overrides):
    """The nuScenes tracking constants: class ranges 50 / 40 m, match distance 2 m, 40 recall levels from 0.1.  The
    contract's stated deviations from the devkit apply (order-statistic thresholds, no track interpolation)."""
    names = tuple(class_names)
    unknown = [n for n in names if n not in _NUSCENES_TRACKING_RANGE]
    if unknown:
        raise ValueError(f"no nuScenes tracking class range for {unknown}")
    return MotEvalConfig(class_names=names, class_range=[float(_NUSCENES_TRACKING_RANGE[n]) for n in names], **overrides)


def summarize_mot(cfg, class_sum, npos):
    """The metrics dictionary from class_sum [C, 12] (native_eval.MOT_CLASS_SUM) and npos [C], in float64 on the
    host.  A class without ground truth is left out of the means (its entries are NaN), as the devkit does."""
    cs, npos = np.asarray(class_sum, dtype=np.float64), np.asarray(npos)
    col = {n: i for i, n in enumerate(NE.MOT_CLASS_SUM)}
    per_class = dict()
    for c, name in enumerate(cfg.class_names):
        d = {k: float(cs[c, col[k]]) for k in ("amota", "amotp", "mota", "motp", "recall")}
        for k in ("tp", "fp", "fn", "ids", "frag"):
            v = cs[c, col[k]]
            d[k] = None if np.isnan(v) else int(v)
        d["threshold"], d["best_slot"], d["npos"] = float(cs[c, col["thr"]]), int(cs[c, col["best"]]), int(npos[c])
        per_class[name] = d
    used = [n for c, n in enumerate(cfg.class_names) if npos[c] > 0]

    def mean(key):
        vals = [per_class[n][key] for n in used if not math.isnan(per_class[n][key])]
        return float(np.mean(vals)) if vals else float("nan")

    out = dict(label_metrics=per_class, classes_evaluated=used)
    out.update({k: mean(k) for k in ("amota", "amotp", "mota", "motp", "recall")})
    out.update({k: int(sum(per_class[n][k] or 0 for n in used)) for k in ("tp", "fp", "fn", "ids", "frag")})
    return out


class TrackingEvaluator:
    """Collects tracked boxes and ground truth with instance ids frame by frame on the device and scores them.

    ``capacity_frames`` frames of at most ``cfg.max_boxes_per_frame`` prediction rows fit; the prediction buffers are
    allocated once.  ``add`` copies on the device and reads nothing back; the (scene, step) table is kept on the host,
    which knows it without asking the device.  ``compute`` / ``run`` read one pair of counts back (the longest
    frame) to size the matrices, then the result."""

    def __init__(self, cfg, capacity_frames: int, device):
        if not isinstance(cfg, MotEvalConfig):
            raise ValueError("cfg must be a MotEvalConfig")
        if not 1 <= int(capacity_frames) <= NE.MOT_MAX_SCENE_STEPS:
            raise ValueError(f"capacity_frames must be in [1, 2^24], got {capacity_frames}")
        self.cfg = cfg
        self.capacity_frames = int(capacity_frames)
        self.device = torch.device(device)
        self._rows = self.capacity_frames * int(cfg.max_boxes_per_frame)
        if self._rows >= 2 ** 31:
            raise ValueError("capacity_frames * max_boxes_per_frame must be below 2^31")
        self._buf = None
        self.reset()

    def reset(self):
        self._n = 0
        self._table = []       # (scene, step) per frame
        self._next_step = {}   # scene -> the step of its next frame
        self._gt = []          # (boxes, labels, frames, ids) per frame
        self._result = None

    def add(self, boxes, scores, labels, track_ids, count=None, *, gt_boxes, gt_labels, gt_ids, scene, step=None):
        """One frame.  ``boxes`` fp32 [n, >= 2] (x, y in front, as the decoder's nine columns have them), ``scores``
        fp32 [n], ``labels`` int [n], ``track_ids`` int32 [n]: ``Tracker.step``'s ``det_track`` as it is (-1: the row
        belongs to no track), ``count``: None or the device int32 of the valid rows.  ``gt_boxes`` fp32 [g, >= 2],
        ``gt_labels`` int [g], ``gt_ids`` int [g], the objects' instance ids inside the scene, below
        ``cfg.max_gt_tracks``.  ``scene``: the frame's scene (an int >= 0); ``step``: its position there (default: one
        after the scene's latest).  A (scene, step) can be added once."""
        n = self._check_rows(boxes, "boxes", scores=scores, labels=labels, track_ids=track_ids)
        g = self._check_rows(gt_boxes, "gt_boxes", gt_labels=gt_labels, gt_ids=gt_ids)
        if scores.dtype != torch.float32 or track_ids.dtype != torch.int32:
            raise ValueError("scores must be fp32 and track_ids int32")
        if n > int(self.cfg.max_boxes_per_frame):
            raise ValueError(f"only <= {self.cfg.max_boxes_per_frame} boxes per frame allowed, got {n}")
        if count is not None and (not torch.is_tensor(count) or count.dtype != torch.int32 or count.numel() != 1):
            raise ValueError("count must be one int32 on the device or None")
        scene = int(scene)
        step = self._next_step.get(scene, 0) if step is None else int(step)
        if scene < 0 or step < 0:
            raise ValueError(f"scene and step must not be negative, got {scene} and {step}")
        if (scene, step) in self._table:
            raise ValueError(f"step {step} of scene {scene} was added before")
        if len(self._table) >= self.capacity_frames:
            raise ValueError(f"capacity of {self.capacity_frames} frames exceeded")
        tensors = [boxes, scores, labels, track_ids, gt_boxes, gt_labels, gt_ids] + ([] if count is None else [count])
        if any(not t.is_cuda for t in tensors):
            raise ValueError("the evaluator needs its tensors on a HIP device (no CPU path)")
        dev, f = self.device, len(self._table)
        if self._buf is None:
            r = self._rows
            self._buf = dict(box=torch.empty((r, 2), dtype=torch.float32, device=dev),
                             score=torch.empty(r, dtype=torch.float32, device=dev),
                             label=torch.empty(r, dtype=torch.int32, device=dev),
                             track=torch.empty(r, dtype=torch.int32, device=dev),
                             frame=torch.empty(r, dtype=torch.int32, device=dev))
        lab = labels.to(device=dev, dtype=torch.int32)
        if count is not None:   # rows at or beyond the count do not exist: label -1
            live = torch.arange(n, device=dev, dtype=torch.int32) < count.to(dev).reshape(1)
            lab = torch.where(live, lab, torch.full_like(lab, -1))
        n0, n1 = self._n, self._n + n
        self._buf["box"][n0:n1].copy_(boxes[:, :2])
        self._buf["score"][n0:n1].copy_(scores)
        self._buf["label"][n0:n1].copy_(lab)
        self._buf["track"][n0:n1].copy_(track_ids)
        self._buf["frame"][n0:n1].fill_(f)
        self._gt.append((gt_boxes[:, :2].to(device=dev, copy=True), gt_labels.to(device=dev, dtype=torch.int32),
                         torch.full((g,), f, dtype=torch.int32, device=dev), gt_ids.to(device=dev, dtype=torch.int32)))
        self._table.append((scene, step))
        self._next_step[scene] = max(self._next_step.get(scene, 0), step + 1)
        self._n, self._result = n1, None

    @staticmethod
    def _check_rows(box, name, **cols):
        if not torch.is_tensor(box) or box.dim() != 2 or box.shape[1] < 2 or box.dtype != torch.float32:
            raise ValueError(f"{name} must be fp32 [n, >= 2]")
        n = int(box.shape[0])
        for k, t in cols.items():
            if not torch.is_tensor(t) or tuple(t.shape) != (n,):
                raise ValueError(f"{k} must be a tensor of shape [{n}]")
            if k in ("labels", "gt_labels", "gt_ids") and t.dtype not in (torch.int32, torch.int64):
                raise ValueError(f"{k} must be int32 or int64")
        return n

    def run(self, events=None, workspace_bytes=NE.MOT_WORKSPACE, alloc=None):
        """the evaluation on the device -> the dict of device tensors of ``native_eval.mot_eval``"""
        if not self._table:
            raise ValueError("no frame was added")
        cfg, buf, n = self.cfg, self._buf, self._n
        gt = tuple(torch.cat([g[k] for g in self._gt]).contiguous() for k in range(4))
        table = torch.tensor(self._table, dtype=torch.int32).reshape(-1, 2).to(self.device)
        self._result = NE.mot_eval(buf["box"][:n], buf["score"][:n], buf["label"][:n], buf["track"][:n], buf["frame"][:n],
                                   gt[0], gt[1], gt[2], gt[3], table,
                                   num_scenes=max(s for s, _ in self._table) + 1,
                                   max_steps=max(t for _, t in self._table) + 1, class_range=cfg.class_range,
                                   dist_th=cfg.dist_th, recall=cfg.recall_levels(), max_gt_tracks=cfg.max_gt_tracks,
                                   workspace_bytes=workspace_bytes, alloc=alloc, events=events)
        return self._result

    def compute(self):
        """AMOTA / AMOTP and, at the recall level of highest MOTA, MOTA / MOTP / recall / TP / FP / FN / IDS / FRAG per
        class, with the means over the classes that have ground truth (``summarize_mot``)."""
        res = self.run()
        return summarize_mot(self.cfg, res["class_sum"].cpu().numpy(), res["npos"].cpu().numpy())

    def detail(self):
        """``track/<class>_<metric>`` and the means, floats rounded to four decimals"""
        res = self.run() if self._result is None else self._result
        m = summarize_mot(self.cfg, res["class_sum"].cpu().numpy(), res["npos"].cpu().numpy())
        detail = dict()
        for name, d in m["label_metrics"].items():
            for k in ("amota", "amotp", "mota", "motp", "recall"):
                detail["track/{}_{}".format(name, k)] = float("{:.4f}".format(d[k]))
            for k in ("ids", "frag", "tp", "fp", "fn"):
                detail["track/{}_{}".format(name, k)] = d[k]
        for k in ("amota", "amotp", "mota", "motp", "recall"):
            detail["track/" + k] = m[k]
        for k in ("ids", "frag"):
            detail["track/" + k] = m[k]
        return detail
