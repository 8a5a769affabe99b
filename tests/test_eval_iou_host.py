"""IoU-matched evaluation without a device: hand-computed answers for tests/_eval_iou_ref.py (the numpy restatement
of cmt_det_eval_match_iou / cmt_det_eval_ap_interp), the argument checks, and the scenes of the device test with
their decision margins.

The device's float32 IoU is within the project's bound of float64 (tests/test_gpu_iou.py: 8 x measure_e32(), below
6.7e-6) but not bit-equal to numpy's.  The device test still compares tp and match_gt exactly, so no scene may decide
anything on a rounding: for every committed scene and configuration, in float64, every |iou - threshold| and every
gap between the best and the second-best unclaimed candidate of a greedy step that ends in a match is at least 1e-4
(a gap of exactly 0 between identical ground-truth boxes is decided by the index and is allowed)."""
import ctypes
import functools
import importlib.util
import math
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _eval_iou_ref as R  # noqa: E402
import _iou_ref as I  # noqa: E402

from conftest import PKG  # noqa: E402

TWO_PI = 2 * math.pi
MARGIN = 1e-4
THS4 = (0.1, 0.25, 0.5, 0.7)
THS8 = (0.05, 0.1, 0.2, 0.3, 0.4, 0.5, 0.6, 0.7)
TIES = [k / 64.0 for k in range(8, 24)]


def _box(x, y, dims=(2, 2, 2), yaw=0.0, z=0.0, vel=(0.0, 0.0)):
    return [x, y, z] + list(dims) + [yaw] + list(vel)


def _one_class(gt, pred, scores, ths, mode="3d", **kw):
    n, g = len(pred), len(gt)
    return R.evaluate(pred, scores, [0] * n, [0] * n, gt, [0] * g, [0] * g, [-1] * g, num_samples=1,
                      class_range=[50.0], yaw_period=[TWO_PI], iou_ths=ths, iou_th_tp=ths[0], mode=mode, **kw)


# ---- hand-computed answers -------------------------------------------------------------------------------------
def test_identical_nested_touching_and_quarter_turn():
    # identical: iou 1, a match at every threshold below 1
    out = _one_class([_box(3, 4, (4, 2, 1.5), 0.7)], [_box(3, 4, (4, 2, 1.5), 0.7)], [0.5], [0.0, 0.5, 0.99])
    assert out["tp"][:, 0].tolist() == [1, 1, 1] and abs(float(out["match_iou"][0, 0]) - 1.0) <= 1e-6
    # nested, axis-aligned, same centre: 2 x 1 x 1 inside 4 x 2 x 2 -> 3D 2 / 16, BEV 2 / 8
    gt, pred = [_box(0, 0, (4, 2, 2))], [_box(0, 0, (2, 1, 1))]
    out = _one_class(gt, pred, [0.5], [0.1, 0.2])
    assert out["match_iou"][0, 0] == np.float32(0.125) and out["tp"][:, 0].tolist() == [1, 0]
    assert math.isnan(out["match_iou"][1, 0]) and out["match_gt"][:, 0].tolist() == [0, -1]
    out = _one_class(gt, pred, [0.5], [0.2, 0.25], mode="bev")
    assert out["match_iou"][0, 0] == np.float32(0.25) and out["tp"][:, 0].tolist() == [1, 0]   # 0.25 is not above itself
    # z_origin 0: z is the bottom, so the same rows overlap over the lower box's height only: still 2 / 16
    assert _one_class(gt, pred, [0.5], [0.1], z_origin=0.0)["match_iou"][0, 0] == np.float32(0.125)
    # touching along x: iou 0, hence no tp even at threshold 0
    out = _one_class([_box(0, 0)], [_box(2, 0)], [0.5], [0.0])
    assert out["tp"].sum() == 0 and out["match_gt"][0, 0] == -1 and out["pairs"][(0, 0)] == 0
    # a quarter-turned square is itself; a quarter-turned 4 x 2 rectangle keeps the 2 x 2 middle: 4 / (8 + 8 - 4)
    out = _one_class([_box(1, 1, (2, 2, 2))], [_box(1, 1, (2, 2, 2), yaw=math.pi / 2)], [0.5], [0.5], mode="bev")
    assert abs(float(out["match_iou"][0, 0]) - 1.0) <= 1e-6
    out = _one_class([_box(1, 1, (4, 2, 2))], [_box(1, 1, (4, 2, 2), yaw=math.pi / 2)], [0.5], [0.3], mode="bev")
    assert abs(float(out["match_iou"][0, 0]) - 1.0 / 3.0) <= 1e-6 and out["tp"][0, 0] == 1


def test_duplicates_and_identical_ground_truth():
    # a duplicate prediction: the ground truth is taken, the second goes to the next best or becomes a false positive
    gt = [_box(0, 0, (4, 2, 2)), _box(1, 0, (4, 2, 2))]          # BEV with the prediction at 0: 1 and 6 / 10
    pred = [_box(0, 0, (4, 2, 2)), _box(0, 0, (4, 2, 2))]
    out = _one_class(gt, pred, [0.9, 0.8], [0.5, 0.7], mode="bev")
    assert out["match_gt"][0].tolist() == [0, 1] and out["match_gt"][1].tolist() == [0, -1]
    assert out["match_iou"][0, 1] == np.float32(0.6) and out["tp"].tolist() == [[1, 1], [1, 0]]
    # equal scores: the later row is visited first
    out = _one_class(gt, pred, [0.8, 0.8], [0.7], mode="bev")
    assert out["match_gt"][0].tolist() == [-1, 0]
    # two identical ground truths: the lowest annotation index wins, the next prediction takes the other
    gt = [_box(5, 5), _box(5, 5)]
    out = _one_class(gt, [_box(5, 5), _box(5.1, 5)], [0.9, 0.8], [0.5])
    assert out["match_gt"][0].tolist() == [0, 1]
    # the errors of a match are the centre-distance evaluator's: err[0] is the centre distance
    assert out["err"][0, 0, 1] == pytest.approx(float(np.float32(5.1)) - 5.0, abs=1e-12) and out["err"][0, 0, 0] == 0.0


def test_envelope_and_interpolated_aps():
    """Three predictions of a class with three ground-truth boxes, tp = 1, 0, 1 in visiting order:
    ctp = 1, 1, 2; prec = 1, 1/2, 2/3; env = 1, 2/3, 2/3; the matches sit at positions 0 and 2.
    ap_all = (env[0] + env[2]) / npos = (1 + 2/3) / 3 = 5/9.
    R40: m_k = ceil(3 k / 40): 1 for k <= 13 (3 * 13 = 39), 2 for k = 14 .. 26 (3 * 26 = 78), 3 > M beyond:
    (13 * 1 + 13 * 2/3 + 14 * 0) / 40 = 13/24."""
    a, r = R.ap_interp([1, 0, 1], 3)
    assert a == pytest.approx(5.0 / 9.0, abs=1e-15) and r == pytest.approx(13.0 / 24.0, abs=1e-15)
    assert R.ap_interp([0, 0], 3) == (0.0, 0.0) and R.ap_interp([1], 0) == (0.0, 0.0) and R.ap_interp([], 2) == (0.0, 0.0)
    assert R.ap_interp([1, 1], 2) == (1.0, 1.0)
    # the same through the evaluator: the second prediction overlaps nothing, one ground truth is never found
    gt = [_box(0, 0), _box(10, 0), _box(20, 0)]
    pred = [_box(0, 0), _box(-10, 0), _box(10.2, 0)]
    out = _one_class(gt, pred, [0.9, 0.8, 0.7], [0.5])
    assert out["tp"][0].tolist() == [1, 0, 1] and out["npos"].tolist() == [3]
    assert out["ap_interp"][0, 0, 0] == pytest.approx(5.0 / 9.0, abs=1e-15)
    assert out["ap_interp"][0, 0, 1] == pytest.approx(13.0 / 24.0, abs=1e-15)
    assert out["summary"]["map_all"] == out["ap_interp"][0, 0, 0]
    assert out["mean_iou"][0] == pytest.approx((1.0 + 1.8 / 2.2) / 2, abs=1e-6)


# ---- the scenes of the device test --------------------------------------------------------------------------------
class Scene:
    """predictions and ground truth as lists of rows, in arrival / annotation order"""

    def __init__(self, seed):
        self.rng = np.random.RandomState(seed)
        self.p, self.g = [], []

    def gt(self, sample, label, box7, num_pts=-1):
        self.g.append((list(box7) + list(self.rng.normal(size=2)), label, sample, num_pts))

    def pred(self, sample, label, score, box7):
        self.p.append((list(box7) + list(self.rng.normal(size=2)), score, label, sample))

    def jitter(self, b):
        r, b = self.rng, np.array(b, np.float64)
        b[0:2] += r.uniform(-0.3, 0.3, 2)
        b[2] += r.uniform(-0.15, 0.15)
        b[3:6] *= r.uniform(0.88, 1.12, 3)
        b[6] += r.uniform(-0.12, 0.12)
        return b

    def fill(self, sample, label, n_gt, n_pred, scores=None, fp_rate=0.2):
        """n_gt objects of one (sample, class) on a 9 m grid (different objects do not touch), every seventh with an
        overlapping sibling; n_pred predictions: jittered objects drawn with replacement (so duplicates) and false
        positives somewhere on the grid"""
        r = self.rng
        side = max(1, int(math.ceil(math.sqrt(max(n_gt, n_pred, 1)))))
        mine = []
        for k in range(n_gt):
            if k % 7 == 6:
                b = np.array(mine[-1], np.float64)
                b[0:2] += r.uniform(0.5, 1.0, 2)
                b[6] += r.uniform(-0.3, 0.3)
            else:
                gx, gy = divmod(k, side)
                b = I.random_boxes(r, 1, ((gx - side / 2) * 9.0, (gy - side / 2) * 9.0), 1.0)[0].astype(np.float64)
                b[3:5] = r.uniform(1.5, 5.0), r.uniform(1.2, 2.5)
            mine.append(b)
            self.gt(sample, label, b)
        for _ in range(n_pred):
            sc = float(r.choice(scores)) if scores is not None else float(np.float32(r.uniform(0.01, 1)))
            if mine and r.rand() > fp_rate:
                b = self.jitter(mine[r.randint(len(mine))])
            else:
                b = I.random_boxes(r, 1, (0.0, 0.0), side * 4.5)[0]
            self.pred(sample, label, sc, b)

    def arrays(self, shuffle=False):
        p, g = self.p, self.g
        if shuffle:   # rows of different samples interleave; the ground truth keeps its annotation order per sample
            p = [p[i] for i in self.rng.permutation(len(p))]
            g = [g[i] for i in self.rng.permutation(len(g))]
        pb = np.array([r[0] for r in p], dtype=np.float32).reshape(-1, 9)
        gb = np.array([r[0] for r in g], dtype=np.float32).reshape(-1, 9)
        col = lambda rows, k, dt: np.array([r[k] for r in rows], dtype=dt)  # noqa: E731
        return dict(pred_boxes=pb, pred_scores=col(p, 1, np.float32), pred_labels=col(p, 2, np.int32),
                    pred_samples=col(p, 3, np.int32), gt_boxes=gb, gt_labels=col(g, 1, np.int32),
                    gt_samples=col(g, 2, np.int32), gt_num_pts=col(g, 3, np.int32))


def scene_lanes(seed):
    """ground truth per (sample, class) 64, 65, 130, 1, 0 and predictions 70, 1, 70, 0, 1: the register / chunk
    border of the lanes; 2 samples, 3 classes"""
    s = Scene(seed)
    s.fill(0, 0, 64, 70)
    s.fill(0, 1, 65, 1)
    s.fill(0, 2, 130, 70, TIES)
    s.fill(1, 0, 1, 0)
    s.fill(1, 1, 0, 1)
    return s.arrays(), 2, 3


def scene_wide(seed):
    """32 classes, 5 samples of which 1 and 3 are empty, rows interleaved across samples, equal scores, invalid boxes
    on either side, labels and samples outside their ranges, ground truth without points, a class range that drops
    far boxes"""
    s = Scene(seed)
    for smp in (0, 2, 4):
        s.fill(smp, 0, 9, 12, TIES)
        s.fill(smp, 5, 3, 4, TIES[:2])
        s.fill(smp, 31, 5, 6)
        s.fill(smp, 17, 0, 2)
        s.fill(smp, 8, 2, 0)
    base = [6.0, -3.0, 0.2, 4.0, 2.0, 1.6, 0.4]
    at = lambda dx, **kw: [base[0] + dx] + base[1:]  # noqa: E731
    # class 9 of sample 2: an invalid ground truth (dz = 0) under a prediction, an invalid prediction (NaN yaw) on a
    # valid ground truth, and an ordinary pair
    s.gt(2, 9, at(0.0)[:5] + [0.0, 0.4])
    s.pred(2, 9, 0.9, at(0.0))
    s.gt(2, 9, at(20.0))
    s.pred(2, 9, 0.8, at(20.0)[:6] + [float("nan")])
    s.gt(2, 9, at(40.0))
    s.pred(2, 9, 0.7, s.jitter(at(40.0)))
    # rows that do not exist: labels -1 and 32, sample 5, ground truth without points; a perfect prediction each
    for lab, smp, num in ((-1, 0, -1), (32, 0, -1), (9, 5, -1), (9, 4, 0)):
        s.gt(smp, lab, at(0.0), num_pts=num)
        s.pred(smp, lab, 0.95, at(0.0))
    # beyond the class range of 60 m: dropped on both sides
    s.gt(4, 31, [70.0, 0.0] + base[2:])
    s.pred(4, 31, 0.99, [70.0, 0.0] + base[2:])
    return s.arrays(shuffle=True), 5, 32


def scene_single(seed):
    """one sample, one class, one ground truth, one jittered prediction"""
    s = Scene(seed)
    s.fill(0, 0, 1, 1, fp_rate=0.0)
    return s.arrays(), 1, 1


def scene_frames(seed):
    """3 samples, 3 classes, sample-major rows with equal scores: what an evaluator collects frame by frame"""
    s = Scene(seed)
    for smp, gts in enumerate(((4, 2, 3), (0, 5, 1), (3, 3, 0))):
        for c, n in enumerate(gts):
            s.fill(smp, c, n, n + 2, TIES[:6])
    return s.arrays(), 3, 3


# name -> (scene, seed, configuration); the seeds are the first ones whose margins hold (test_decision_margins)
CASES = {
    "lanes_3d": (scene_lanes, 1, dict(iou_ths=THS4, iou_th_tp=0.5, mode="3d", z_origin=0.5)),
    "lanes_bev": (scene_lanes, 1, dict(iou_ths=THS4, iou_th_tp=0.5, mode="bev", z_origin=0.0)),
    "wide_bev": (scene_wide, 2, dict(iou_ths=THS8, iou_th_tp=0.3, mode="bev", z_origin=0.5, class_range=60.0)),
    "wide_3d": (scene_wide, 2, dict(iou_ths=THS8, iou_th_tp=0.5, mode="3d", z_origin=0.0, class_range=60.0)),
    "frames": (scene_frames, 4, dict(iou_ths=THS4, iou_th_tp=0.5, mode="3d", z_origin=0.5)),
    "single": (scene_single, 3, dict(iou_ths=(0.3,), iou_th_tp=0.3, mode="3d", z_origin=0.5)),
}


@functools.lru_cache(maxsize=None)
def inputs(name):
    """-> (arrays, S, configuration of _eval_iou_ref.evaluate / native_eval.det_eval_iou)"""
    scene, seed, kw = CASES[name]
    a, S, C = scene(seed)
    kw = dict(kw)
    rng = kw.pop("class_range", 1.0e9)
    # class 1 knows its orientation up to pi only
    per = [math.pi if c == 1 else TWO_PI for c in range(C)]
    return a, S, dict(class_range=[rng] * C, yaw_period=per, min_recall=0.1, min_precision=0.1, **kw)


@functools.lru_cache(maxsize=None)
def reference(name):
    a, S, cfg = inputs(name)
    return R.evaluate(**a, num_samples=S, **cfg)


def margins(a, S, cfg):
    """(the smallest |iou - threshold| over every pair of a kept ground truth and a kept prediction of one (sample,
    class) and every threshold, the smallest gap between the best and the second-best unclaimed candidate over the
    greedy steps that end in a match), in float64; a gap of 0 between identical ground-truth rows does not count"""
    trace = []
    out = R.evaluate(**a, num_samples=S, **cfg, dtype=np.float64, trace=trace)
    ths = [float(t) for t in cfg["iou_ths"]]
    vals = np.array(list(out["pairs"].values()), np.float64)
    m_th = min(float(np.abs(vals - t).min()) for t in ths) if vals.size else math.inf
    m_gap = math.inf
    gb = a["gt_boxes"]
    for (_, _, t, best, second, bg, sg) in trace:
        if second is None or not best > ths[t]:
            continue
        gap = float(best - second)
        if gap == 0.0 and np.array_equal(gb[bg, :7], gb[sg, :7]):
            continue
        m_gap = min(m_gap, gap)
    return m_th, m_gap


@pytest.mark.parametrize("name", sorted(CASES))
def test_decision_margins(name):
    a, S, cfg = inputs(name)
    m_th, m_gap = margins(a, S, cfg)
    print(f"{name}: threshold margin {m_th:.3e}, candidate gap {m_gap:.3e}")
    assert m_th >= MARGIN and m_gap >= MARGIN


def test_scenes_hold_what_they_claim():
    a, S, _ = inputs("lanes_3d")
    per = {}
    for lab, smp in zip(a["gt_labels"], a["gt_samples"]):
        per[(int(smp), int(lab))] = per.get((int(smp), int(lab)), 0) + 1
    assert sorted(per.values()) == [1, 64, 65, 130]
    ref = reference("lanes_3d")
    assert 0.0 < ref["summary"]["map_all"] < 1.0 and 0.0 < ref["summary"]["map_r40"] < 1.0
    tp = ref["tp"]
    assert tp[0].sum() > tp[3].sum() > 0                                   # the thresholds bite
    mg = ref["match_gt"][0]
    assert len(set(mg[mg >= 0].tolist())) == int((mg >= 0).sum())         # a ground truth is taken once
    # duplicates and second choices occur: some prediction matches a ground truth that is not its best overlap
    pairs = ref["pairs"]
    second = 0
    for i in np.nonzero(mg >= 0)[0]:
        best = max(v for (g, p), v in pairs.items() if p == i)
        second += int(pairs[(int(mg[i]), int(i))] < best)
    assert second > 0
    w, Sw, cw = inputs("wide_3d")
    rw = reference("wide_3d")
    assert Sw == 5 and len(cw["class_range"]) == 32 and len(cw["iou_ths"]) == 8
    assert set(w["pred_samples"].tolist()) >= {0, 2, 4, 5} and not {1, 3} & set(w["gt_samples"].tolist())
    assert (np.diff(w["pred_samples"]) < 0).any()                          # interleaved
    c9 = np.nonzero((w["pred_labels"] == 9) & (w["pred_samples"] == 2))[0]
    assert sorted(rw["tp"][0, c9].tolist()) == [0, 0, 1]                   # the two invalid boxes match nothing
    assert rw["npos"][9] == 3 and rw["npos"][17] == 0 and rw["npos"][8] == 6
    far = np.nonzero(w["pred_boxes"][:, 0] == 70.0)[0]
    assert rw["tp"][:, far].sum() == 0
    assert len(np.unique(w["pred_scores"])) <= len(w["pred_scores"]) - 20  # equal scores


# ---- argument checks ------------------------------------------------------------------------------------------
def test_struct_size_abi_and_symbols():
    from projects.mmdet3d_plugin import native, native_eval as NE
    L = NE.eval_lib()
    assert L.cmt_abi_version() == 25 == native.ABI_VERSION
    assert L.cmt_det_iou_args_size() == ctypes.sizeof(NE.DetIouArgs) == 64
    assert native.STRUCTS["det_iou"] is NE.DetIouArgs
    assert NE.IOU_MODES == {"bev": 0, "3d": 1}


def _valid_base(NE):
    a = NE.DetEvalArgs()
    a.S, a.C, a.T, a.first_ind = 1, 1, 1, 11
    a.range[0] = a.yaw_period[0] = a.dist_th[0] = 1.0
    return a


def test_c_entry_points_refuse_before_any_device_work():
    from projects.mmdet3d_plugin import native_eval as NE
    L = NE.eval_lib()
    nan = float("nan")

    def refused(fn, a, b, message):
        assert fn(ctypes.byref(a), None if b is None else ctypes.byref(b), None) != 0
        assert message in L.cmt_last_error(), L.cmt_last_error()

    for fn in (L.cmt_det_eval_match_iou, L.cmt_det_eval_ap_interp):
        a, b = _valid_base(NE), NE.DetIouArgs()
        refused(fn, a, None, b"null IoU argument struct")
        b.mode = 2
        refused(fn, a, b, b"mode must be 0 (BEV) or 1 (3D)")
        b.mode, b.z_origin = 1, 0.25
        refused(fn, a, b, b"z_origin must be 0 or 0.5")
        b.z_origin = 0.5
        for bad in (1.0, -0.1, nan, float("inf")):
            b.iou_th[0] = bad
            refused(fn, a, b, b"iou_th must be in [0, 1)")
        b.iou_th[0] = 0.5
        # the base struct is checked as cmt_det_eval_match checks it
        a.C = 33
        refused(fn, a, b, b"C must be in [1, 32]")
        a.C, a.dist_th[0] = 1, 0.0
        refused(fn, a, b, b"dist_th must be finite and positive")
        a.dist_th[0] = 1.0
        refused(fn, a, b, b"npos must be non-null")      # N = G = 0: the first pointer that is needed
    # with host words standing in for npos and the workspace, the IoU struct's own pointers are reached; both calls
    # return before a launch
    a, b = _valid_base(NE), NE.DetIouArgs()
    b.mode, b.z_origin, b.iou_th[0] = 0, 0.0, 0.0
    words = (ctypes.c_double * 8)()
    a.npos = a.workspace = ctypes.addressof(words)
    a.workspace_bytes = NE.workspace_bytes(0, 0, 1, 1, 1)
    assert a.workspace_bytes <= ctypes.sizeof(words)
    b.match_iou = ctypes.addressof(words) + 2
    refused(L.cmt_det_eval_match_iou, a, b, b"match_iou must be 4-byte aligned")
    b.match_iou = None
    refused(L.cmt_det_eval_ap_interp, a, b, b"ap_interp must be non-null and 8-byte aligned")
    b.ap_interp = ctypes.addressof(words) + 4
    refused(L.cmt_det_eval_ap_interp, a, b, b"ap_interp must be non-null and 8-byte aligned")


def _cpu_inputs(n=4, g=2):
    return (torch.zeros(n, 9), torch.zeros(n), torch.zeros(n, dtype=torch.int32), torch.zeros(n, dtype=torch.int32),
            torch.zeros(g, 9), torch.zeros(g, dtype=torch.int32), torch.zeros(g, dtype=torch.int32),
            torch.zeros(g, dtype=torch.int32))


CFG = dict(num_samples=1, class_range=[50.0], yaw_period=[TWO_PI], iou_ths=[0.25, 0.5], iou_th_tp=0.5)


@pytest.mark.parametrize("change, message", [
    (dict(iou_ths=[0.1 * k for k in range(9)], iou_th_tp=0.0), "at most 8 IoU thresholds"),
    (dict(iou_ths=[], iou_th_tp=0.5), "at most 8 IoU thresholds"),
    (dict(iou_ths=[0.5, 1.0]), r"iou_ths must be in \[0, 1\)"),
    (dict(iou_ths=[-0.1, 0.5]), r"iou_ths must be in \[0, 1\)"),
    (dict(iou_ths=[float("nan"), 0.5]), r"iou_ths must be in \[0, 1\)"),
    (dict(iou_th_tp=0.3), "not one of iou_ths"),
    (dict(mode="2d"), "mode must be 'bev' or '3d'"),
    (dict(z_origin=1.0), "z_origin must be 0 or 0.5"),
    (dict(class_range=[float("inf")]), "finite and positive"),
    (dict(yaw_period=[0.0]), "finite and positive"),
    (dict(class_range=[50.0] * 33, yaw_period=[TWO_PI] * 33), "at most 32 classes"),
    (dict(min_precision=1.0), "min_precision"),
    (dict(min_recall=1.0), "no recall bin"),
    (dict(num_samples=0), "S must be in"),
    (dict(n_gt=torch.zeros(2, dtype=torch.int32)), "n_gt must be one int32"),
    (dict(), "HIP device"),
])
def test_det_eval_iou_refuses_without_a_device(change, message):
    from projects.mmdet3d_plugin import native_eval as NE
    with pytest.raises(ValueError, match=message):
        NE.det_eval_iou(*_cpu_inputs(), **dict(CFG, **change))
    with pytest.raises(ValueError, match="pred_boxes must be a float32"):
        NE.det_eval_iou(torch.zeros(4, 7), *_cpu_inputs()[1:], **CFG)


def test_config_and_evaluator_refuse_without_a_device():
    from projects.mmdet3d_plugin.core import evaluation as E
    cfg = E.tumtraf_iou_config()
    assert cfg.class_names == E.TUMTRAF_CLASSES and cfg.iou_ths == (0.1, 0.25, 0.5, 0.7) and cfg.iou_th_tp == 0.5
    assert cfg.mode == "3d" and cfg.z_origin == 0.5 and cfg.gt_velocity_zero and cfg.max_boxes_per_sample == 500
    assert list(cfg.class_range) == [E.NO_RANGE] * 9 and math.isfinite(E.NO_RANGE)
    assert all(p == TWO_PI for p in cfg.yaw_period) and cfg.min_recall == 0.1 and cfg.min_precision == 0.1
    assert "not taken from" in E.tumtraf_iou_config.__doc__
    assert E.tumtraf_iou_config(["CAR", "BUS"], mode="bev").mode == "bev"
    with pytest.raises(ValueError, match="mode"):
        E.IouEvalConfig(class_names="ab", mode="2d")
    with pytest.raises(ValueError, match="not one of iou_ths"):
        E.IouEvalConfig(class_names="ab", iou_th_tp=0.6)
    with pytest.raises(ValueError, match="class names"):
        E.IouEvalConfig(class_names="ab", class_range=[50.0])
    with pytest.raises(ValueError, match="max_boxes_per_sample"):
        E.IouEvalConfig(class_names="a", max_boxes_per_sample=0)
    with pytest.raises(ValueError, match="IouEvalConfig"):
        E.IouDetectionEvaluator(E.tumtraf_eval_config(), 2, "cuda")
    with pytest.raises(ValueError, match="DetEvalConfig"):
        E.DetectionEvaluator(cfg, 2, "cuda")
    ev = E.IouDetectionEvaluator(cfg, 2, "cuda")     # allocates nothing yet
    b, s, l = torch.zeros(1, 5, 9), torch.zeros(1, 5), torch.zeros(1, 5, dtype=torch.int32)
    with pytest.raises(ValueError, match="HIP device"):
        ev.add(b, s, l, None, [torch.zeros(2, 9)], [torch.zeros(2, dtype=torch.int64)])
    with pytest.raises(ValueError, match="no frame"):
        ev.compute()


def test_summarize_iou_matches_the_reference_summary():
    from projects.mmdet3d_plugin.core import evaluation as E
    rng = np.random.RandomState(0)
    ap, ai, te = rng.rand(3, 4), rng.rand(3, 4, 2), rng.rand(3, 4)
    te[1, 1] = float("nan")
    cfg = E.IouEvalConfig(class_names="abc")
    got, want = E.summarize_iou(cfg, ap, ai, te, [0.5, float("nan"), 0.75]), R.summary(ap, ai, te)
    assert got["map_all"] == want["map_all"] and got["map_r40"] == want["map_r40"] and got["map_101"] == want["map_101"]
    assert got["tp_errors"] == want["tp_errors"]
    assert got["label_aps"]["b"][0.25] == dict(ap_all=ai[1, 1, 0], ap_r40=ai[1, 1, 1], ap_101=ap[1, 1])
    assert got["mean_aps"]["c"]["ap_r40"] == want["mean_r40"][2]
    assert got["label_mean_iou"]["a"] == 0.5 and math.isnan(got["label_mean_iou"]["b"])
    assert got["label_tp_errors"]["c"]["scale_err"] == te[2, 2]


def test_cli_parses_the_iou_metric():
    spec = importlib.util.spec_from_file_location("cmt_test_cli", os.path.join(PKG, "tools", "test.py"))
    cli = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(cli)
    a = cli.parse_args(["cmt_lidar_nus", "--synthetic", "--eval", "iou"])
    assert a.eval == ["iou"] and a.iou_mode == "3d" and a.iou_thr is None
    a = cli.parse_args(["cmtcoop_fusion_tumtraf", "--synthetic", "--eval", "bbox", "nds", "iou", "--iou-mode", "bev",
                        "--iou-thr", "0.3", "0.6"])
    assert a.eval == ["bbox", "nds", "iou"] and a.iou_mode == "bev" and a.iou_thr == [0.3, 0.6]
    cfg = cli.iou_eval_config(["car", "barrier"], "bev", [0.3, 0.6])
    assert cfg.iou_ths == (0.3, 0.6) and cfg.iou_th_tp == 0.3 and cfg.mode == "bev" and not cfg.gt_velocity_zero
    cfg = cli.iou_eval_config(["CAR", "BUS"])
    assert cfg.iou_ths == (0.1, 0.25, 0.5, 0.7) and cfg.iou_th_tp == 0.5 and cfg.gt_velocity_zero
