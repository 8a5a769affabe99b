"""Detection evaluation without a device: known answers for tests/_eval_ref.py (the numpy restatement of the
cmt_det_eval_* contract), the constants, the argument checks and the CLI's metric names."""
import ctypes
import importlib.util
import math
import os
import sys
from fractions import Fraction

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _eval_ref as R  # noqa: E402

from conftest import PKG  # noqa: E402

TWO_PI = 2 * math.pi


def _box(x, y, dims=(2, 2, 2), yaw=0.5, vel=(1.0, 0.0)):
    return [x, y, 0.0] + list(dims) + [yaw] + list(vel)


def test_known_answer_two_ground_truth_three_predictions():
    """One class, two ground-truth boxes, three predictions with scores 0.75 (0.5 m from the first box), 0.5 (20 m
    from everything) and 0.25 (1 m from the second box), threshold 2 m.

    tp = 1, 0, 1: precision 1, 1/2, 2/3 at recall 1/2, 1/2, 1.  Resampled: recall < 1/2 -> 1 (left value);
    recall = 1/2 -> 1/2 (the LAST of the repeated abscissae); above, 1/2 + (r - 1/2) / 3.
    AP = [39 * 0.9 + 0.4 + sum_{k=51..100} (0.4 + (k - 50) / 300)] / 90 / 0.9 = 59.75 / 81.
    confidence: 0.75, then 0.5 at r = 1/2, then 0.5 - (r - 1/2) / 2.
    trans_err: the matches' errors 0.5 and 1.0 have the cumulative mean 0.5, 0.75; over the confidence that is
    0.75 - (conf - 0.25) / 2, so the curve is 0.5, then 0.625 at r = 1/2, then 0.625 + (r - 1/2) / 4, and its mean
    over k = 11..100 is (19.5 + 0.625 + 31.25 + 1275 / 400) / 90 = 0.60625.
    scale: boxes 2 x 2 x 2 against 2 x 2 x 1: iou = 4 / (8 + 4 - 4) = 1/2 for both, error 1/2.
    orient: yaw 0.5 against 0.25: 0.25.  vel: (1, 0) against (1, 0.5): 0.5.
    At 1 m only the first prediction matches: precision 1, 1/2, 1/3 at recall 1/2 three times, so the curve is 1
    below r = 1/2, 1/3 at it and 0 (right) above: AP = (39 * 0.9 + 1/3 - 0.1) / 81.  At 0.5 m nothing matches."""
    gt = [_box(0.0, 0.0), _box(10.0, 0.0)]
    pred = [_box(0.5, 0.0, dims=(2, 2, 1), yaw=0.25, vel=(1.0, 0.5)), _box(-20.0, 0.0),
            _box(10.0, 1.0, dims=(2, 2, 1), yaw=0.25, vel=(1.0, 0.5))]
    out = R.evaluate(pred, [0.75, 0.5, 0.25], [0, 0, 0], [0, 0, 0], gt, [0, 0], [0, 0], [-1, -1], num_samples=1,
                     class_range=[50.0], yaw_period=[TWO_PI], dist_ths=[0.5, 1.0, 2.0, 4.0], dist_th_tp=2.0)
    assert out["tp"].tolist() == [[0, 0, 0], [1, 0, 0], [1, 0, 1], [1, 0, 1]]   # 0.5 and 1.0 are not below themselves
    assert out["match_gt"][2].tolist() == [0, -1, 1] and out["npos"].tolist() == [1 + 1]
    md = out["md"][(0, 2)]
    r = np.linspace(0, 1, 101)
    want_p = np.where(r < 0.5, 1.0, 0.5 + (r - 0.5) / 3)
    want_c = np.where(r < 0.5, 0.75, 0.5 - (r - 0.5) / 2)
    want_t = np.where(r < 0.5, 0.5, 0.625 + (r - 0.5) / 4)
    np.testing.assert_allclose(md["precision"], want_p, rtol=0, atol=1e-15)
    np.testing.assert_allclose(md["confidence"], want_c, rtol=0, atol=1e-15)
    np.testing.assert_allclose(md["trans_err"], want_t, rtol=0, atol=1e-15)
    assert md["precision"][50] == 0.5 and md["confidence"][50] == 0.5
    assert out["ap"][0, 2] == pytest.approx(59.75 / 81, abs=1e-14)
    assert out["ap"][0, 0] == 0.0 and out["ap"][0, 3] == pytest.approx(59.75 / 81, abs=1e-14)
    ap1 = (39 * 0.9 + 1.0 / 3 - 0.1) / 81
    assert out["ap"][0, 1] == pytest.approx(ap1, abs=1e-14)
    te = dict(zip(R.ERR_NAMES, out["tp_err"][0]))
    assert te["trans_err"] == pytest.approx(0.60625, abs=1e-14)
    assert te["scale_err"] == pytest.approx(0.5, abs=1e-15)
    assert te["orient_err"] == pytest.approx(0.25, abs=1e-15)
    assert te["vel_err"] == pytest.approx(0.5, abs=1e-15)
    s = out["summary"]
    mean_ap = (0 + ap1 + 2 * 59.75 / 81) / 4
    assert s["mean_ap"] == pytest.approx(mean_ap, abs=1e-14)
    nds = (5 * mean_ap + (1 - 0.60625) + 0.5 + 0.75 + 0.5) / 9
    assert s["nd_score"] == pytest.approx(nds, abs=1e-14)


def test_interp_takes_the_last_of_repeated_abscissae():
    assert np.interp(0.5, [0, .5, .5, .5, 1], [1, 2, 3, 4, 5]) == 4
    # the recall grid of the contract, k * 0.01 with the end point set, is numpy's linspace bit for bit
    grid = np.array([1.0 if k == 100 else k * 0.01 for k in range(101)])
    assert np.array_equal(grid, np.linspace(0, 1, 101))


def test_cummean_nan_cases():
    nan = float("nan")
    assert R.cummean([nan, nan, nan]).tolist() == [1.0, 1.0, 1.0]
    assert R.cummean([nan, 2.0, nan, 4.0]).tolist() == [0.0, 2.0, 2.0, 3.0]
    assert R.cummean([1.0, 3.0]).tolist() == [1.0, 2.0]


def test_calc_tp_and_ap_edges():
    md = R.no_predictions()
    assert R.calc_tp(md, 0.1, "trans_err") == 1.0 and R.calc_ap(md, 0.1, 0.1) == 0.0
    md = dict(md, confidence=np.where(np.arange(101) <= 10, 0.5, 0.0), trans_err=np.full(101, 0.25))
    assert R.calc_tp(md, 0.1, "trans_err") == 1.0          # last_ind 10 < first_ind 11
    md["confidence"][11] = 0.5
    assert R.calc_tp(md, 0.1, "trans_err") == 0.25         # exactly one bin
    md["precision"] = np.full(101, 0.05)
    assert R.calc_ap(md, 0.1, 0.1) == 0.0                  # clipped below min_precision


def _orient_exact(d, period):
    """the contract's formula in exact rational arithmetic on the float inputs"""
    P, pi = Fraction(period), Fraction(math.pi)
    a = Fraction(d) + P / 2
    r = a - P * (a // P)          # Python's %: the sign of the divisor
    diff = r - P / 2
    if diff > pi:
        diff -= 2 * pi
    return abs(diff)


@pytest.mark.parametrize("period", [math.pi, TWO_PI])
def test_orient_err_at_the_wraps(period):
    eps = 2.0 ** -20
    for d in (math.pi, -math.pi, math.pi + eps, math.pi - eps, -math.pi + eps, -math.pi - eps, 1.5 * math.pi, 0.0,
              0.5 * math.pi, -0.5 * math.pi):
        d32 = float(np.float32(d))
        got = R.orient_err(np.float32(d), np.float32(0.0), period)
        want = float(_orient_exact(d32, period))
        assert abs(got - want) <= 4e-16 * max(1.0, abs(d32)), (d, period, got, want)
        assert 0.0 <= got <= period / 2 + 1e-15
    assert R.orient_err(1.5 * math.pi, 0.0, TWO_PI) == pytest.approx(0.5 * math.pi, abs=1e-15)
    assert R.orient_err(math.pi, 0.0, math.pi) == pytest.approx(0.0, abs=1e-15)


def test_scale_err_nan_and_order():
    assert R.scale_err([2, 2, 2], [2, 2, 1]) == 0.5
    assert math.isnan(R.scale_err([2, 2, 2], [2, float("nan"), 1]))


def test_tumtraf_constants():
    from projects.mmdet3d_plugin.core.evaluation import TUMTRAF_CLASSES, nuscenes_eval_config, tumtraf_eval_config
    cfg = tumtraf_eval_config()
    assert cfg.class_names == ("CAR", "TRAILER", "TRUCK", "VAN", "PEDESTRIAN", "BUS", "MOTORCYCLE", "BICYCLE",
                               "EMERGENCY_VEHICLE") == TUMTRAF_CLASSES
    assert list(cfg.class_range) == [50, 50, 50, 50, 40, 50, 40, 40, 50]
    assert tuple(cfg.dist_ths) == (0.5, 1.0, 2.0, 4.0) and cfg.dist_th_tp == 2.0
    assert cfg.min_recall == 0.1 and cfg.min_precision == 0.1 and cfg.mean_ap_weight == 5
    assert cfg.max_boxes_per_sample == 500 and cfg.gt_velocity_zero
    assert all(p == TWO_PI for p in cfg.yaw_period)
    sub = tumtraf_eval_config(["BICYCLE", "CAR"])
    assert list(sub.class_range) == [40, 50]
    with pytest.raises(ValueError):
        tumtraf_eval_config(["car"])
    nus = nuscenes_eval_config(["car", "barrier", "traffic_cone"])
    assert list(nus.class_range) == [50, 30, 30] and list(nus.yaw_period) == [TWO_PI, math.pi, TWO_PI]


def test_summarize_matches_reference_summary():
    from projects.mmdet3d_plugin.core.evaluation import DetEvalConfig, summarize
    rng = np.random.RandomState(0)
    ap, te = rng.rand(3, 4), rng.rand(3, 4) * 1.5
    te[1, 1] = float("nan")
    cfg = DetEvalConfig(class_names="abc", class_range=[50, 40, 50], yaw_period=[TWO_PI] * 3)
    got, want = summarize(cfg, ap, te), R.summary(ap, te, 5.0)
    assert got["nd_score"] == want["nd_score"] and got["mean_ap"] == want["mean_ap"]
    assert got["tp_errors"] == want["tp_errors"] and got["tp_scores"] == want["tp_scores"]
    assert got["label_tp_errors"]["b"]["scale_err"] == te[1, 2] and got["label_aps"]["c"][4.0] == ap[2, 3]
    assert list(got["tp_errors"]) == ["trans_err", "scale_err", "orient_err", "vel_err"]


def test_struct_size_and_workspace():
    from projects.mmdet3d_plugin import native_eval as NE
    L = NE.eval_lib()
    assert L.cmt_det_eval_args_size() == ctypes.sizeof(NE.DetEvalArgs)
    assert NE.workspace_bytes(1000, 77, 5, 9, 4) >= 16 * 4 * 1000 + 77
    assert L.cmt_det_eval_workspace_bytes(1 << 31, 0, 1, 1, 1) == -1
    assert L.cmt_det_eval_workspace_bytes(0, 0, 1, 33, 1) == -1 and L.cmt_det_eval_workspace_bytes(0, 0, 1, 1, 9) == -1
    # the C entry points refuse before any device work
    a = NE.DetEvalArgs()
    a.S, a.C, a.T = 1, 33, 1
    assert L.cmt_det_eval_match(ctypes.byref(a), None) != 0
    assert b"C must be in [1, 32]" in L.cmt_last_error()
    a.C, a.T = 1, 9
    assert L.cmt_det_eval_curves(ctypes.byref(a), None) != 0 and b"T must be in [1, 8]" in L.cmt_last_error()
    a.T, a.first_ind, a.N = 1, 11, 1 << 31
    a.range[0] = a.yaw_period[0] = a.dist_th[0] = 1.0
    assert L.cmt_det_eval_keys(ctypes.byref(a), None) != 0 and b"N must be in [0, 2^31)" in L.cmt_last_error()


def _cpu_inputs(n=4, g=2):
    return dict(pred_boxes=torch.zeros(n, 9), pred_scores=torch.zeros(n), pred_labels=torch.zeros(n, dtype=torch.int32),
                pred_samples=torch.zeros(n, dtype=torch.int32), gt_boxes=torch.zeros(g, 9),
                gt_labels=torch.zeros(g, dtype=torch.int32), gt_samples=torch.zeros(g, dtype=torch.int32),
                gt_num_pts=torch.zeros(g, dtype=torch.int32))


CFG = dict(num_samples=1, class_range=[50.0], yaw_period=[TWO_PI], dist_ths=[0.5, 2.0], dist_th_tp=2.0)


@pytest.mark.parametrize("change, message", [
    (dict(pred_boxes=torch.zeros(4, 9, dtype=torch.float64)), "pred_boxes must be a float32"),
    (dict(pred_boxes=torch.zeros(4, 7)), "pred_boxes must be a float32"),
    (dict(pred_scores=torch.zeros(3)), "pred_scores is short"),
    (dict(pred_scores=torch.zeros(8)[::2]), "pred_scores must be contiguous"),
    (dict(pred_labels=torch.zeros(4, dtype=torch.int64)), "pred_labels must be a int32"),
    (dict(gt_num_pts=torch.zeros(1, dtype=torch.int32)), "gt_num_pts is short"),
    (dict(), "HIP device"),
])
def test_det_eval_refuses_bad_tensors_without_a_device(change, message):
    from projects.mmdet3d_plugin import native_eval as NE
    a = dict(_cpu_inputs(), **change)
    with pytest.raises(ValueError, match=message):
        NE.det_eval(a["pred_boxes"], a["pred_scores"], a["pred_labels"], a["pred_samples"], a["gt_boxes"],
                    a["gt_labels"], a["gt_samples"], a["gt_num_pts"], **CFG)


@pytest.mark.parametrize("change, message", [
    (dict(class_range=[50.0] * 33, yaw_period=[TWO_PI] * 33), "at most 32 classes"),
    (dict(dist_ths=[0.5 + k for k in range(9)], dist_th_tp=0.5), "at most 8 distance thresholds"),
    (dict(dist_th_tp=3.0), "not one of dist_ths"),
    (dict(class_range=[float("inf")]), "finite and positive"),
    (dict(yaw_period=[0.0]), "finite and positive"),
    (dict(min_precision=1.0), "min_precision"),
    (dict(min_recall=1.0), "no recall bin"),
    (dict(num_samples=0), "S must be in"),
    (dict(n_pred=torch.zeros(2, dtype=torch.int32)), "n_pred must be one int32"),
])
def test_det_eval_refuses_bad_configuration_without_a_device(change, message):
    from projects.mmdet3d_plugin import native_eval as NE
    a = _cpu_inputs()
    with pytest.raises(ValueError, match=message):
        NE.det_eval(a["pred_boxes"], a["pred_scores"], a["pred_labels"], a["pred_samples"], a["gt_boxes"],
                    a["gt_labels"], a["gt_samples"], a["gt_num_pts"], **dict(CFG, **change))


def test_evaluator_refuses_bad_arguments_without_a_device():
    from projects.mmdet3d_plugin.core.evaluation import DetEvalConfig, DetectionEvaluator, tumtraf_eval_config
    cfg = tumtraf_eval_config()
    with pytest.raises(ValueError):
        DetectionEvaluator(dict(), 4, "cuda")
    with pytest.raises(ValueError):
        DetectionEvaluator(cfg, 0, "cuda")
    with pytest.raises(ValueError, match="max_boxes_per_sample"):
        DetEvalConfig(class_names="a", class_range=[50], yaw_period=[TWO_PI], max_boxes_per_sample=1025)
    with pytest.raises(ValueError, match="class names"):
        DetEvalConfig(class_names="ab", class_range=[50], yaw_period=[TWO_PI])
    ev = DetectionEvaluator(cfg, 2, "cuda")     # allocates nothing yet
    b, s, l = torch.zeros(1, 5, 9), torch.zeros(1, 5), torch.zeros(1, 5, dtype=torch.int32)
    gb, gl = [torch.zeros(2, 9)], [torch.zeros(2, dtype=torch.int64)]
    with pytest.raises(ValueError, match="HIP device"):
        ev.add(b, s, l, None, gb, gl)
    with pytest.raises(ValueError, match="boxes per sample"):
        ev.add(torch.zeros(1, 501, 9), torch.zeros(1, 501), torch.zeros(1, 501, dtype=torch.int32), None, gb, gl)
    with pytest.raises(ValueError, match="fp32"):
        ev.add(b.double(), s, l, None, gb, gl)
    with pytest.raises(ValueError, match="count must be int32"):
        ev.add(b, s, l, torch.zeros(2, dtype=torch.int32), gb, gl)
    with pytest.raises(ValueError, match="ground truth"):
        ev.add(b, s, l, None, gb + gb, gl + gl)
    with pytest.raises(ValueError, match="required"):
        ev.add(b, s, l)
    with pytest.raises(ValueError, match="capacity"):
        ev.add(b.expand(3, 5, 9), s.expand(3, 5), l.expand(3, 5), None, gb * 3, gl * 3)
    with pytest.raises(ValueError, match="no frame"):
        ev.compute()


def test_cli_parses_the_nds_metric():
    spec = importlib.util.spec_from_file_location("cmt_test_cli", os.path.join(PKG, "tools", "test.py"))
    cli = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(cli)
    a = cli.parse_args(["cmtcoop_fusion_tumtraf", "--synthetic", "--detector", "--eval", "bbox", "nds"])
    assert a.eval == ["bbox", "nds"]
    assert cli.parse_args(["cmt_lidar_nus", "--synthetic", "--eval", "nds"]).eval == ["nds"]
    assert cli.eval_config(["CAR", "BUS"]).gt_velocity_zero and not cli.eval_config(["car", "barrier"]).gt_velocity_zero
    b0, l0 = cli.frame_ground_truth(0, 0, [-72.0, -72.0, -8, 72.0, 72.0, 0], 7)
    b1, _ = cli.frame_ground_truth(1, 0, [-72.0, -72.0, -8, 72.0, 72.0, 0], 7)
    assert tuple(b0.shape) == (20, 9) and b0.dtype == torch.float32 and tuple(l0.shape) == (20,) and not torch.equal(b0, b1)
