"""cmt_det_eval_match_iou / cmt_det_eval_ap_interp / IouDetectionEvaluator on the device against
tests/_eval_iou_ref.py (the contract of cmt_hip.h in numpy).

The scenes are those of tests/test_eval_iou_host.py, which asserts that none of them decides anything within 1e-4 of
a rounding (the device's float32 IoU is within 8 x measure_e32() < 6.7e-6 of float64).  Held to:
  * tp, match_gt and npos equal exactly;
  * match_iou within the bar of tests/test_gpu_iou.py, 8 x _iou_ref.measure_e32();
  * every curve value, the 101-point AP, the TP errors, ap_all and ap_r40 within 1e-9 * max(1, |value|): given equal
    tp they are the same float64 arithmetic up to the order of the curves' cumulative sums.
"""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _eval_iou_ref as R  # noqa: E402
import _iou_ref as I  # noqa: E402
import test_eval_iou_host as H  # noqa: E402

from conftest import PKG, ROOT  # noqa: E402

pytestmark = pytest.mark.gpu


@pytest.fixture(autouse=True)
def _device(dev):
    return dev


TOL = 1e-9
CURVES = ("recall", "precision", "confidence") + R.ERR_NAMES


def iou_bar():
    return 8 * I.measure_e32()


def to_dev(a):
    return {k: torch.from_numpy(v).cuda() for k, v in a.items()}


def call(d, S, cfg, **kw):
    from projects.mmdet3d_plugin import native_eval as NE
    return NE.det_eval_iou(d["pred_boxes"], d["pred_scores"], d["pred_labels"], d["pred_samples"], d["gt_boxes"],
                           d["gt_labels"], d["gt_samples"], d["gt_num_pts"], num_samples=S, **cfg, **kw)


def run_device(name):
    a, S, cfg = H.inputs(name)
    out = call(to_dev(a), S, cfg)
    torch.cuda.synchronize()
    return {k: v.cpu().numpy() for k, v in out.items()}


def close(got, want, what, tol=TOL, scaled=True):
    got, want = np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64)
    assert got.shape == want.shape, what
    assert np.array_equal(np.isnan(got), np.isnan(want)), f"{what}: NaN pattern differs"
    m = ~np.isnan(want)
    err = np.abs(got[m] - want[m]) / (np.maximum(1.0, np.abs(want[m])) if scaled else 1.0)
    worst = float(err.max()) if err.size else 0.0
    print(f"{what}: max error {worst:.3e} (bound {tol:.3e})")
    assert worst <= tol, f"{what}: max error {worst:.3e} > {tol:.3e}"


def check(out, ref, n=None):
    C, T = ref["ap"].shape
    n = ref["tp"].shape[1] if n is None else n
    assert np.array_equal(out["npos"], ref["npos"]), (out["npos"], ref["npos"])
    assert np.array_equal(out["tp"][:, :n], ref["tp"][:, :n])
    assert np.array_equal(out["match_gt"][:, :n], ref["match_gt"][:, :n])
    assert out["match_iou"].dtype == np.float32
    close(out["match_iou"][:, :n], ref["match_iou"][:, :n], "match_iou", iou_bar(), scaled=False)
    close(out["err"][:, :, :n], ref["err"][:, :, :n], "err")
    worst = 0.0
    for c in range(C):
        for t in range(T):
            for i, k in enumerate(CURVES):
                got, want = out["md"][c, t, i], ref["md"][(c, t)][k]
                assert not np.isnan(got).any()
                worst = max(worst, float((np.abs(got - want) / np.maximum(1.0, np.abs(want))).max()))
    print(f"md: max scaled error {worst:.3e}")
    assert worst <= TOL
    close(out["ap"], ref["ap"], "ap_101")
    close(out["tp_err"], ref["tp_err"], "tp_err")
    close(out["ap_interp"][:, :, 0], ref["ap_interp"][:, :, 0], "ap_all")
    close(out["ap_interp"][:, :, 1], ref["ap_interp"][:, :, 1], "ap_r40")


@pytest.mark.parametrize("name", sorted(H.CASES))
def test_matches_reference(name):
    check(run_device(name), H.reference(name))


def test_buffers_guarded_and_device_counts():
    """capacity-sized inputs with device counts below the capacity and rows beyond them that look like perfect,
    high-scoring detections; outputs and workspace pre-filled with NaN / sentinels: every output element is written,
    the guard tails behind every buffer are untouched"""
    from projects.mmdet3d_plugin import native_eval as NE
    a, S, cfg = H.inputs("wide_3d")
    ref = H.reference("wide_3d")
    n, g = len(a["pred_scores"]), len(a["gt_labels"])
    pad_n, pad_g, guard = 37, 11, 64
    big = dict(a)
    big["pred_boxes"] = np.concatenate([a["pred_boxes"], a["gt_boxes"][:pad_n]])
    big["pred_scores"] = np.concatenate([a["pred_scores"], np.full(pad_n, 2.0, np.float32)])
    big["pred_labels"] = np.concatenate([a["pred_labels"], a["gt_labels"][:pad_n]])
    big["pred_samples"] = np.concatenate([a["pred_samples"], a["gt_samples"][:pad_n]])
    big["gt_boxes"] = np.concatenate([a["gt_boxes"], a["pred_boxes"][:pad_g]])
    big["gt_labels"] = np.concatenate([a["gt_labels"], a["pred_labels"][:pad_g]])
    big["gt_samples"] = np.concatenate([a["gt_samples"], a["pred_samples"][:pad_g]])
    big["gt_num_pts"] = np.concatenate([a["gt_num_pts"], np.full(pad_g, 5, np.int32)])
    d = to_dev(big)
    N, G, C, T = n + pad_n, g + pad_g, len(cfg["class_range"]), len(cfg["iou_ths"])
    shapes = dict(tp=((T, N), torch.uint8), match_gt=((T, N), torch.int32), err=((T, 4, N), torch.float64),
                  npos=((C,), torch.int32), md=((C, T, 7, 101), torch.float64), ap=((C, T), torch.float64),
                  tp_err=((C, 4), torch.float64), match_iou=((T, N), torch.float32),
                  ap_interp=((C, T, 2), torch.float64))
    fill = {torch.uint8: 0xA5, torch.int32: -77777, torch.float64: float("nan"), torch.float32: -7.0}
    flat, out = {}, {}
    for k, (shape, dt) in shapes.items():
        numel = int(np.prod(shape))
        flat[k] = torch.full((numel + guard,), fill[dt], dtype=dt, device="cuda")
        out[k] = flat[k][:numel].view(shape)
    need = NE.workspace_bytes(N, G, S, C, T)
    ws = torch.full((need + guard,), 0xA5, dtype=torch.uint8, device="cuda")
    res = call(d, S, cfg, n_pred=torch.tensor([n], dtype=torch.int32, device="cuda"),
               n_gt=torch.tensor([g], dtype=torch.int32, device="cuda"), out=out, workspace=ws[:need])
    torch.cuda.synchronize()
    got = {k: v.cpu().numpy() for k, v in res.items()}
    check(got, ref, n=n)
    assert (got["tp"][:, n:] == 0).all() and (got["match_gt"][:, n:] == -1).all() and np.isnan(got["err"][:, :, n:]).all()
    assert np.isnan(got["match_iou"][:, n:]).all() and not (got["match_iou"] == -7.0).any()
    assert np.isin(got["tp"], (0, 1)).all() and (got["match_gt"] != -77777).all() and (got["npos"] != -77777).all()
    assert np.array_equal(np.isnan(got["err"][:, 0]), got["tp"] == 0)
    for k in ("md", "ap", "tp_err", "ap_interp"):
        assert not np.isnan(got[k]).any(), k
    for k, (shape, dt) in shapes.items():
        tail = flat[k][int(np.prod(shape)):].cpu()
        assert bool(torch.isnan(tail).all()) if dt == torch.float64 else bool((tail == fill[dt]).all()), k
    assert bool((ws[need:] == 0xA5).all())


def test_two_runs_bit_equal():
    one, two = run_device("lanes_3d"), run_device("lanes_3d")
    assert set(one) == {"tp", "match_gt", "err", "npos", "md", "ap", "tp_err", "match_iou", "ap_interp"}
    for k in one:
        assert one[k].tobytes() == two[k].tobytes(), k


def test_match_iou_is_box_iou_with_the_ground_truth_first():
    """the value written for a match is cmt_box_iou's for (ground truth, prediction), bit for bit"""
    from projects.mmdet3d_plugin import native_iou as NI
    a, _, cfg = H.inputs("lanes_3d")
    out = run_device("lanes_3d")
    t = 1
    rows = np.nonzero(out["tp"][t])[0]
    gt = torch.from_numpy(a["gt_boxes"][out["match_gt"][t, rows]]).cuda()
    pr = torch.from_numpy(a["pred_boxes"][rows]).cuda()
    v3 = NI.box_iou(gt, pr, mode="3d", aligned=True, z_origin=cfg["z_origin"])
    assert rows.size > 50
    assert v3.cpu().numpy().tobytes() == out["match_iou"][t, rows].tobytes()


def test_evaluator_three_frames():
    """IouDetectionEvaluator on padded frames with device counts: the dictionary of compute() and the curves of
    metric_data() equal the reference"""
    from projects.mmdet3d_plugin.core.evaluation import IouDetectionEvaluator, IouEvalConfig
    a, S, cfg = H.inputs("frames")
    ref = H.reference("frames")
    names = ("a", "b", "c")
    ev = IouDetectionEvaluator(IouEvalConfig(class_names=names, iou_ths=cfg["iou_ths"], iou_th_tp=cfg["iou_th_tp"],
                                             mode=cfg["mode"], z_origin=cfg["z_origin"], yaw_period=cfg["yaw_period"]),
                               S, "cuda")
    M = 24
    boxes = np.zeros((S, M, 9), np.float32)
    scores, labels, count = np.zeros((S, M), np.float32), np.zeros((S, M), np.int32), np.zeros(S, np.int32)
    for i in range(len(a["pred_scores"])):
        s = a["pred_samples"][i]
        boxes[s, count[s]], scores[s, count[s]], labels[s, count[s]] = a["pred_boxes"][i], a["pred_scores"][i], a["pred_labels"][i]
        count[s] += 1
    cu = lambda v: torch.from_numpy(np.ascontiguousarray(v)).cuda()  # noqa: E731
    for s in range(S):
        m = a["gt_samples"] == s
        k = min(M - count[s], int(m.sum()))      # rows behind the count look like perfect detections
        boxes[s, count[s]:count[s] + k], scores[s, count[s]:count[s] + k] = a["gt_boxes"][m][:k], 3.0
        labels[s, count[s]:count[s] + k] = a["gt_labels"][m][:k]
        ev.add(cu(boxes[s:s + 1]), cu(scores[s:s + 1]), cu(labels[s:s + 1]), cu(count[s:s + 1]),
               [cu(a["gt_boxes"][m])], [cu(a["gt_labels"][m])], [cu(a["gt_num_pts"][m])])
    got = ev.compute()
    want = ref["summary"]
    for k in ("map_all", "map_r40", "map_101"):
        close(got[k], want[k], k)
    for k in R.TP_METRICS:
        close(got["tp_errors"][k], want["tp_errors"][k], k)
    for c, name in enumerate(names):
        for t, th in enumerate(cfg["iou_ths"]):
            d = got["label_aps"][name][th]
            close([d["ap_all"], d["ap_r40"], d["ap_101"]], [ref["ap_interp"][c, t, 0], ref["ap_interp"][c, t, 1], ref["ap"][c, t]],
                  f"label_aps[{name}][{th}]")
        close([got["label_tp_errors"][name][k] for k in R.ERR_NAMES], ref["tp_err"][c], f"label_tp_errors[{name}]")
        close(got["mean_aps"][name]["ap_all"], want["mean_all"][c], f"mean_aps[{name}]")
    close([got["label_mean_iou"][n] for n in names], ref["mean_iou"], "label_mean_iou", iou_bar(), scaled=False)
    assert 0.0 < got["map_all"] < 1.0 and got["mode"] == "3d" and got["iou_th_tp"] == 0.5
    md = ev.metric_data()
    assert set(md) == {f"{n}:{float(th)}" for n in names for th in cfg["iou_ths"]}
    close(md["b:0.5"]["precision"], ref["md"][(1, 2)]["precision"], "metric_data")
    assert set(ev.detail()) >= {"object/map_all", "object/map_r40", "object/a_ap_all_iou_0.5"}
    ev.reset()
    with pytest.raises(ValueError):
        ev.compute()


def test_cli_eval_iou_in_a_fresh_process():
    """tools/test.py --eval iou: one JSON line metric="iou_ap" (random weights: the boxes hardly ever overlap the
    ground truth, so this checks the plumbing; the cases above check the arithmetic)"""
    r = subprocess.run([sys.executable, os.path.join(PKG, "tools", "test.py"), "cmt_lidar_nus", "--synthetic",
                        "--num-query", "32", "--num-layers", "1", "--eval", "iou"],
                       cwd=ROOT, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    lines = [json.loads(l) for l in r.stdout.strip().splitlines() if l.startswith("{")]
    assert [l["metric"] for l in lines] == [["iou"], "iou_ap"]
    m = lines[-1]
    assert {"frames", "gt_per_frame", "label_aps", "mean_aps", "map_all", "map_r40", "map_101", "label_tp_errors",
            "tp_errors", "label_mean_iou", "iou_ths", "iou_th_tp", "mode"} <= set(m)
    assert m["frames"] == 1 and m["mode"] == "3d" and m["iou_ths"] == [0.1, 0.25, 0.5, 0.7] and m["iou_th_tp"] == 0.5
    assert 0.0 <= m["map_all"] <= 1.0 and 0.0 <= m["map_r40"] <= 1.0
    first = next(iter(m["label_aps"].values()))
    assert set(first) == {"0.1", "0.25", "0.5", "0.7"} and set(first["0.5"]) == {"ap_all", "ap_r40", "ap_101"}
