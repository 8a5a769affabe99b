"""Tracking evaluation without a device: the C ABI's symbols, struct size and argument errors, the wrappers'
ValueErrors, hand-worked answers for tests/_mot_ref.py (the numpy restatement of the cmt_mot_eval_* contract), and the
restatement's uniqueness assertion over the seeded cases tests/test_gpu_mot.py runs on the device."""
import ctypes
import math
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _mot_cases as MC  # noqa: E402
import _mot_ref as R  # noqa: E402

EINVAL, ENOTSUP = 1001, 1002
CALLS = ("keys", "runs", "cost", "update", "thresholds", "summary")


@pytest.fixture(scope="module")
def NE():
    from projects.mmdet3d_plugin import native_eval
    native_eval.mot_lib()
    return native_eval


# ---- the C ABI ------------------------------------------------------------------------------------------------

def test_symbols_struct_size_and_abi(NE):
    from projects.mmdet3d_plugin import native
    L = NE.mot_lib()
    for name in CALLS:
        assert hasattr(L, "cmt_mot_eval_" + name)
    assert L.cmt_mot_eval_args_size() == ctypes.sizeof(NE.MotEvalArgs)
    assert L.cmt_abi_version() == native.ABI_VERSION == 25
    hdr = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "cmt_hip.h")).read()
    assert "tracking evaluation (moteval.hip; additive to ABI 25)" in hdr
    assert "NOT been compared with an installed devkit" in hdr
    for name, value in (("CMT_MOT_MAX_CLASSES", NE.MOT_MAX_CLASSES), ("CMT_MOT_MAX_THRESHOLDS", NE.MOT_MAX_THRESHOLDS),
                        ("CMT_MOT_MAX_GT_TRACKS", NE.MOT_MAX_GT_TRACKS), ("CMT_MOT_MAX_GT", NE.MOT_MAX_GT),
                        ("CMT_MOT_MAX_PRED", NE.MOT_MAX_PRED), ("CMT_MOT_MAX_CHAINS", NE.MOT_MAX_CHAINS)):
        assert f"#define {name} {value}\n" in hdr


def _args(NE, **over):
    """a struct every call accepts (made-up, aligned pointers: never passed on without one broken field)"""
    a = NE.MotEvalArgs()
    a.N, a.G, a.F, a.S, a.Fmax, a.C, a.R, a.ld_pred, a.ld_gt, a.max_gt_tracks = 8, 8, 4, 2, 2, 3, 5, 9, 9, 16
    a.phase, a.step, a.chain0, a.nchains, a.Gmax, a.Hmax = 2, 0, 0, 30, 4, 4
    a.range[:3], a.dist_th[:3], a.recall[:5] = [50.0] * 3, [2.0] * 3, [0.2, 0.4, 0.6, 0.8, 1.0]
    for name, _ in NE.MotEvalArgs._fields_:
        if isinstance(getattr(a, name), (int, type(None))) and name not in ("N", "G") and getattr(NE.MotEvalArgs, name).size == 8:
            setattr(a, name, 0x10000)
    for k, v in over.items():
        if isinstance(v, tuple):
            getattr(a, k)[v[0]] = v[1]
        else:
            setattr(a, k, v)
    return a


BASE_ERRORS = [(dict(N=-1), EINVAL), (dict(N=2 ** 31), EINVAL), (dict(G=-1), EINVAL), (dict(G=2 ** 31), EINVAL),
               (dict(F=0), EINVAL), (dict(S=0), EINVAL), (dict(Fmax=0), EINVAL), (dict(S=4097, Fmax=4096), EINVAL),
               (dict(C=0), EINVAL), (dict(R=0), EINVAL), (dict(max_gt_tracks=0), EINVAL), (dict(C=65), ENOTSUP),
               (dict(R=65), ENOTSUP), (dict(max_gt_tracks=65537), ENOTSUP), (dict(ld_pred=1), EINVAL), (dict(ld_gt=1), EINVAL),
               (dict(range=(1, 0.0)), EINVAL), (dict(range=(2, float("inf"))), EINVAL), (dict(range=(0, float("nan"))), EINVAL),
               (dict(dist_th=(1, -1.0)), EINVAL), (dict(dist_th=(0, float("nan"))), EINVAL),
               (dict(recall=(0, 0.0)), EINVAL), (dict(recall=(4, 1.5)), EINVAL), (dict(recall=(2, float("nan"))), EINVAL)]
STEP_ERRORS = [(dict(phase=0), EINVAL), (dict(phase=3), EINVAL), (dict(step=-1), EINVAL), (dict(step=2), EINVAL),
               (dict(chain0=-1), EINVAL), (dict(nchains=0), EINVAL), (dict(chain0=1, nchains=30), EINVAL),
               (dict(phase=1, nchains=7), EINVAL), (dict(Gmax=-1), EINVAL), (dict(Hmax=-1), EINVAL),
               (dict(Gmax=513), ENOTSUP), (dict(Hmax=2049), ENOTSUP), (dict(S=40000, Fmax=1, nchains=65536), ENOTSUP)]
POINTERS = dict(
    keys=("pred_box", "pred_score", "pred_label", "pred_track", "pred_frame", "gt_box", "gt_label", "gt_frame", "gt_inst",
          "tp_score", "tp_key", "frame_tab", "key_pred", "key_gt"),
    runs=("sk_pred", "sk_gt", "npos", "run_max"),
    cost=("pred_box", "pred_score", "pred_track", "gt_box", "gt_inst", "sk_pred", "sk_gt", "state_m", "state_lost", "desc",
          "cost", "cols", "smatch", "thr"),
    update=("match_q", "match_g", "chain_cnt2", "chain_dist2", "tp_score", "tp_key", "cols", "smatch", "cost", "desc"),
    thresholds=("sk_tp", "si_tp", "tp_score", "npos", "thr"),
    summary=("npos", "thr", "chain_cnt1", "chain_dist1", "chain_cnt2", "chain_dist2", "counters", "dist_sum", "metrics",
             "class_sum", "counters1", "dist_sum1"))


def _rc(NE, call, a):
    return getattr(NE.mot_lib(), "cmt_mot_eval_" + call)(None if a is None else ctypes.byref(a), None)


@pytest.mark.parametrize("call", CALLS)
def test_argument_errors_before_any_device_work(NE, call):
    L = NE.mot_lib()
    assert _rc(NE, call, None) == EINVAL and b"null argument struct" in L.cmt_last_error()
    for over, want in BASE_ERRORS + (STEP_ERRORS if call in ("cost", "update") else []):
        assert _rc(NE, call, _args(NE, **over)) == want, (call, over, L.cmt_last_error())
        assert call.encode() in L.cmt_last_error()
    for name in POINTERS[call]:
        assert _rc(NE, call, _args(NE, **{name: None})) == EINVAL, (call, name)
        assert name.encode() in L.cmt_last_error()
        if name != "state_lost":   # a byte array has no alignment
            assert _rc(NE, call, _args(NE, **{name: 0x10001})) == EINVAL, (call, name, "misaligned")
    if call == "keys":
        assert _rc(NE, call, _args(NE, n_pred=0x10002)) == EINVAL and _rc(NE, call, _args(NE, n_gt=0x10001)) == EINVAL
    if call == "update":   # phase 1 writes the other pair of chain buffers
        assert _rc(NE, call, _args(NE, phase=1, nchains=6, chain_cnt1=None)) == EINVAL


def test_wrapper_value_errors(NE):
    ok = dict(class_range=[50.0, 40.0], dist_th=[2.0, 2.0], recall=[0.5, 1.0], max_gt_tracks=8)
    assert NE.check_mot_config(**ok) == ([50.0, 40.0], [2.0, 2.0], [0.5, 1.0], 8)
    for bad in (dict(class_range=[50.0]), dict(class_range=[50.0, -1.0]), dict(dist_th=[2.0, float("nan")]),
                dict(recall=[]), dict(recall=[0.0, 1.0]), dict(recall=[0.5, 1.1]), dict(max_gt_tracks=0),
                dict(max_gt_tracks=65537), dict(class_range=[1.0] * 65, dist_th=[1.0] * 65), dict(recall=[0.5] * 65)):
        with pytest.raises(ValueError):
            NE.check_mot_config(**dict(ok, **bad))
    assert NE.mot_recall_levels(1, 0.1) == [1.0]
    lv = NE.mot_recall_levels(40, 0.1)
    assert lv == R.recall_levels(40, 0.1) and lv[0] == 0.1 and abs(lv[-1] - 1.0) < 1e-15 and len(lv) == 40
    for bad in ((0, 0.1), (65, 0.1), (5, 0.0), (5, 1.5)):
        with pytest.raises(ValueError):
            NE.mot_recall_levels(*bad)
    i32 = torch.int32
    t = dict(pb=torch.zeros((3, 9)), ps=torch.zeros(3), pl=torch.zeros(3, dtype=i32), pt=torch.zeros(3, dtype=i32),
             pf=torch.zeros(3, dtype=i32), gb=torch.zeros((2, 9)), gl=torch.zeros(2, dtype=i32), gf=torch.zeros(2, dtype=i32),
             gi=torch.zeros(2, dtype=i32), tab=torch.zeros((1, 2), dtype=i32))
    kw = dict(num_scenes=1, max_steps=1, **ok)

    def run(**over):
        v = dict(t, **{k: x for k, x in over.items() if k in t})
        NE.mot_eval(v["pb"], v["ps"], v["pl"], v["pt"], v["pf"], v["gb"], v["gl"], v["gf"], v["gi"], v["tab"],
                    **dict(kw, **{k: x for k, x in over.items() if k not in t}))
    for bad, match in ((dict(pb=torch.zeros((3, 1))), "pred_boxes"), (dict(ps=torch.zeros(2)), "short"),
                       (dict(pl=torch.zeros(3)), "pred_labels"), (dict(pt=torch.zeros(3, dtype=torch.int64)), "pred_tracks"),
                       (dict(gb=torch.zeros(2)), "gt_boxes"), (dict(gi=torch.zeros(1, dtype=i32)), "short"),
                       (dict(tab=torch.zeros((1, 3), dtype=i32)), "frame_table"), (dict(num_scenes=0), "num_scenes"),
                       (dict(num_scenes=4097, max_steps=4096), "2\\^24"), (dict(workspace_bytes=0), "workspace_bytes"),
                       (dict(n_pred=torch.zeros(2, dtype=i32)), "n_pred"), (dict(recall=[2.0]), "recall"),
                       (dict(), "HIP device")):
        with pytest.raises(ValueError, match=match):
            run(**bad)


def test_evaluator_value_errors():
    from projects.mmdet3d_plugin.core import evaluation as E
    with pytest.raises(ValueError):
        E.MotEvalConfig(class_names=["a", "b"], class_range=[1.0])
    with pytest.raises(ValueError):
        E.MotEvalConfig(class_names=["a"], num_thresholds=0)
    with pytest.raises(ValueError):
        E.tumtraf_mot_config(["nope"])
    cfg = E.nuscenes_mot_config()
    assert len(cfg.class_names) == 7 and cfg.dist_th == [2.0] * 7 and cfg.num_thresholds == 40 and cfg.min_recall == 0.1
    assert E.tumtraf_mot_config().class_range[4] == 40.0
    ev = E.TrackingEvaluator(E.MotEvalConfig(class_names=["a"], max_boxes_per_frame=4), 2, "cpu")
    b, s, lab, tr = torch.zeros((2, 9)), torch.zeros(2), torch.zeros(2, dtype=torch.int32), torch.zeros(2, dtype=torch.int32)
    gt = dict(gt_boxes=torch.zeros((1, 9)), gt_labels=torch.zeros(1, dtype=torch.int32), gt_ids=torch.zeros(1, dtype=torch.int32))
    with pytest.raises(ValueError, match="HIP device"):
        ev.add(b, s, lab, tr, scene=0, **gt)
    with pytest.raises(ValueError, match="int32"):
        ev.add(b, s, lab, tr.long(), scene=0, **gt)
    with pytest.raises(ValueError, match="per frame"):
        ev.add(torch.zeros((5, 9)), torch.zeros(5), torch.zeros(5, dtype=torch.int32), torch.zeros(5, dtype=torch.int32), scene=0, **gt)
    with pytest.raises(ValueError, match="negative"):
        ev.add(b, s, lab, tr, scene=-1, **gt)
    with pytest.raises(ValueError, match="no frame"):
        ev.run()
    with pytest.raises(ValueError):
        E.TrackingEvaluator(object(), 2, "cpu")
    nan = float("nan")
    cs = np.array([[0.5, 1.0, 3, 0.4, 0.9, 0.6, 6, 1, 4, 1, 2, 0.3], [nan, nan, -1] + [nan] * 9])
    m = E.summarize_mot(E.MotEvalConfig(class_names=["a", "b"]), cs, [10, 0])
    assert m["classes_evaluated"] == ["a"] and m["amota"] == 0.5 and m["ids"] == 1 and m["frag"] == 2
    assert m["label_metrics"]["a"]["best_slot"] == 3 and m["label_metrics"]["b"]["ids"] is None


def test_cli_eval_track_needs_track(capsys):
    import importlib.util
    from conftest import PKG
    spec = importlib.util.spec_from_file_location("cmt_test_cli_mot_host", os.path.join(PKG, "tools", "test.py"))
    cli = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(cli)
    with pytest.raises(SystemExit) as e:
        cli.parse_args(["cmt_lidar_nus", "--synthetic", "--eval", "track"])
    assert e.value.code == 2 and "needs --track" in capsys.readouterr().err
    a = cli.parse_args(["cmt_lidar_nus", "--synthetic", "--eval", "bbox", "track", "--track"])
    assert a.eval == ["bbox", "track"] and a.track


# ---- the restatement, by hand ----------------------------------------------------------------------------------

def ev(pred, gt, frames, C=1, recall=(1.0,), dist_th=2.0, scenes=1, **kw):
    """pred rows (frame, x, y, score, track[, label]); gt rows (frame, x, y, inst[, label]); one scene of ``frames``
    steps unless ``table`` says otherwise"""
    pred, gt = [tuple(p) + (0,) * (6 - len(p)) for p in pred], [tuple(g) + (0,) * (5 - len(g)) for g in gt]
    table = kw.pop("table", [(0, t) for t in range(frames)])
    return R.evaluate(np.array([[p[1], p[2]] for p in pred], dtype=np.float32).reshape(-1, 2), [p[3] for p in pred],
                      [p[5] for p in pred], [p[4] for p in pred], [p[0] for p in pred],
                      np.array([[g[1], g[2]] for g in gt], dtype=np.float32).reshape(-1, 2), [g[4] for g in gt],
                      [g[0] for g in gt], [g[3] for g in gt], table, num_scenes=scenes, max_steps=frames,
                      class_range=[100.0] * C, dist_th=[dist_th] * C, recall=list(recall), max_gt_tracks=8, **kw)


def cnt(out, c=0):
    return dict(zip(R.COUNTERS, out["counters1"][c].tolist()))


def test_sticky_pass_keeps_the_previous_track():
    """frame 1 has a nearer, admissible prediction of another track: the previous track stays, no switch"""
    out = ev([(0, 0.5, 0, 0.9, 1), (1, 1.0, 0, 0.9, 1), (1, 0.125, 0, 0.9, 2)], [(0, 0, 0, 0), (1, 0, 0, 0)], 2)
    assert cnt(out) == dict(tp=2, fp=1, fn=0, ids=0, frag=0, npred=3) and out["dist_sum1"][0] == 1.5
    # without the sticky pass the assignment would take the nearer one: the same frame alone
    alone = ev([(0, 1.0, 0, 0.9, 1), (0, 0.125, 0, 0.9, 2)], [(0, 0, 0, 0)], 1)
    assert alone["dist_sum1"][0] == 0.125
    # an inadmissible previous track does not stick
    far = ev([(0, 0.5, 0, 0.9, 1), (1, 2.5, 0, 0.9, 1), (1, 0.125, 0, 0.9, 2)], [(0, 0, 0, 0), (1, 0, 0, 0)], 2)
    assert cnt(far)["ids"] == 1 and far["dist_sum1"][0] == 0.625


def test_switches():
    """a switch when the previous track is absent, and a switch after a gap of missed frames (which is also a
    fragmentation)"""
    out = ev([(0, 0.5, 0, 0.9, 1), (1, 0.25, 0, 0.9, 2)], [(0, 0, 0, 0), (1, 0, 0, 0)], 2)
    assert cnt(out) == dict(tp=2, fp=0, fn=0, ids=1, frag=0, npred=2)
    out = ev([(0, 0.5, 0, 0.9, 1), (3, 0.25, 0, 0.9, 2)], [(t, 0, 0, 0) for t in range(4)], 4)
    assert cnt(out) == dict(tp=2, fp=0, fn=2, ids=1, frag=1, npred=2)
    # the first match of an instance is no switch, whatever the id
    out = ev([(1, 0.5, 0, 0.9, 5)], [(0, 0, 0, 0), (1, 0, 0, 0)], 2)
    assert cnt(out) == dict(tp=1, fp=0, fn=1, ids=0, frag=0, npred=1)


def test_frag_counts_on_reacquisition_only():
    gt = [(t, 0, 0, 0) for t in range(4)]
    out = ev([(0, 0.5, 0, 0.9, 1), (1, 0.5, 0, 0.9, 1)], gt, 4)   # match, match, miss, miss
    assert cnt(out) == dict(tp=2, fp=0, fn=2, ids=0, frag=0, npred=2)
    out = ev([(0, 0.5, 0, 0.9, 1), (3, 0.5, 0, 0.9, 1)], gt, 4)   # match, miss, miss, match
    assert cnt(out) == dict(tp=2, fp=0, fn=2, ids=0, frag=1, npred=2)
    out = ev([(0, 0.5, 0, 0.9, 1), (2, 0.5, 0, 0.9, 1)], gt, 4)   # match, miss, match, miss
    assert cnt(out) == dict(tp=2, fp=0, fn=2, ids=0, frag=1, npred=2)
    out = ev([(2, 0.5, 0, 0.9, 1)], gt, 4)                        # misses before the first match are none
    assert cnt(out) == dict(tp=1, fp=0, fn=3, ids=0, frag=0, npred=1)


def test_two_instances_holding_the_same_last_track():
    """instances 0 and 1 were both last matched to track 7; in frame 2 the sticky pass is sequential: instance 0 (the
    first row) takes the box although it is nearer to instance 1"""
    pred = [(0, 0.25, 0, 0.9, 7), (1, 10.125, 0, 0.9, 7), (2, 0.875, 0, 0.9, 7)]
    gt = [(0, 0, 0, 0), (0, 10, 0, 1), (1, 10, 0, 1), (2, 0, 0, 0), (2, 1, 0, 1)]
    out = ev(pred, gt, 3)
    assert cnt(out) == dict(tp=3, fp=0, fn=2, ids=0, frag=0, npred=3)
    assert out["dist_sum1"][0] == 0.25 + 0.125 + 0.875
    assert np.isnan(out["tp_score"][[1, 4]]).all() and not np.isnan(out["tp_score"][[0, 2, 3]]).any()


def test_optimum_is_not_the_nearest_choice_per_row():
    """row 0's nearest prediction is column 0, which row 1 needs: two pairs at 1.5 + 0.5, not one at 1.0"""
    out = ev([(0, 1.0, 0, 0.9, 1), (0, -1.5, 0, 0.8, 2)], [(0, 0, 0, 0), (0, 1.5, 0, 1)], 1)
    assert cnt(out) == dict(tp=2, fp=0, fn=0, ids=0, frag=0, npred=2) and out["dist_sum1"][0] == 2.0
    assert out["tp_score"].tolist() == [np.float32(0.8), np.float32(0.9)]


def test_distance_equal_to_the_threshold_is_no_match():
    out = ev([(0, 2.0, 0, 0.9, 1)], [(0, 0, 0, 0)], 1)
    assert cnt(out) == dict(tp=0, fp=1, fn=1, ids=0, frag=0, npred=1)
    out = ev([(0, float(np.nextafter(np.float32(2.0), np.float32(0))), 0, 0.9, 1)], [(0, 0, 0, 0)], 1)
    assert cnt(out)["tp"] == 1


def test_thresholds_ties_and_slots_not_achieved():
    """four objects, three matched with scores 0.5, 0.5, 0.25, and a false box of score 0.5.  Recall 0.5 needs the
    second true positive: threshold 0.5, where score == threshold is active, ties included (TP 2, FP 1, FN 2):
    MOTA = 1 - 3 / 4, MOTAR = 1 - (3 - 0.5 * 4) / (0.5 * 4) = 0.5.  Recall 0.75 needs the third: threshold 0.25, all
    active.  Recall 1 needs a fourth: not achieved."""
    pred = [(0, 0.5, 0, 0.5, 1), (0, 10.5, 0, 0.5, 2), (0, 20.25, 0, 0.25, 3), (0, 50, 0, 0.5, 4)]
    gt = [(0, 0, 0, 0), (0, 10, 0, 1), (0, 20, 0, 2), (0, 30, 0, 3)]
    out = ev(pred, gt, 1, recall=(0.5, 0.75, 1.0))
    assert out["npos"].tolist() == [4] and out["thr"][0, :2].tolist() == [0.5, 0.25] and np.isnan(out["thr"][0, 2])
    assert out["counters"][0].tolist() == [[2, 1, 2, 0, 0, 3], [3, 1, 1, 0, 0, 4], [0, 0, 0, 0, 0, 0]]
    assert out["metrics"][0, 0].tolist() == [0.5, 0.25, 0.5, 0.5]
    assert out["metrics"][0, 1].tolist() == [0.75, 0.5, 1.25 / 3, 1 - (2 - 0.25 * 4) / (0.75 * 4)]
    assert out["metrics"][0, 2].tolist() == [0.0, 0.0, 2.0, 0.0]
    cs = dict(zip(R.CLASS_SUM, out["class_sum"][0]))
    assert cs["amota"] == (0.5 + (1 - 1 / 3.0) + 0.0) / 3 and cs["amotp"] == ((0.5 + 1.25 / 3) + 2.0) / 3
    assert (cs["best"], cs["mota"], cs["recall"], cs["tp"], cs["fp"], cs["fn"], cs["thr"]) == (1, 0.5, 0.75, 3, 1, 1, 0.25)


def test_one_recall_level():
    pred = [(0, 0.5, 0, 0.5, 1), (0, 10.5, 0, 0.75, 2)]
    out = ev(pred, [(0, 0, 0, 0), (0, 10, 0, 1)], 1, recall=R.recall_levels(1, 0.1))
    assert out["thr"].tolist() == [[0.5]] and out["metrics"][0, 0].tolist() == [1.0, 1.0, 0.5, 1.0]
    assert out["class_sum"][0, :4].tolist() == [1.0, 0.5, 0.0, 1.0]
    out = ev(pred[:1], [(0, 0, 0, 0), (0, 10, 0, 1)], 1, recall=R.recall_levels(1, 0.1))   # recall 1 is out of reach
    assert np.isnan(out["thr"][0, 0]) and out["class_sum"][0, :3].tolist() == [0.0, 2.0, -1.0]
    assert np.isnan(out["class_sum"][0, 3:]).all()
    # a MOTA tie goes to the lowest slot
    out = ev(pred, [(0, 0, 0, 0), (0, 10, 0, 1)], 1, recall=(0.9, 1.0))
    assert out["class_sum"][0, 2] == 0.0 and out["metrics"][0, :, 1].tolist() == [1.0, 1.0]


def test_class_without_ground_truth_and_class_without_predictions():
    pred = [(0, 0.5, 0, 0.5, 1, 0), (0, 5, 5, 0.5, 2, 1)]
    gt = [(0, 0, 0, 0, 0), (0, 9, 9, 1, 2)]
    out = ev(pred, gt, 1, C=3, recall=(0.5, 1.0))
    assert out["npos"].tolist() == [1, 0, 1]
    assert np.isnan(out["metrics"][1]).all() and np.isnan(out["class_sum"][1, [0, 1] + list(range(3, 12))]).all()
    assert out["class_sum"][1, 2] == -1 and out["counters1"][1].tolist() == [0, 1, 0, 0, 0, 1]
    assert out["counters1"][2].tolist() == [0, 0, 1, 0, 0, 0] and np.isnan(out["thr"][2]).all()
    assert out["class_sum"][2, :3].tolist() == [0.0, 2.0, -1.0] and out["class_sum"][0, :3].tolist() == [1.0, 0.5, 0.0]


def test_scenes_do_not_share_state():
    """the same instance id in two scenes: no switch across them; frames given out of order"""
    table = [(1, 0), (0, 1), (0, 0)]
    out = ev([(2, 0.5, 0, 0.9, 1), (1, 0.5, 0, 0.9, 1), (0, 0.5, 0, 0.9, 2)], [(0, 0, 0, 0), (1, 0, 0, 0), (2, 0, 0, 0)], 2,
             scenes=2, table=table)
    assert cnt(out) == dict(tp=3, fp=0, fn=0, ids=0, frag=0, npred=3)


def test_uniqueness_assertion_fires_on_a_tie():
    with pytest.raises(AssertionError, match="not unique"):
        ev([(0, 1.0, 0, 0.9, 1), (0, -1.0, 0, 0.9, 2)], [(0, 0, 0, 0)], 1)


@pytest.mark.parametrize("name", list(MC.CASES))
def test_seeded_cases_have_unique_optima(name):
    """the restatement alone passes its uniqueness assertion for every frame of every chain of the device cases"""
    inp, ref = MC.case(name)
    assert ref["counters1"][:, 0].sum() > 0


def test_cases_hold_the_shapes_the_device_paths_differ_at():
    g = {n: int(MC.case(n)[1]["run_max"][0]) for n in MC.CASES}
    h = {n: int(MC.case(n)[1]["run_max"][1]) for n in MC.CASES}
    assert (g["tiny"], h["tiny"], g["exact64"], h["exact64"]) == (1, 1, 64, 64)
    assert (g["edge64"], h["edge64"], g["big300"], h["big300"]) == (64, 65, 65, 300)
    inp, ref = MC.case("edge64")
    kept = R.kept_rows(inp["gt_box"], inp["gt_label"], inp["gt_frame"], inp["frame_tab"], len(inp["gt_label"]), num_scenes=1,
                       max_steps=2, class_range=inp["class_range"],
                       extra_ok=lambda i: 0 <= inp["gt_inst"][i] < inp["max_gt_tracks"])
    sizes = {}
    for k in kept:
        if k is not None:
            sizes[k] = sizes.get(k, 0) + 1
    assert set(sizes.values()) == {63, 64} and sum(k is None for k in kept) == 7
    sweep = MC.case("sweep")[1]
    assert (sweep["counters1"][:, 3] > 0).sum() >= 3 and (sweep["counters1"][:, 4] > 0).sum() >= 3   # switches, fragmentations
    assert np.isnan(sweep["thr"]).any() and (sweep["npos"] == 0).sum() == 1
    assert len(MC.CASES["sweep"]["classes"]) == 10 and MC.CASES["sweep"]["lengths"] == (1, 2, 30)


def test_moving_scene_with_truth_leaves_the_old_keys_byte_identical():
    from projects.mmdet3d_plugin import synthetic as S
    for kw in (dict(), dict(pad_to=40), dict(n_objects=5, frames=7, num_classes=2)):
        old, new = S.moving_scene(3, **kw), S.moving_scene(3, with_truth=True, **kw)
        assert len(old) == len(new)
        for a, b in zip(old, new):
            assert set(b) == set(a) | {"gt_boxes", "gt_labels", "gt_ids"}
            for k, v in a.items():
                w = b[k]
                assert type(v) is type(w)
                if isinstance(v, np.ndarray):
                    assert v.dtype == w.dtype and v.shape == w.shape and v.tobytes() == w.tobytes()
                else:
                    assert v == w
            n = len(b["gt_ids"])
            assert b["gt_boxes"].shape == (n, 9) and b["gt_boxes"].dtype == np.float32
            assert b["gt_labels"].dtype == np.int32 and b["gt_ids"].tolist() == list(range(n))
            seen = b["object"][b["object"] >= 0]
            assert np.abs(b["boxes"][b["object"] >= 0][:, :2] - b["gt_boxes"][seen, :2]).max() <= 0.2 + 1e-5
    assert math.isclose(new[1]["timestamp"], 0.1)
