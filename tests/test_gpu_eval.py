"""cmt_det_eval_* / DetectionEvaluator on the device against tests/_eval_ref.py (the contract of cmt_hip.h in numpy).

Every case is built so that each decision is the same whatever the order of a sum: box centres are multiples of
2^-4 m within +-64 m, so dx^2 + dy^2 is exact in float64, the squares of the thresholds and ranges are exact and a
correctly rounded square root decides alike on both sides.  Held to two things:
  * tp, match_gt and npos equal exactly;
  * every curve value, AP, TP error and NDS within 1e-9 * max(1, |value|): the only freedom is the order of the
    float64 cumulative sums over at most 2^20 terms (2^20 * 2^-53 = 1.2e-10, with an 8x margin).
"""
import functools
import json
import math
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _eval_ref as R  # noqa: E402

from conftest import PKG  # noqa: E402

pytestmark = pytest.mark.gpu


@pytest.fixture(autouse=True)
def _device(dev):
    return dev


TOL = 1e-9
RANGES = (50.0, 40.0, 50.0)
PERIODS = (2 * math.pi, math.pi, 2 * math.pi)
THS = (0.5, 1.0, 2.0, 4.0)
CFG = dict(class_range=RANGES, yaw_period=PERIODS, dist_ths=THS, dist_th_tp=2.0, min_recall=0.1, min_precision=0.1)
STEP = 1.0 / 16.0


class Rows:
    """predictions and ground truth as plain lists, in arrival / annotation order"""

    def __init__(self, seed):
        self.rng = np.random.RandomState(seed)
        self.p, self.g = [], []

    def _rest(self, dims=None, yaw=None, vel=None):
        r = self.rng
        dims = r.uniform(0.5, 4.0, 3) if dims is None else dims
        yaw = r.uniform(-math.pi, math.pi) if yaw is None else yaw
        vel = r.normal(size=2) if vel is None else vel
        return [r.uniform(-2, 2)] + list(dims) + [yaw] + list(vel)

    def pred(self, sample, label, score, x, y, **kw):
        self.p.append(([x, y] + self._rest(**kw), score, label, sample))
        return len(self.p) - 1

    def gt(self, sample, label, x, y, num_pts=-1, **kw):
        self.g.append(([x, y] + self._rest(**kw), label, sample, num_pts))
        return len(self.g) - 1

    def grid(self, lo=-36.0, hi=36.0):
        return float(self.rng.randint(int(lo / STEP), int(hi / STEP) + 1)) * STEP

    def fill(self, sample, gt_per_class, n_pred, scores, fp_rate=0.3):
        """gt_per_class boxes per class and n_pred predictions for one sample: jittered ground truth and false
        positives, scores drawn from ``scores`` (a list: ties) or distinct when None"""
        mine = []
        for c, n in enumerate(gt_per_class):
            for _ in range(n):
                x, y = self.grid(), self.grid()
                self.gt(sample, c, x, y)
                mine.append((c, x, y))
        for _ in range(n_pred):
            sc = float(self.rng.choice(scores)) if scores is not None else float(np.float32(self.rng.uniform(0.01, 1)))
            if mine and self.rng.rand() > fp_rate:
                c, x, y = mine[self.rng.randint(len(mine))]
                x += self.rng.randint(-40, 41) * STEP
                y += self.rng.randint(-40, 41) * STEP
                x, y = min(max(x, -64.0), 64.0), min(max(y, -64.0), 64.0)
            else:
                c, x, y = self.rng.randint(len(gt_per_class)), self.grid(-44, 44), self.grid(-44, 44)
            self.pred(sample, c, sc, x, y)

    def arrays(self):
        pb = np.array([r[0] for r in self.p], dtype=np.float32).reshape(-1, 9)
        gb = np.array([r[0] for r in self.g], dtype=np.float32).reshape(-1, 9)
        col = lambda rows, k, dt: np.array([r[k] for r in rows], dtype=dt)  # noqa: E731
        return dict(pred_boxes=pb, pred_scores=col(self.p, 1, np.float32), pred_labels=col(self.p, 2, np.int32),
                    pred_samples=col(self.p, 3, np.int32), gt_boxes=gb, gt_labels=col(self.g, 1, np.int32),
                    gt_samples=col(self.g, 2, np.int32), gt_num_pts=col(self.g, 3, np.int32))


TIES = [k / 64.0 for k in range(8, 24)]


def case_lanes():
    """ground truth per (sample, class) 63, 64, 65, 130, 1, 0; predictions per sample 500, 65, 64; 3 samples, the
    last without ground truth"""
    r = Rows(1)
    r.fill(0, (63, 64, 65), 500, TIES)
    r.fill(1, (130, 1, 0), 65, None)
    r.fill(2, (0, 0, 0), 64, TIES)
    return r.arrays(), 3


def case_sparse():
    """70 samples, few boxes each; samples without ground truth, without predictions, with one of each; equal scores
    within a sample and across samples"""
    r = Rows(2)
    preds = [0, 1, 5, 9, 2, 0, 17]
    for s in range(70):
        gts = (0, 0, 0) if s % 5 == 0 else tuple(int(v) for v in r.rng.randint(0, 4, 3))
        r.fill(s, gts, preds[s % len(preds)], TIES if s % 2 else TIES[:3])
    return r.arrays(), 70


def case_single():
    """one sample, one ground-truth box, one prediction on it"""
    r = Rows(3)
    r.gt(0, 0, 1.0, 2.0)
    r.pred(0, 0, 0.5, 1.25, 2.0)
    return r.arrays(), 1


def case_edges():
    """the hand-made decisions: ties, thresholds, range, filters, per-threshold taken state, NaN velocities"""
    r = Rows(4)
    nanv = [float("nan"), float("nan")]
    # sample 0, class 0: two ground-truth boxes equidistant from a prediction: the lowest index wins
    r.gt(0, 0, 10.0, 1.0)
    r.gt(0, 0, 10.0, -1.0)
    r.pred(0, 0, 0.9, 10.0, 0.0)
    # sample 1, class 0: distance exactly equal to each threshold (no match at that threshold)
    for k, th in enumerate(THS):
        r.gt(1, 0, -20.0 + 10.0 * k, 5.0)
        r.pred(1, 0, 0.8 - 0.1 * k, -20.0 + 10.0 * k + th, 5.0)
    # sample 2: a box exactly on its class range (dropped) and one step inside (kept), ground truth and predictions
    r.gt(2, 1, 40.0, 0.0)
    r.gt(2, 1, 40.0 - STEP, 0.0)
    r.pred(2, 1, 0.7, 0.0, 40.0)
    r.pred(2, 1, 0.7, 40.0 - STEP, 0.25)
    r.gt(2, 0, 30.0, 40.0)             # norm exactly 50
    r.pred(2, 0, 0.6, 30.0, 40.0 - STEP)
    # sample 3: num_pts == 0 dropped, labels -1 and C ignored, NaN centres dropped
    r.gt(3, 0, 5.0, 5.0, num_pts=0)
    r.gt(3, 0, 6.0, 5.0, num_pts=3)
    r.gt(3, -1, 5.0, 5.0)
    r.gt(3, 3, 5.0, 5.0)
    r.gt(3, 0, float("nan"), 5.0)
    r.pred(3, 0, 0.95, 5.0, 5.0)
    r.pred(3, -1, 0.99, 6.0, 5.0)
    r.pred(3, 3, 0.99, 6.0, 5.0)
    r.pred(3, 0, 0.99, float("nan"), 5.0)
    r.pred(7, 0, 0.99, 6.0, 5.0)       # sample outside [0, S)
    # sample 4, class 0: the nearest ground truth is taken at one threshold but not at a tighter one
    r.gt(4, 0, 0.0, 0.0)
    r.gt(4, 0, 3.0, 0.0)
    r.pred(4, 0, 0.9, 0.75, 0.0)
    r.pred(4, 0, 0.8, 0.25, 0.0)
    # class 1 (period pi): orientation differences around the wrap, NaN velocity for every prediction of the class
    for k, dyaw in enumerate((0.1, math.pi / 2 + 0.01, math.pi - 0.01, 3.0, -2.0)):
        r.gt(5, 1, 4.0 * k, 8.0, yaw=0.3)
        r.pred(5, 1, 0.5 + 0.05 * k, 4.0 * k + 0.25, 8.0, yaw=0.3 - dyaw, vel=nanv)
    # class 2: NaN velocities for some predictions; the first match in visiting order is one of them
    for k in range(6):
        r.gt(6, 2, 4.0 * k, -8.0)
        r.pred(6, 2, 0.9 - 0.1 * k, 4.0 * k + 0.25 * (k % 3), -8.0, vel=nanv if k in (0, 3) else None)
    # -0.0 and +0.0 scores are equal: the index decides
    r.gt(5, 0, -10.0, -10.0)
    r.pred(5, 0, -0.0, -10.0, -10.25)
    r.pred(5, 0, 0.0, -10.0, -9.75)
    return r.arrays(), 7


def _fix_class1_velocities(a):
    """every prediction of class 1 gets NaN velocities (the class's vel_err curve is all ones)"""
    a["pred_boxes"][a["pred_labels"] == 1, 7:9] = np.nan
    return a


def case_edges_fixed():
    a, S = case_edges()
    return _fix_class1_velocities(a), S


def case_empty_classes():
    """class 1 absent from the ground truth (npos == 0) but predicted; class 2 with ground truth and predictions that
    never match; class 0 ordinary"""
    r = Rows(5)
    r.fill(0, (4, 0, 0), 9, None)
    for k in range(5):
        r.pred(0, 1, 0.3 + 0.1 * k, 2.0 * k, 3.0)
        r.gt(0, 2, 2.0 * k, -20.0)
        r.pred(0, 2, 0.3 + 0.1 * k, 2.0 * k, 20.0)
    return r.arrays(), 1


def case_chunks():
    """more than 2048 predictions and more than 2048 matches in one class (the scans' second chunk), 280 ground-truth
    boxes per (sample, class) (five lane chunks), 300 predictions per sample"""
    r = Rows(6)
    for s in range(9):
        mine = []
        for _ in range(280):
            x, y = r.grid(-30, 30), r.grid(-30, 30)
            r.gt(s, 0, x, y)
            mine.append((x, y))
        order = r.rng.permutation(300)
        for k in order:
            sc = float(np.float32(r.rng.uniform(0.01, 1)))
            if k < 280:
                r.pred(s, 0, sc, mine[k][0] + r.rng.randint(-4, 5) * STEP, mine[k][1] + r.rng.randint(-4, 5) * STEP,
                       vel=[float("nan")] * 2 if k % 7 == 0 else None)
            else:
                r.pred(s, int(r.rng.randint(3)), sc, r.grid(-44, 44), r.grid(-44, 44))
    return r.arrays(), 9


CASES = dict(chunks=case_chunks, lanes=case_lanes, sparse=case_sparse, single=case_single, edges=case_edges_fixed,
             empty_classes=case_empty_classes)


@functools.lru_cache(maxsize=None)
def inputs(name):
    a, S = CASES[name]()
    return a, S


@functools.lru_cache(maxsize=None)
def reference(name):
    a, S = inputs(name)
    return R.evaluate(**a, num_samples=S, **CFG)


def to_dev(a):
    return {k: torch.from_numpy(v).cuda() for k, v in a.items()}


def run_device(a, S, **kw):
    from projects.mmdet3d_plugin import native_eval as NE
    d = to_dev(a)
    out = NE.det_eval(d["pred_boxes"], d["pred_scores"], d["pred_labels"], d["pred_samples"], d["gt_boxes"],
                      d["gt_labels"], d["gt_samples"], d["gt_num_pts"], num_samples=S, **CFG, **kw)
    torch.cuda.synchronize()
    return {k: v.cpu().numpy() for k, v in out.items()}


def close(got, want, what):
    got, want = np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64)
    assert got.shape == want.shape, what
    assert np.array_equal(np.isnan(got), np.isnan(want)), f"{what}: NaN pattern differs"
    m = ~np.isnan(want)
    err = np.abs(got[m] - want[m]) / np.maximum(1.0, np.abs(want[m]))
    worst = float(err.max()) if err.size else 0.0
    print(f"{what}: max scaled error {worst:.3e}")
    assert worst <= TOL, f"{what}: max scaled error {worst:.3e} > {TOL}"


def check(out, ref, n=None):
    C, T = len(RANGES), len(THS)
    n = ref["tp"].shape[1] if n is None else n
    assert np.array_equal(out["npos"], ref["npos"]), (out["npos"], ref["npos"])
    assert np.array_equal(out["tp"][:, :n], ref["tp"][:, :n])
    assert np.array_equal(out["match_gt"][:, :n], ref["match_gt"][:, :n])
    close(out["err"][:, :, :n], ref["err"][:, :, :n], "err")
    names = ("recall", "precision", "confidence") + R.ERR_NAMES
    for c in range(C):
        for t in range(T):
            for i, k in enumerate(names):
                close(out["md"][c, t, i], ref["md"][(c, t)][k], f"md[{c}][{t}].{k}")
    close(out["ap"], ref["ap"], "ap")
    close(out["tp_err"], ref["tp_err"], "tp_err")
    s = R.summary(out["ap"], out["tp_err"], 5.0)
    close(s["nd_score"], ref["summary"]["nd_score"], "nd_score")
    close(s["mean_ap"], ref["summary"]["mean_ap"], "mean_ap")


@pytest.mark.parametrize("name", sorted(CASES))
def test_matches_reference(name):
    a, S = inputs(name)
    check(run_device(a, S), reference(name))


def test_cases_cover_what_they_claim():
    """the hand-made case really holds the decisions it is there for (read from the reference's result)"""
    a, _ = inputs("edges")
    ref = reference("edges")
    tp, mg = ref["tp"], ref["match_gt"]
    assert mg[2, 0] == 0 and mg[3, 0] == 0                 # equidistant at 1 m: the lowest index
    for k in range(4):                                     # distance == threshold k: no match at k, a match above
        assert tp[k, 1 + k] == 0 and all(tp[j, 1 + k] == 1 for j in range(k + 1, 4))
    lab, smp = a["pred_labels"], a["pred_samples"]
    on = [i for i in range(len(lab)) if smp[i] == 2]
    assert [int(mg[3, i]) >= 0 for i in on] == [False, True, False]   # on the range: dropped (a box and a ground truth); inside: kept
    i0 = [i for i in range(len(lab)) if smp[i] == 4]
    assert tp[:, i0[0]].tolist() == [0, 1, 1, 1] and tp[:, i0[1]].tolist() == [1, 0, 0, 1]   # per-threshold taken
    assert np.all(ref["md"][(1, 2)]["vel_err"] == 1.0) and ref["md"][(1, 2)]["confidence"].max() > 0
    e = reference("empty_classes")
    assert e["npos"][1] == 0 and e["npos"][2] == 5 and e["tp"][:, inputs("empty_classes")[0]["pred_labels"] == 2].sum() == 0
    assert 0.0 < reference("lanes")["summary"]["mean_ap"] < 1.0
    assert reference("chunks")["tp"][0].sum() > 2048 and (inputs("chunks")[0]["pred_labels"] == 0).sum() > 2048


def test_buffers_guarded_and_device_counts():
    """capacity-sized inputs with device counts below the capacity, outputs and workspace pre-filled with NaN /
    sentinels, guard tails behind every buffer untouched"""
    from projects.mmdet3d_plugin import native_eval as NE
    a, S = inputs("sparse")
    ref = reference("sparse")
    n, g = len(a["pred_scores"]), len(a["gt_labels"])
    pad_n, pad_g, guard = 37, 11, 64
    rng = np.random.RandomState(9)
    big = dict(a)
    # rows beyond the counts look like valid, matching boxes: they must not be read as such
    big["pred_boxes"] = np.concatenate([a["pred_boxes"], a["pred_boxes"][:pad_n]])
    big["pred_scores"] = np.concatenate([a["pred_scores"], np.full(pad_n, 2.0, np.float32)])
    big["pred_labels"] = np.concatenate([a["pred_labels"], a["pred_labels"][:pad_n]])
    big["pred_samples"] = np.concatenate([a["pred_samples"], a["pred_samples"][:pad_n]])
    big["gt_boxes"] = np.concatenate([a["gt_boxes"], a["gt_boxes"][:pad_g]])
    for k in ("gt_labels", "gt_samples", "gt_num_pts"):
        big[k] = np.concatenate([a[k], a[k][:pad_g]])
    d = to_dev(big)
    N, G, C, T = n + pad_n, g + pad_g, len(RANGES), len(THS)
    shapes = dict(tp=((T, N), torch.uint8), match_gt=((T, N), torch.int32), err=((T, 4, N), torch.float64),
                  npos=((C,), torch.int32), md=((C, T, 7, 101), torch.float64), ap=((C, T), torch.float64),
                  tp_err=((C, 4), torch.float64))
    fill = {torch.uint8: 0xA5, torch.int32: -77777, torch.float64: float("nan")}
    flat, out = {}, {}
    for k, (shape, dt) in shapes.items():
        numel = int(np.prod(shape))
        flat[k] = torch.full((numel + guard,), fill[dt], dtype=dt, device="cuda")
        out[k] = flat[k][:numel].view(shape)
    need = NE.workspace_bytes(N, G, S, C, T)
    ws = torch.full((need + guard,), 0xA5, dtype=torch.uint8, device="cuda")
    res = NE.det_eval(d["pred_boxes"], d["pred_scores"], d["pred_labels"], d["pred_samples"], d["gt_boxes"],
                      d["gt_labels"], d["gt_samples"], d["gt_num_pts"], num_samples=S, **CFG,
                      n_pred=torch.tensor([n], dtype=torch.int32, device="cuda"),
                      n_gt=torch.tensor([g], dtype=torch.int32, device="cuda"), out=out, workspace=ws[:need])
    torch.cuda.synchronize()
    got = {k: v.cpu().numpy() for k, v in res.items()}
    check(got, ref, n=n)
    assert (got["tp"][:, n:] == 0).all() and (got["match_gt"][:, n:] == -1).all() and np.isnan(got["err"][:, :, n:]).all()
    assert not np.isnan(got["md"]).any() and not np.isnan(got["ap"]).any() and not np.isnan(got["tp_err"]).any()
    for k, (shape, dt) in shapes.items():
        tail = flat[k][int(np.prod(shape)):].cpu()
        assert bool(torch.isnan(tail).all()) if dt == torch.float64 else bool((tail == fill[dt]).all()), k
    assert bool((ws[need:] == 0xA5).all())
    del rng


def test_two_runs_bit_equal_and_sample_permutation():
    a, S = inputs("lanes")
    one, two = run_device(a, S), run_device(a, S)
    for k in one:
        assert one[k].tobytes() == two[k].tobytes(), k
    # distinct scores: permuting the samples changes nothing in the metrics
    r = Rows(11)
    for s in range(5):
        r.fill(s, (3, 2, 4), 40, None)
    b = r.arrays()
    assert len(np.unique(b["pred_scores"])) == len(b["pred_scores"])
    perm = np.array([3, 0, 4, 1, 2])
    po = np.argsort(perm[b["pred_samples"]], kind="stable")
    go = np.argsort(perm[b["gt_samples"]], kind="stable")
    c = {k: (v[po] if k.startswith("pred") else v[go]) for k, v in b.items()}
    c["pred_samples"], c["gt_samples"] = perm[b["pred_samples"]][po].astype(np.int32), perm[b["gt_samples"]][go].astype(np.int32)
    x, y = run_device(b, 5), run_device(c, 5)
    for k in ("md", "ap", "tp_err", "npos"):
        assert x[k].tobytes() == y[k].tobytes(), k


def _evaluator(S):
    from projects.mmdet3d_plugin.core.evaluation import DetEvalConfig, DetectionEvaluator
    cfg = DetEvalConfig(class_names=("a", "b", "c"), **CFG)
    return DetectionEvaluator(cfg, S, "cuda")


def _frames(a, S, M):
    """the case as padded [S, M, ...] frames with counts, and per-frame ground truth"""
    boxes = np.zeros((S, M, 9), np.float32)
    scores, labels = np.zeros((S, M), np.float32), np.zeros((S, M), np.int32)
    count = np.zeros(S, np.int32)
    for i in range(len(a["pred_scores"])):
        s = a["pred_samples"][i]
        if 0 <= s < S:
            boxes[s, count[s]], scores[s, count[s]], labels[s, count[s]] = a["pred_boxes"][i], a["pred_scores"][i], a["pred_labels"][i]
            count[s] += 1
    # rows behind the count look like perfect detections
    gt = []
    for s in range(S):
        m = a["gt_samples"] == s
        gt.append((a["gt_boxes"][m], a["gt_labels"][m], a["gt_num_pts"][m]))
        k = min(M - count[s], int(m.sum()))
        if k:
            boxes[s, count[s]:count[s] + k] = a["gt_boxes"][m][:k]
            scores[s, count[s]:count[s] + k] = 3.0
            labels[s, count[s]:count[s] + k] = a["gt_labels"][m][:k]
    return boxes, scores, labels, count, gt


def test_evaluator_incremental_and_summary():
    """DetectionEvaluator on padded frames with device counts: three add() calls equal one, and the summary, detail
    and curves equal the reference"""
    from projects.mmdet3d_plugin.core.evaluation import summarize
    a, S = inputs("sparse")
    ref = reference("sparse")
    boxes, scores, labels, count, gt = _frames(a, S, 20)
    cu = lambda v: torch.from_numpy(np.ascontiguousarray(v)).cuda()  # noqa: E731

    def feed(ev, lo, hi):
        ev.add(cu(boxes[lo:hi]), cu(scores[lo:hi]), cu(labels[lo:hi]), cu(count[lo:hi]),
               [cu(g[0]) for g in gt[lo:hi]], [cu(g[1]) for g in gt[lo:hi]], [cu(g[2]) for g in gt[lo:hi]])

    one, three = _evaluator(S), _evaluator(S)
    feed(one, 0, S)
    feed(three, 0, 1)
    feed(three, 1, 33)
    feed(three, 33, S)
    m1, m3 = one.compute(), three.compute()
    assert json.dumps(m1, sort_keys=True) == json.dumps(m3, sort_keys=True)
    want = ref["summary"]
    close(m1["nd_score"], want["nd_score"], "nd_score")
    close(m1["mean_ap"], want["mean_ap"], "mean_ap")
    for k in R.TP_METRICS:
        close(m1["tp_errors"][k], want["tp_errors"][k], k)
    for c, name in enumerate("abc"):
        close([m1["label_aps"][name][t] for t in THS], ref["ap"][c], f"label_aps[{name}]")
        close([m1["label_tp_errors"][name][k] for k in R.ERR_NAMES], ref["tp_err"][c], f"label_tp_errors[{name}]")
    md = one.metric_data()
    close(md["b:2.0"]["precision"], ref["md"][(1, 2)]["precision"], "metric_data")
    d = one.detail()
    assert d["object/nds"] == m1["nd_score"] and d["object/map"] == m1["mean_ap"]
    assert d["object/a_ap_dist_0.5"] == float("{:.4f}".format(m1["label_aps"]["a"][0.5]))
    assert set(("object/mATE", "object/mASE", "object/mAOE", "object/mAVE", "object/c_vel_err")) <= set(d)
    one.reset()
    with pytest.raises(ValueError):
        one.compute()
    assert summarize(one.cfg, ref["ap"], ref["tp_err"])["nd_score"] == pytest.approx(want["nd_score"], abs=1e-12)


def test_cli_eval_nds(tmp_path, capsys):
    """tools/test.py --eval bbox nds: the unchanged statistics line, then the summary, which equals the reference
    on the dumped boxes and the frame-seeded synthetic ground truth (random weights: the boxes hardly ever match, so
    this checks the plumbing and the "no predictions" blocks; the cases above check the arithmetic)"""
    import importlib.util
    spec = importlib.util.spec_from_file_location("cmt_test_cli", os.path.join(PKG, "tools", "test.py"))
    cli = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(cli)
    out = tmp_path / "res.json"
    base = ["cmt_lidar_nus", "--synthetic", "--num-query", "32", "--num-layers", "1", "--frames", "3",
            "--out", str(out)]
    assert cli.main(base + ["--eval", "bbox"]) == 0
    plain = capsys.readouterr().out.strip().splitlines()
    assert cli.main(base + ["--eval", "bbox", "nds"]) == 0
    lines = capsys.readouterr().out.strip().splitlines()
    assert len(lines) == len(plain) + 1
    s0, s1 = json.loads(plain[-1]), json.loads(lines[-2])
    assert s0.pop("metric") == ["bbox"] and s1.pop("metric") == ["bbox", "nds"]
    s0.pop("seconds"), s1.pop("seconds")
    assert s0 == s1
    got = json.loads(lines[-1])
    dump = json.loads(out.read_text())
    names = dump["class_names"]
    cfg = cli.eval_config(names)
    pb, ps, pl, psm, gb, gl, gs = [], [], [], [], [], [], []
    for f in dump["frames"]:
        k = len(f["scores_3d"])
        pb += f["boxes_3d"]; ps += f["scores_3d"]; pl += f["labels_3d"]; psm += [f["frame"]] * k  # noqa: E702
        b, l = cli.frame_ground_truth(f["frame"], 0, cli.eval_pc_range("cmt_lidar_nus"), len(names))
        b = b.numpy().copy()
        if cfg.gt_velocity_zero:
            b[:, 7:9] = 0
        gb += b.tolist(); gl += l.tolist(); gs += [f["frame"]] * len(l)  # noqa: E702
    ref = R.evaluate(np.array(pb, np.float32).reshape(-1, 9), ps, pl, psm, np.array(gb, np.float32), gl, gs,
                     [-1] * len(gl), num_samples=3, class_range=cfg.class_range, yaw_period=cfg.yaw_period,
                     dist_ths=cfg.dist_ths, dist_th_tp=cfg.dist_th_tp)
    assert got["metric"] == "nds" and got["frames"] == 3
    close(got["nd_score"], ref["summary"]["nd_score"], "cli nd_score")
    close(got["mean_ap"], ref["summary"]["mean_ap"], "cli mean_ap")
    for k in R.TP_METRICS:
        close(got["tp_errors"][k], ref["summary"]["tp_errors"][k], "cli " + k)
