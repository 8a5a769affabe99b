"""The cmt_mot_eval_* contract of include/cmt_hip.h as numpy loops: the restatement the device is compared with.

Arithmetic as the contract states it: float32 centre distances with every operation rounded on its own, float64 range
test, sums and metrics.  The assignment is ``scipy.optimize.linear_sum_assignment`` on the cost matrix.  cmt_lsap
solves the same matrix in float32 costs with float64 duals, so a frame whose optimum is not unique compares nothing:
``evaluate`` ASSERTS for every frame of every chain it solves that the optimum is unique with a margin (each chosen
admissible pair forbidden in turn gives fewer admissible pairs, or a total at least ``MARGIN`` metres larger).  That is
a condition on the test's inputs, not on the code under test.
"""
import math

import numpy as np
from scipy.optimize import linear_sum_assignment

BIG = np.float32(1.0e6)
MARGIN = 1e-3
COUNTERS = ("tp", "fp", "fn", "ids", "frag", "npred")
CLASS_SUM = ("amota", "amotp", "best", "mota", "motp", "recall", "tp", "fp", "fn", "ids", "frag", "thr")


def recall_levels(num_thresholds, min_recall):
    """r_k = min_recall + k (1 - min_recall) / (R - 1) in float64; r_0 = 1 for R = 1"""
    R = int(num_thresholds)
    if R == 1:
        return [1.0]
    return [float(min_recall) + k * (1.0 - float(min_recall)) / (R - 1) for k in range(R)]


def _solve(cost):
    """-> (sorted admissible pairs of the optimum, their number, their total in float64)"""
    if cost.shape[0] == 0 or cost.shape[1] == 0:
        return [], 0, 0.0
    r, c = linear_sum_assignment(cost.astype(np.float64))
    pairs = [(int(i), int(j)) for i, j in zip(r, c) if cost[i, j] < BIG]
    return pairs, len(pairs), float(sum(float(cost[i, j]) for i, j in pairs))


_UNIQUE = {}


def assert_unique(cost, pairs, count, total):
    key = (cost.shape, cost.tobytes())
    if key in _UNIQUE:
        return
    for i, j in pairs:
        c2 = cost.copy()
        c2[i, j] = BIG
        _, n2, t2 = _solve(c2)
        assert n2 < count or t2 >= total + MARGIN, \
            f"assignment optimum not unique with margin: pair {(i, j)} forbidden gives {n2} pairs, total {t2} vs {count}, {total}"
    _UNIQUE[key] = True


def kept_rows(box, label, frame, frame_tab, n, *, num_scenes, max_steps, class_range, extra_ok):
    """-> per row (scene, step, class) or None"""
    box = np.asarray(box, dtype=np.float32).reshape(len(label), -1)
    out = []
    tab = np.asarray(frame_tab, dtype=np.int64).reshape(-1, 2)
    C = len(class_range)
    for i in range(len(label)):
        c, f = int(label[i]), int(frame[i])
        ok = i < n and 0 <= c < C and 0 <= f < len(tab) and extra_ok(i)
        if ok:
            scene, step = int(tab[f, 0]), int(tab[f, 1])
            ok = 0 <= scene < num_scenes and 0 <= step < max_steps
        if ok:
            x, y = box[i, 0], box[i, 1]
            ok = bool(np.isfinite(x) and np.isfinite(y))
            if ok:
                x, y = np.float64(x), np.float64(y)
                ok = bool(np.sqrt(x * x + y * y) < np.float64(class_range[c]))
        out.append((scene, step, c) if ok else None)
    return out


def _clamp(n, cap):
    return cap if n is None else max(0, min(int(n), cap))


def evaluate(pred_box, pred_score, pred_label, pred_track, pred_frame, gt_box, gt_label, gt_frame, gt_inst, frame_tab, *,
             num_scenes, max_steps, class_range, dist_th, recall, max_gt_tracks, n_pred=None, n_gt=None,
             check_unique=True):
    """-> dict of numpy arrays named as native_eval.mot_eval's result"""
    N, G = len(pred_label), len(gt_label)
    pbox = np.asarray(pred_box, dtype=np.float32).reshape(N, -1)
    gbox = np.asarray(gt_box, dtype=np.float32).reshape(G, -1)
    score = np.asarray(pred_score, dtype=np.float32)
    track = np.asarray(pred_track, dtype=np.int64)
    inst = np.asarray(gt_inst, dtype=np.int64)
    C, R, S = len(class_range), len(recall), int(num_scenes)
    dth = [np.float32(v) for v in dist_th]
    kw = dict(num_scenes=S, max_steps=int(max_steps), class_range=class_range)
    pk = kept_rows(pbox, pred_label, pred_frame, frame_tab, _clamp(n_pred, N),
                   extra_ok=lambda i: track[i] >= 0 and bool(np.isfinite(score[i])), **kw)
    gk = kept_rows(gbox, gt_label, gt_frame, frame_tab, _clamp(n_gt, G),
                   extra_ok=lambda i: 0 <= inst[i] < max_gt_tracks, **kw)
    runs_p, runs_g = {}, {}
    for i, k in enumerate(pk):
        if k is not None:
            runs_p.setdefault(k, []).append(i)
    for i, k in enumerate(gk):
        if k is not None:
            runs_g.setdefault(k, []).append(i)
    npos = np.zeros(C, dtype=np.int32)
    for k in gk:
        if k is not None:
            npos[k[2]] += 1
    run_max = np.array([max([len(v) for v in runs_g.values()] + [0]), max([len(v) for v in runs_p.values()] + [0])],
                       dtype=np.int32)

    def chain(scene, c, thr, tp_score):
        """one chain -> (six counters, dist_sum); thr None: every prediction active (phase 1, writes tp_score)"""
        n = dict.fromkeys(COUNTERS, 0)
        dist = np.float64(0.0)
        m, lost = {}, {}
        for step in range(int(max_steps)):
            gr = runs_g.get((scene, step, c), [])
            pr = [j for j in runs_p.get((scene, step, c), []) if thr is None or score[j] >= thr]
            ng, na = len(gr), len(pr)
            gx, gy = gbox[gr, 0], gbox[gr, 1]
            px, py = pbox[pr, 0], pbox[pr, 1]
            dx, dy = gx[:, None] - px[None, :], gy[:, None] - py[None, :]
            xx, yy = dx * dx, dy * dy
            with np.errstate(invalid="ignore"):
                d = np.sqrt(xx + yy)
            assert d.dtype == np.float32
            adm = d < dth[c]
            rmatch, ctaken = [-1] * ng, [False] * na
            for i in range(ng):   # the sticky pass
                want = m.get(int(inst[gr[i]]), -1)
                if want < 0:
                    continue
                for j in range(na):
                    if not ctaken[j] and track[pr[j]] == want and adm[i, j]:
                        rmatch[i], ctaken[j] = j, True
                        break
            free = adm.copy()
            for i in range(ng):
                if rmatch[i] >= 0:
                    free[i, :] = False
            for j in range(na):
                if ctaken[j]:
                    free[:, j] = False
            cost = np.where(free, d, BIG).astype(np.float32)
            pairs, count, total = _solve(cost)
            if check_unique:
                assert_unique(cost, pairs, count, total)
            for i, j in pairs:
                rmatch[i] = j
            tp = 0
            for i in range(ng):   # the accounting
                o, j = int(inst[gr[i]]), rmatch[i]
                mo = m.get(o, -1)
                if j >= 0:
                    h = int(track[pr[j]])
                    tp += 1
                    dist = dist + np.float64(d[i, j])
                    n["ids"] += int(mo >= 0 and mo != h)
                    n["frag"] += int(lost.get(o, False))
                    m[o], lost[o] = h, False
                else:
                    lost[o] = mo >= 0
                if tp_score is not None:
                    tp_score[gr[i]] = score[pr[j]] if j >= 0 else np.float32("nan")
            n["tp"] += tp
            n["fn"] += ng - tp
            n["fp"] += na - tp
            n["npred"] += na
        return [n[k] for k in COUNTERS], dist

    tp_score = np.full(G, np.nan, dtype=np.float32)
    counters1 = np.zeros((C, 6), dtype=np.int64)
    dist_sum1 = np.zeros(C, dtype=np.float64)
    for c in range(C):
        for s in range(S):
            n, dist = chain(s, c, None, tp_score)
            counters1[c] += n
            dist_sum1[c] = dist_sum1[c] + dist

    thr = np.full((C, R), np.nan, dtype=np.float32)
    for c in range(C):
        sc = [tp_score[g] for g in range(G) if gk[g] is not None and gk[g][2] == c and not np.isnan(tp_score[g])]
        sc = sorted(sc, reverse=True)
        for k in range(R):
            need = max(1, int(math.ceil(float(recall[k]) * float(npos[c]))))
            if npos[c] > 0 and need <= len(sc):
                thr[c, k] = sc[need - 1]

    counters = np.zeros((C, R, 6), dtype=np.int64)
    dist_sum = np.zeros((C, R), dtype=np.float64)
    metrics = np.zeros((C, R, 4), dtype=np.float64)
    class_sum = np.full((C, 12), np.nan, dtype=np.float64)
    nan = float("nan")
    for c in range(C):
        n_, th = float(npos[c]), float(dth[c])
        ok = [not np.isnan(thr[c, k]) for k in range(R)]
        for k in range(R):
            if ok[k]:
                for s in range(S):
                    n, dist = chain(s, c, thr[c, k], None)
                    counters[c, k] += n
                    dist_sum[c, k] = dist_sum[c, k] + dist
            tp, fp, fn, ids = (int(v) for v in counters[c, k, :4])
            if npos[c] == 0:
                metrics[c, k] = nan
            elif not ok[k]:
                metrics[c, k] = [0.0, 0.0, th, 0.0]
            else:
                e = float(ids + fp + fn)
                rec = float(tp) / n_
                mota = 1.0 - e / n_
                motp, motar = th, 0.0
                if tp > 0:
                    motp = float(dist_sum[c, k]) / float(tp)
                    miss = (1.0 - rec) * n_
                    den = rec * n_
                    motar = max(0.0, 1.0 - (e - miss) / den)
                metrics[c, k] = [rec, mota, motp, motar]
        best = -1
        sa = sp = 0.0
        for k in range(R):
            sa = sa + metrics[c, k, 3]
            sp = sp + metrics[c, k, 2]
            if ok[k] and npos[c] > 0 and (best < 0 or metrics[c, k, 1] > metrics[c, best, 1]):
                best = k
        if npos[c] > 0:
            class_sum[c, 0], class_sum[c, 1] = sa / float(R), sp / float(R)
        class_sum[c, 2] = float(best)
        if best >= 0:
            class_sum[c, 3:6] = [metrics[c, best, 1], metrics[c, best, 2], metrics[c, best, 0]]
            class_sum[c, 6:11] = counters[c, best, :5]
            class_sum[c, 11] = float(thr[c, best])
    return dict(npos=npos, run_max=run_max, tp_score=tp_score, thr=thr, counters=counters, dist_sum=dist_sum,
                metrics=metrics, class_sum=class_sum, counters1=counters1, dist_sum1=dist_sum1)
