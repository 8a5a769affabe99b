"""Plain numpy float64 restatement of the detection-evaluation contract of include/cmt_hip.h (cmt_det_eval_*):
Python loops, dictionaries per sample and the real numpy.interp, in the style of the evaluator the contract
restates.  The tests compare the device results with this."""
import math

import numpy as np

ERR_NAMES = ("trans_err", "vel_err", "scale_err", "orient_err")
TP_METRICS = ("trans_err", "scale_err", "orient_err", "vel_err")
NELEM = 101


def pymod(a, p):
    return float(a) % float(p)


def orient_err(yaw_gt, yaw_pred, period):
    diff = pymod((float(yaw_gt) - float(yaw_pred)) + period / 2, period) - period / 2
    if diff > np.pi:
        diff = diff - (2 * np.pi)
    return abs(diff)


def scale_err(g, p):
    sa = np.array([float(v) for v in g], dtype=np.float64)
    sr = np.array([float(v) for v in p], dtype=np.float64)
    m = np.minimum(sa, sr)
    vg, vp, i = (sa[0] * sa[1]) * sa[2], (sr[0] * sr[1]) * sr[2], (m[0] * m[1]) * m[2]
    return 1.0 - i / ((vg + vp) - i)


def dist2d(ax, ay, bx, by):
    dx, dy = float(ax) - float(bx), float(ay) - float(by)
    return math.sqrt(dx * dx + dy * dy)


def cummean(x):
    x = np.asarray(x, dtype=np.float64)
    if np.isnan(x).sum() == len(x):
        return np.ones(len(x))
    s = np.nancumsum(x)
    n = np.cumsum(~np.isnan(x))
    return np.divide(s, n, out=np.zeros_like(s), where=n != 0)


def no_predictions():
    md = {"recall": np.linspace(0, 1, NELEM), "precision": np.zeros(NELEM), "confidence": np.zeros(NELEM)}
    md.update({k: np.ones(NELEM) for k in ERR_NAMES})
    return md


def calc_ap(md, min_recall, min_precision):
    prec = np.copy(md["precision"])[round(100 * min_recall) + 1:]
    prec -= min_precision
    prec[prec < 0] = 0
    return float(np.mean(prec)) / (1.0 - min_precision)


def calc_tp(md, min_recall, name):
    first = round(100 * min_recall) + 1
    nz = np.nonzero(md["confidence"])[0]
    last = 0 if len(nz) == 0 else nz[-1]
    if last < first:
        return 1.0
    return float(np.mean(md[name][first:last + 1]))


def evaluate(pred_boxes, pred_scores, pred_labels, pred_samples, gt_boxes, gt_labels, gt_samples, gt_num_pts, *,
             num_samples, class_range, yaw_period, dist_ths, dist_th_tp, min_recall=0.1, min_precision=0.1,
             mean_ap_weight=5.0, n_pred=None, n_gt=None):
    """-> dict(tp [T, N] uint8, match_gt [T, N], err [T, 4, N], npos [C], md {(c, t): curves}, ap [C, T],
    tp_err [C, 4] (columns ERR_NAMES), summary)"""
    pb = np.asarray(pred_boxes, dtype=np.float32).reshape(-1, 9)
    ps = np.asarray(pred_scores, dtype=np.float32)
    pl, psm = np.asarray(pred_labels), np.asarray(pred_samples)
    gb = np.asarray(gt_boxes, dtype=np.float32).reshape(-1, 9)
    gl, gsm, gnp = np.asarray(gt_labels), np.asarray(gt_samples), np.asarray(gt_num_pts)
    N, G = len(pb), len(gb)
    n_pred = N if n_pred is None else min(max(int(n_pred), 0), N)
    n_gt = G if n_gt is None else min(max(int(n_gt), 0), G)
    C, T, S = len(class_range), len(dist_ths), int(num_samples)

    def kept(box, label, sample):
        if not (0 <= label < C and 0 <= sample < S):
            return False
        return dist2d(box[0], box[1], 0.0, 0.0) < class_range[label]   # NaN compares false

    # per sample, in row order
    preds = {s: [] for s in range(S)}
    for i in range(n_pred):
        if kept(pb[i], int(pl[i]), int(psm[i])):
            preds[int(psm[i])].append(i)
    gts = {s: [] for s in range(S)}
    for g in range(n_gt):
        if kept(gb[g], int(gl[g]), int(gsm[g])) and int(gnp[g]) != 0:
            gts[int(gsm[g])].append(g)

    tp_out = np.zeros((T, N), dtype=np.uint8)
    match_out = np.full((T, N), -1, dtype=np.int64)
    err_out = np.full((T, 4, N), np.nan)
    npos_out = np.zeros(C, dtype=np.int64)
    md_out = {}
    for c in range(C):
        npos = sum(1 for s in gts for g in gts[s] if int(gl[g]) == c)
        npos_out[c] = npos
        # the class's kept predictions by rising row: the position in this list is the "list index"
        plist = sorted(i for s in range(S) for i in preds[s] if int(pl[i]) == c)
        confs = [float(ps[i]) + 0.0 for i in plist]
        sortind = [i for (v, i) in sorted((v, i) for (i, v) in enumerate(confs))][::-1]
        for t, th in enumerate(dist_ths):
            taken = set()
            tp, conf = [], []
            match = {k: [] for k in ERR_NAMES}
            mconf = []
            for ind in sortind:
                i = plist[ind]
                s = int(psm[i])
                best, best_g = np.inf, None
                for g in gts[s]:
                    if int(gl[g]) == c and g not in taken:
                        d = dist2d(gb[g][0], gb[g][1], pb[i][0], pb[i][1])
                        if d < best:
                            best, best_g = d, g
                conf.append(confs[ind])
                if best < th:
                    taken.add(best_g)
                    tp.append(1)
                    e = (best,
                         dist2d(pb[i][7], pb[i][8], gb[best_g][7], gb[best_g][8]),
                         scale_err(gb[best_g][3:6], pb[i][3:6]),
                         orient_err(gb[best_g][6], pb[i][6], yaw_period[c]))
                    for k, v in zip(ERR_NAMES, e):
                        match[k].append(v)
                    mconf.append(confs[ind])
                    tp_out[t, i], match_out[t, i] = 1, best_g
                    err_out[t, :, i] = e
                else:
                    tp.append(0)
            if npos == 0 or len(mconf) == 0:
                md_out[(c, t)] = no_predictions()
                continue
            tpc = np.cumsum(tp).astype(float)
            fpc = np.cumsum([1 - v for v in tp]).astype(float)
            prec = tpc / (fpc + tpc)
            rec = tpc / float(npos)
            r = np.linspace(0, 1, NELEM)
            md = {"recall": r, "precision": np.interp(r, rec, prec, right=0),
                  "confidence": np.interp(r, rec, np.array(conf), right=0)}
            for k in ERR_NAMES:
                cm = cummean(np.array(match[k]))
                md[k] = np.interp(md["confidence"][::-1], mconf[::-1], cm[::-1])[::-1]
            md_out[(c, t)] = md

    tpi = list(dist_ths).index(dist_th_tp)
    ap = np.array([[calc_ap(md_out[(c, t)], min_recall, min_precision) for t in range(T)] for c in range(C)])
    tp_err = np.array([[calc_tp(md_out[(c, tpi)], min_recall, k) for k in ERR_NAMES] for c in range(C)])
    return dict(tp=tp_out, match_gt=match_out, err=err_out, npos=npos_out, md=md_out, ap=ap, tp_err=tp_err,
                summary=summary(ap, tp_err, mean_ap_weight))


def summary(ap, tp_err, mean_ap_weight):
    """mean_dist_aps, mean_ap, tp_errors, tp_scores and nd_score from ap [C, T] and tp_err [C, 4] (ERR_NAMES)"""
    mean_dist_aps = [float(np.mean(ap[c])) for c in range(len(ap))]
    mean_ap = float(np.mean(mean_dist_aps))
    tp_errors = {k: float(np.nanmean(tp_err[:, ERR_NAMES.index(k)])) for k in TP_METRICS}
    tp_scores = {k: max(0.0, 1.0 - v) for k, v in tp_errors.items()}
    nd = float(mean_ap_weight * mean_ap + np.sum(list(tp_scores.values()))) / float(mean_ap_weight + len(tp_scores))
    return dict(mean_dist_aps=mean_dist_aps, mean_ap=mean_ap, tp_errors=tp_errors, tp_scores=tp_scores, nd_score=nd)
