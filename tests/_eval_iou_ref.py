"""Plain numpy restatement of the IoU-matched evaluation of include/cmt_hip.h (cmt_det_eval_match_iou,
cmt_det_eval_ap_interp), in the style of _eval_ref.py: Python loops, dictionaries per sample, the real numpy.interp
for the reused curves, and the interpolated APs as plain loops.  The overlap is _iou_ref.iou_pairs with the ground
truth as the first box: float32 for the values the match decides on (the device's arithmetic up to sin / cos), float64
for the margins the tests keep between those values and every decision."""
import numpy as np

import _eval_ref as R
import _iou_ref as I

ERR_NAMES = R.ERR_NAMES
TP_METRICS = R.TP_METRICS
MODES = ("bev", "3d")


def pair_iou(gt_rows, pred_rows, mode, z_origin, dtype):
    """iou [len(gt_rows), len(pred_rows)] of ``dtype``, clipped in the ground truth's frame; invalid boxes and NaN
    quotients give 0"""
    g, p = np.asarray(gt_rows, np.float32).reshape(-1, 9), np.asarray(pred_rows, np.float32).reshape(-1, 9)
    out = np.zeros((len(g), len(p)), dtype)
    if len(g) and len(p):
        gi, pi = np.meshgrid(np.arange(len(g)), np.arange(len(p)), indexing="ij")
        bev, v3 = I.iou_pairs(g[gi.reshape(-1)], p[pi.reshape(-1)], z_origin, dtype)
        v = (v3 if mode == "3d" else bev).reshape(len(g), len(p))
        out = np.where(np.isnan(v), dtype(0), v)
    return out


def ap_interp(tp, npos):
    """(all-point AP, 40-point AP) of one (class, threshold) from the tp flags in visiting order"""
    n, M = len(tp), int(sum(tp))
    if npos == 0 or M == 0:
        return 0.0, 0.0
    ctp, run = [], 0
    for v in tp:
        run += int(v)
        ctp.append(run)
    prec = [ctp[j] / float(j + 1) for j in range(n)]
    env, best = [0.0] * n, -np.inf
    for j in range(n - 1, -1, -1):
        best = max(best, prec[j])
        env[j] = best
    pos = [j for j in range(n) if tp[j]]          # pos[m - 1]: the position of the m-th match
    s = 0.0
    for j in pos:
        s = s + env[j]
    r = 0.0
    for k in range(1, 41):
        mk = None
        for m in range(1, M + 1):
            if m * 40 >= k * npos:
                mk = m
                break
        r = r + (env[pos[mk - 1]] if mk is not None else 0.0)
    return s / float(npos), r / 40.0


def evaluate(pred_boxes, pred_scores, pred_labels, pred_samples, gt_boxes, gt_labels, gt_samples, gt_num_pts, *,
             num_samples, class_range, yaw_period, iou_ths, iou_th_tp, mode="3d", z_origin=0.5, min_recall=0.1,
             min_precision=0.1, n_pred=None, n_gt=None, dtype=np.float32, trace=None):
    """-> dict(tp [T, N] uint8, match_gt [T, N], err [T, 4, N], match_iou [T, N] float32 (NaN: none), npos [C],
    md {(c, t): curves}, ap [C, T] (101-point), ap_interp [C, T, 2], tp_err [C, 4] (columns ERR_NAMES),
    mean_iou [C] (at iou_th_tp; NaN: no match), pairs {(gt row, prediction row): iou}, summary).  ``dtype``: the arithmetic of the overlap.  ``trace``: a
    list that receives (sample, class, t, best iou, second-best iou, best row, second row) of every greedy step with
    at least one candidate."""
    assert mode in MODES
    pb = np.asarray(pred_boxes, dtype=np.float32).reshape(-1, 9)
    ps = np.asarray(pred_scores, dtype=np.float32)
    pl, psm = np.asarray(pred_labels), np.asarray(pred_samples)
    gb = np.asarray(gt_boxes, dtype=np.float32).reshape(-1, 9)
    gl, gsm, gnp = np.asarray(gt_labels), np.asarray(gt_samples), np.asarray(gt_num_pts)
    N, G = len(pb), len(gb)
    n_pred = N if n_pred is None else min(max(int(n_pred), 0), N)
    n_gt = G if n_gt is None else min(max(int(n_gt), 0), G)
    C, T, S = len(class_range), len(iou_ths), int(num_samples)
    ths = [dtype(t) for t in iou_ths]

    def kept(box, label, sample):
        if not (0 <= label < C and 0 <= sample < S):
            return False
        return R.dist2d(box[0], box[1], 0.0, 0.0) < class_range[label]

    preds = {(s, c): [] for s in range(S) for c in range(C)}
    for i in range(n_pred):
        if kept(pb[i], int(pl[i]), int(psm[i])):
            preds[(int(psm[i]), int(pl[i]))].append(i)
    gts = {(s, c): [] for s in range(S) for c in range(C)}
    for g in range(n_gt):
        if kept(gb[g], int(gl[g]), int(gsm[g])) and int(gnp[g]) != 0:
            gts[(int(gsm[g]), int(gl[g]))].append(g)
    # the overlap of every (ground truth, prediction) of a (sample, class), computed once
    iou = {}
    for key in preds:
        m = pair_iou(gb[gts[key]], pb[preds[key]], mode, z_origin, dtype)
        for a, g in enumerate(gts[key]):
            for b, i in enumerate(preds[key]):
                iou[(g, i)] = m[a, b]

    tp_out = np.zeros((T, N), dtype=np.uint8)
    match_out = np.full((T, N), -1, dtype=np.int64)
    err_out = np.full((T, 4, N), np.nan)
    miou_out = np.full((T, N), np.nan, dtype=np.float32)
    npos_out = np.zeros(C, dtype=np.int64)
    ai_out = np.zeros((C, T, 2))
    md_out = {}
    for c in range(C):
        npos = sum(len(gts[(s, c)]) for s in range(S))
        npos_out[c] = npos
        plist = sorted(i for s in range(S) for i in preds[(s, c)])
        confs = [float(ps[i]) + 0.0 for i in plist]
        sortind = [i for (v, i) in sorted((v, i) for (i, v) in enumerate(confs))][::-1]
        for t in range(T):
            taken = set()
            tp, conf, mconf = [], [], []
            match = {k: [] for k in ERR_NAMES}
            for ind in sortind:
                i = plist[ind]
                s = int(psm[i])
                best, best_g, second, second_g = None, None, None, None
                for g in gts[(s, c)]:                 # annotation order: a strict comparison keeps the lowest index
                    if g in taken:
                        continue
                    v = iou[(g, i)]
                    if best is None or v > best:
                        best, best_g, second, second_g = v, g, best, best_g
                    elif second is None or v > second:
                        second, second_g = v, g
                if trace is not None and best is not None:
                    trace.append((s, c, t, best, second, best_g, second_g))
                conf.append(confs[ind])
                if best is not None and best > ths[t]:
                    taken.add(best_g)
                    tp.append(1)
                    e = (R.dist2d(gb[best_g][0], gb[best_g][1], pb[i][0], pb[i][1]),
                         R.dist2d(pb[i][7], pb[i][8], gb[best_g][7], gb[best_g][8]),
                         R.scale_err(gb[best_g][3:6], pb[i][3:6]),
                         R.orient_err(gb[best_g][6], pb[i][6], yaw_period[c]))
                    for k, v in zip(ERR_NAMES, e):
                        match[k].append(v)
                    mconf.append(confs[ind])
                    tp_out[t, i], match_out[t, i], miou_out[t, i] = 1, best_g, best
                    err_out[t, :, i] = e
                else:
                    tp.append(0)
            ai_out[c, t] = ap_interp(tp, npos)
            if npos == 0 or len(mconf) == 0:
                md_out[(c, t)] = R.no_predictions()
                continue
            tpc = np.cumsum(tp).astype(float)
            fpc = np.cumsum([1 - v for v in tp]).astype(float)
            prec = tpc / (fpc + tpc)
            rec = tpc / float(npos)
            r = np.linspace(0, 1, R.NELEM)
            md = {"recall": r, "precision": np.interp(r, rec, prec, right=0),
                  "confidence": np.interp(r, rec, np.array(conf), right=0)}
            for k in ERR_NAMES:
                cm = R.cummean(np.array(match[k]))
                md[k] = np.interp(md["confidence"][::-1], mconf[::-1], cm[::-1])[::-1]
            md_out[(c, t)] = md

    tpi = [float(t) for t in iou_ths].index(float(iou_th_tp))
    ap = np.array([[R.calc_ap(md_out[(c, t)], min_recall, min_precision) for t in range(T)] for c in range(C)])
    tp_err = np.array([[R.calc_tp(md_out[(c, tpi)], min_recall, k) for k in ERR_NAMES] for c in range(C)])
    mean_iou = np.full(C, np.nan)
    for c in range(C):
        vals = [float(miou_out[tpi, i]) for i in range(N) if tp_out[tpi, i] and int(pl[i]) == c]
        if vals:
            mean_iou[c] = float(np.mean(vals))
    return dict(tp=tp_out, match_gt=match_out, err=err_out, match_iou=miou_out, npos=npos_out, md=md_out, ap=ap,
                ap_interp=ai_out, tp_err=tp_err, mean_iou=mean_iou, pairs=iou, summary=summary(ap, ai_out, tp_err))


def summary(ap, ai, tp_err):
    """the means over thresholds and classes, and the class means of the TP errors"""
    C = len(ap)
    mean_all = [float(np.mean(ai[c, :, 0])) for c in range(C)]
    mean_r40 = [float(np.mean(ai[c, :, 1])) for c in range(C)]
    mean_101 = [float(np.mean(ap[c])) for c in range(C)]
    return dict(mean_all=mean_all, mean_r40=mean_r40, mean_101=mean_101, map_all=float(np.mean(mean_all)),
                map_r40=float(np.mean(mean_r40)), map_101=float(np.mean(mean_101)),
                tp_errors={k: float(np.nanmean(tp_err[:, ERR_NAMES.index(k)])) for k in TP_METRICS})
