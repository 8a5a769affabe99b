"""Restatements of the rotated-box contract of include/cmt_hip.h (cmt_box_iou, cmt_box_nms, cmt_box_concat) in
numpy, and the input generators the host and the device tests share.

``iou_pairs(A, B, z_origin, dtype)`` follows the header operation for operation on arrays of ``dtype``: with
float64 it is the reference (the float32 inputs are exact in float64), with float32 it is the float32 restatement
(numpy rounds every elementwise float32 operation on its own, as the kernels do; only sin / cos may differ from the
device's by a few ulp).  ``measure_e32()`` is the worst difference of the two over every input set the device test
uses; the device test's bar is 8 times that.
"""
import functools
import math

import numpy as np

F = np.float32
CORNERS = ((-1, -1), (-1, 1), (1, 1), (1, -1))     # the corner order of cmt_gtdb_collide


# ---- the overlap of pairs ----------------------------------------------------------------------------------------
def valid_rows(b):
    b = np.asarray(b)
    return np.isfinite(b[:, :7]).all(1) & (b[:, 3] > 0) & (b[:, 4] > 0) & (b[:, 5] > 0)


def _clip(U, V, n, b, upper):
    """one half-plane over P polygons at once: U the clipped coordinate [P, 8], V the other, n [P] vertex counts"""
    P = U.shape[0]
    OU, OV, m = np.zeros_like(U), np.zeros_like(V), np.zeros(P, np.int64)
    rows = np.arange(P)
    for i in range(8):
        act = i < n
        if not act.any():
            break
        k = np.where(i + 1 < n, i + 1, 0)
        pu, pv, qu, qv = U[:, i], V[:, i], U[rows, k], V[rows, k]
        pin, qin = (pu <= b, qu <= b) if upper else (pu >= b, qu >= b)
        e = act & pin & (m < 8)
        OU[rows[e], m[e]], OV[rows[e], m[e]] = pu[e], pv[e]
        m = m + e
        e = act & (pin != qin) & (m < 8)
        with np.errstate(all="ignore"):
            t = (b - pu) / (qu - pu)
            cv = pv + t * (qv - pv)
        OU[rows[e], m[e]], OV[rows[e], m[e]] = b[e], cv[e]
        m = m + e
    return OU, OV, m


def iou_pairs(A, B, z_origin=0.5, dtype=np.float64):
    """rows of A against the same rows of B, each [P, >= 7] -> (bev [P], iou3d [P]) of ``dtype``"""
    A, B = np.asarray(A)[:, :7], np.asarray(B)[:, :7]
    P = A.shape[0]
    bev, v3 = np.zeros(P, dtype), np.zeros(P, dtype)
    ok = valid_rows(A) & valid_rows(B)
    if not ok.any():
        return bev, v3
    a, b = A[ok].astype(dtype), B[ok].astype(dtype)
    half, zo = dtype(0.5), dtype(z_origin)
    xa, ya, za, dxa, dya, dza, wa = a.T
    xb, yb, zb, dxb, dyb, dzb, wb = b.T
    hxa, hya, hxb, hyb = dxa * half, dya * half, dxb * half, dyb * half
    sa, ca, sb, cb = np.sin(wa), np.cos(wa), np.sin(wb), np.cos(wb)
    bota, botb = za - zo * dza, zb - zo * dzb
    topa, topb = bota + dza, botb + dzb
    areaa, areab = dxa * dya, dxb * dyb
    vola, volb = areaa * dza, areab * dzb
    tx, ty = xb - xa, yb - ya
    ox, oy = tx * ca + ty * sa, ty * ca - tx * sa
    c, s = cb * ca + sb * sa, sb * ca - cb * sa
    n = a.shape[0]
    X, Y = np.zeros((n, 8), dtype), np.zeros((n, 8), dtype)
    for k, (sx, sy) in enumerate(CORNERS):
        lx, ly = dtype(sx) * hxb, dtype(sy) * hyb
        X[:, k] = (lx * c - ly * s) + ox
        Y[:, k] = (lx * s + ly * c) + oy
    cnt = np.full(n, 4, np.int64)
    X, Y, cnt = _clip(X, Y, cnt, hxa, True)
    X, Y, cnt = _clip(X, Y, cnt, -hxa, False)
    Y, X, cnt = _clip(Y, X, cnt, hya, True)
    Y, X, cnt = _clip(Y, X, cnt, -hya, False)
    acc = np.zeros(n, dtype)
    for i in range(1, 7):
        use = i + 1 < cnt
        ax, ay = X[:, i] - X[:, 0], Y[:, i] - Y[:, 0]
        bx, by = X[:, i + 1] - X[:, 0], Y[:, i + 1] - Y[:, 0]
        acc = np.where(use, acc + (ax * by - ay * bx), acc)
    area = np.abs(acc) * half
    with np.errstate(all="ignore"):
        bev[ok] = area / ((areaa + areab) - area)
        h = np.maximum(dtype(0), np.minimum(topa, topb) - np.maximum(bota, botb))
        inter = area * h
        v3[ok] = inter / ((vola + volb) - inter)
    return bev, v3


def iou_matrix(a, b, z_origin=0.5, dtype=np.float64, prune=False, chunk=200000):
    """every row of a [N, >= 7] against every row of b [M, >= 7] -> (bev [N, M], iou3d [N, M]).  ``prune``: pairs
    whose centres are farther apart than the two half diagonals (and a millimetre) are exactly 0 and skip the
    clipping; that keeps the large NMS cases quick."""
    a, b = np.asarray(a), np.asarray(b)
    N, M = a.shape[0], b.shape[0]
    bev, v3 = np.zeros((N, M), dtype), np.zeros((N, M), dtype)
    if N == 0 or M == 0:
        return bev, v3
    ii, jj = np.meshgrid(np.arange(N), np.arange(M), indexing="ij")
    ii, jj = ii.reshape(-1), jj.reshape(-1)
    if prune:
        with np.errstate(all="ignore"):
            ra = 0.5 * np.hypot(a[:, 3].astype(np.float64), a[:, 4].astype(np.float64))
            rb = 0.5 * np.hypot(b[:, 3].astype(np.float64), b[:, 4].astype(np.float64))
            d = np.hypot(a[ii, 0].astype(np.float64) - b[jj, 0], a[ii, 1].astype(np.float64) - b[jj, 1])
            near = ~(d > ra[ii] + rb[jj] + 1e-3)
        ii, jj = ii[near], jj[near]
    for s in range(0, ii.size, chunk):
        i, j = ii[s:s + chunk], jj[s:s + chunk]
        e, t = iou_pairs(a[i], b[j], z_origin, dtype)
        bev[i, j], v3[i, j] = e, t
    return bev, v3


# ---- NMS -----------------------------------------------------------------------------------------------------------
def visiting_order(scores, count=None, score_thr=-math.inf):
    """the existing rows in descending score, equal scores (-0 == +0) by ascending row index"""
    s = np.asarray(scores, np.float64)
    n = len(s) if count is None else max(0, min(int(count), len(s)))
    rows = [i for i in range(n) if not math.isnan(s[i]) and s[i] >= score_thr]
    return sorted(rows, key=lambda i: (-(s[i] + 0.0), i))


def _ranked_matrix(boxes, order, z_origin, use_3d):
    b = np.asarray(boxes)[order]
    bev, v3 = iou_matrix(b, b, z_origin, np.float64, prune=True)
    return v3 if use_3d else bev          # [r, q]: computed in the frame of rank r


def nms(boxes, scores, iou_thr, labels=None, count=None, score_thr=-math.inf, z_origin=0.5, use_3d=False):
    """the float64 greedy loop -> the kept rows in visiting order"""
    order = visiting_order(scores, count, score_thr)
    iou = _ranked_matrix(boxes, order, z_origin, use_3d)
    kept = []
    for q, i in enumerate(order):
        if not any(iou[r, q] > iou_thr and (labels is None or labels[order[r]] == labels[i]) for r in kept):
            kept.append(q)
    return [order[q] for q in kept]


def margins(boxes, scores, iou_thr, labels=None, count=None, score_thr=-math.inf, z_origin=0.5, use_3d=False):
    """the smallest |iou64 - iou_thr| over every pair the NMS can compare (an earlier rank against a later one, of
    equal label when labels are given); inf without such a pair"""
    order = visiting_order(scores, count, score_thr)
    if len(order) < 2:
        return math.inf
    iou = _ranked_matrix(boxes, order, z_origin, use_3d)
    upper = np.triu(np.ones_like(iou, bool), 1)
    if labels is not None:
        lab = np.asarray(labels)[order]
        upper &= lab[:, None] == lab[None, :]
    v = valid_rows(np.asarray(boxes)[order])
    upper &= v[:, None] & v[None, :]
    return float(np.abs(iou[upper] - iou_thr).min()) if upper.any() else math.inf


# ---- concat ----------------------------------------------------------------------------------------------------------
def concat(sources, poses=None, cols=None):
    """float64 cmt_box_concat: sources of (boxes, scores, labels[, count]) -> (boxes, scores, labels, source)"""
    poses = [None] * len(sources) if poses is None else poses
    cols = min(min(np.asarray(s[0]).shape[1] for s in sources), 16) if cols is None else cols
    ob, os_, ol, osrc = [], [], [], []
    for k, src in enumerate(sources):
        b = np.asarray(src[0], np.float64)[:, :cols].copy()
        sc, lab = np.asarray(src[1], np.float64).copy(), np.asarray(src[2], np.int64).copy()
        n = b.shape[0]
        c = n if len(src) < 4 or src[3] is None else max(0, min(int(src[3]), n))
        if poses[k] is not None:
            m = np.asarray(poses[k], np.float64)
            b[:, :3] = b[:, :3] @ m[:3, :3].T + m[:3, 3]
            b[:, 6] += math.atan2(m[1, 0], m[0, 0])
            if cols >= 9:
                b[:, 7:9] = b[:, 7:9] @ m[:2, :2].T
        b[c:], sc[c:], lab[c:] = 0.0, -np.inf, -1
        ob.append(b), os_.append(sc), ol.append(lab), osrc.append(np.full(n, k, np.int64))
    return np.concatenate(ob), np.concatenate(os_), np.concatenate(ol), np.concatenate(osrc)


# ---- inputs ----------------------------------------------------------------------------------------------------------
def random_boxes(rng, n, centre=(0.0, 0.0), spread=10.0):
    b = np.zeros((n, 7), F)
    b[:, 0] = centre[0] + rng.uniform(-spread, spread, n)
    b[:, 1] = centre[1] + rng.uniform(-spread, spread, n)
    b[:, 2] = rng.uniform(-2, 1, n)
    b[:, 3], b[:, 4], b[:, 5] = rng.uniform(0.5, 6, n), rng.uniform(0.4, 3, n), rng.uniform(0.5, 3, n)
    b[:, 6] = rng.uniform(-7, 7, n)
    return b


def related(rng, a, kind):
    """a box that stands in relation ``kind`` (0 identical, 1 quarter turn, 2 nested, 3 touching along its own
    axis, 4 nearby and random) to the row ``a``; float32"""
    b = a.astype(np.float64).copy()
    if kind == 1:
        b[6] += math.pi / 2
    elif kind == 2:
        b[3:6] *= rng.uniform(0.3, 0.9, 3)
        b[6] += rng.choice([0.0, math.pi])
    elif kind == 3:
        b[0] += a[3] * math.cos(a[6])
        b[1] += a[3] * math.sin(a[6])
    elif kind == 4:
        b[0:2] += rng.uniform(-2, 2, 2)
        b[2] += rng.uniform(-1, 1)
        b[3:6] *= rng.uniform(0.6, 1.5, 3)
        b[6] = rng.uniform(-7, 7)
    return b.astype(F)


def mixed_sets(seed, n, m):
    """a [n, 7] and b [m, 7] somewhere within 150 m of the origin: a is random in a 20 m window, row j of b stands
    in relation j % 5 to row j % n of a, so identical, quarter-turned, nested, touching and random pairs all occur
    and most other pairs overlap a little or not at all"""
    rng = np.random.RandomState(seed)
    centre = rng.uniform(-150, 150, 2)
    a = random_boxes(rng, n, centre)
    b = np.zeros((m, 7), F)
    for j in range(m):
        b[j] = related(rng, a[j % n], j % 5) if n else random_boxes(rng, 1, centre)[0]
    return a, b


def mixed_pairs(seed, n):
    """n aligned pairs of the five relations, every pair at a scene offset of its own up to 150 m"""
    rng = np.random.RandomState(seed)
    a = random_boxes(rng, n, (0.0, 0.0), 150.0)
    b = np.stack([related(rng, a[j], j % 5) for j in range(n)]) if n else np.zeros((0, 7), F)
    return a, b


MATRIX_SHAPES = ((1, 1), (63, 65), (65, 63), (130, 7), (0, 5))
ALIGNED_PAIRS = 6000


def matrix_case(k):
    """the k-th pair of sets of the device test; the larger ones carry rows that overlap nothing: a NaN, an inf, a
    size of zero and a negative size"""
    n, m = MATRIX_SHAPES[k]
    a, b = mixed_sets(100 + k, n, m)
    if n >= 8:
        a[3, 1], a[6, 3] = np.nan, 0.0
    if m >= 7:
        b[5, 6], b[6, 5] = np.inf, -1.0
    return a, b


def aligned_case():
    return mixed_pairs(7, ALIGNED_PAIRS)


@functools.lru_cache(maxsize=None)
def measure_e32():
    """the worst |float32 restatement - float64| of bev and iou3d over every input set of the device test, both
    values of z_origin"""
    worst = 0.0
    for zo in (0.5, 0.0):
        sets = [matrix_case(k) for k in range(len(MATRIX_SHAPES))]
        for a, b in sets:
            for x, y in zip(iou_matrix(a, b, zo, np.float64), iou_matrix(a, b, zo, np.float32)):
                if x.size:
                    worst = max(worst, float(np.abs(x - y.astype(np.float64)).max()))
        a, b = aligned_case()
        for x, y in zip(iou_pairs(a, b, zo, np.float64), iou_pairs(a, b, zo, np.float32)):
            worst = max(worst, float(np.abs(x - y.astype(np.float64)).max()))
    return worst


def cluster_scene(seed, n, extent=None, ncls=3):
    """n boxes for the NMS tests: objects on a jittered grid 12 m apart (so different objects never touch), each
    seen 1..4 times with perturbations of up to 0.3 m, 0.1 rad and 10 % in size -> (boxes [n, 9] float32, scores,
    labels int32)"""
    rng = np.random.RandomState(seed)
    boxes, labels = [], []
    side = max(1, int(math.ceil(math.sqrt(max(n, 1) / 2.0))))
    cells = rng.permutation(side * side)
    c = 0
    while len(boxes) < n:
        gx, gy = divmod(int(cells[c % len(cells)]), side)
        c += 1
        base = random_boxes(rng, 1, (gx * 12.0 - side * 6.0, gy * 12.0 - side * 6.0), 1.5)[0]
        base[3:5] = rng.uniform(1.5, 5.0), rng.uniform(1.2, 2.5)
        lab = rng.randint(0, ncls)
        for _ in range(rng.randint(1, 5)):
            if len(boxes) >= n:
                break
            b = np.zeros(9, F)
            b[:7] = base
            b[0:2] += rng.uniform(-0.3, 0.3, 2)
            b[3:6] *= rng.uniform(0.9, 1.1, 3)
            b[6] += rng.uniform(-0.1, 0.1)
            b[7:9] = rng.uniform(-5, 5, 2)
            boxes.append(b), labels.append(lab if rng.uniform() < 0.8 else rng.randint(0, ncls))
    boxes = np.stack(boxes) if boxes else np.zeros((0, 9), F)
    scores = rng.uniform(0.05, 1.0, len(boxes)).astype(F)
    return boxes.astype(F), scores, np.asarray(labels, np.int32).reshape(-1)
