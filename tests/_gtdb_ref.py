"""The contracts of cmt_gtdb_extract, cmt_gtdb_gather and cmt_gtdb_collide (include/cmt_hip.h) and the host side of
native_gtdb.py restated in numpy, for the tests.

The inside test is ``_aug_ref.inside`` (float64; it binds only points clear of every face, which
``_aug_ref.inside_inputs`` builds).  The subtractions and additions of extract / gather are single float32
operations.  The collision test is float64 and SEQUENTIAL, with the reference's early exits, and returns with every
answer the smallest |lhs - rhs| over the comparisons it made: the device's float32 answer is bound only where that
margin is above ``tol``.
"""
import numpy as np

import _aug_ref as A


# ---- extract / gather --------------------------------------------------------------------------------------------
def extract(points, boxes, count=None):
    """-> (rows float32 [total, F], offsets int32 [M + 1]): points[inside[:, b]] with box b's bottom centre
    subtracted, box after box"""
    points, boxes = np.asarray(points, np.float32), np.asarray(boxes, np.float32)
    m = A.inside(points, boxes)
    if count is not None:
        m[max(0, min(int(count), points.shape[0])):] = False
    segs, offsets = [], [0]
    for b in range(boxes.shape[0]):
        seg = points[m[:, b]].copy()
        with np.errstate(invalid="ignore"):
            seg[:, :3] = seg[:, :3] - boxes[b, :3]
        segs.append(seg)
        offsets.append(offsets[-1] + seg.shape[0])
    rows = np.concatenate(segs, 0) if segs else np.zeros((0, points.shape[1]), np.float32)
    return rows.astype(np.float32), np.asarray(offsets, np.int32)


def gather(rows, seg_offset, seg_len, centre):
    """-> float32 [sum(seg_len), F]: the chosen segments one after another, each moved to its centre"""
    rows, centre = np.asarray(rows, np.float32), np.asarray(centre, np.float32).reshape(-1, 3)
    out = []
    for k, (o, n) in enumerate(zip(seg_offset, seg_len)):
        seg = rows[int(o):int(o) + int(n)].copy()
        with np.errstate(invalid="ignore"):
            seg[:, :3] = seg[:, :3] + centre[k]
        out.append(seg)
    return np.concatenate(out, 0) if out else np.zeros((0, rows.shape[1]), np.float32)


# ---- the collision test ------------------------------------------------------------------------------------------
SIGNS = np.array([[-1, -1], [-1, 1], [1, 1], [1, -1]], np.float64)


def corners(boxes):
    """center_to_corner_box2d with origin 0.5, float64 [n, 4, 2], rotated counter-clockwise by yaw"""
    b = np.asarray(boxes, np.float32).astype(np.float64)
    loc = SIGNS[None] * (b[:, None, 3:5] / 2)
    c, s = np.cos(b[:, 6])[:, None], np.sin(b[:, 6])[:, None]
    x = loc[..., 0] * c - loc[..., 1] * s + b[:, None, 0]
    y = loc[..., 0] * s + loc[..., 1] * c + b[:, None, 1]
    return np.stack([x, y], -1)


def tol(boxes):
    """2^-16 * (1 + Cmax) * (1 + Emax): Cmax the largest |corner coordinate|, Emax the largest box diagonal"""
    b = np.asarray(boxes, np.float32).astype(np.float64)
    if b.shape[0] == 0:
        return 2.0 ** -16
    return 2.0 ** -16 * (1 + np.abs(corners(b)).max()) * (1 + np.hypot(b[:, 3], b[:, 4]).max())


class _Margin:
    def __init__(self):
        self.m = np.inf

    def gt(self, lhs, rhs):
        self.m = min(self.m, abs(lhs - rhs))
        return lhs > rhs


def _contains(P, Q, mg):
    """every corner of Q strictly inside P (clockwise corners): cross < 0 for each edge; the first cross >= 0 ends it"""
    for l in range(4):
        for k in range(4):
            v = P[(k + 1) % 4] - P[k]
            lhs, rhs = v[1] * (P[k, 0] - Q[l, 0]), v[0] * (P[k, 1] - Q[l, 1])
            if not mg.gt(rhs, lhs):        # cross = lhs - rhs >= 0
                return False
    return True


def collide_pair(P, Q, mg=None):
    """box_collision_test(..., clockwise=True) for one pair of [4, 2] corner sets, sequential -> bool; ``mg``
    collects the smallest margin of the comparisons made"""
    mg = mg or _Margin()
    iw = min(P[:, 0].max(), Q[:, 0].max()) - max(P[:, 0].min(), Q[:, 0].min())
    if not mg.gt(iw, 0.0):
        return False
    ih = min(P[:, 1].max(), Q[:, 1].max()) - max(P[:, 1].min(), Q[:, 1].min())
    if not mg.gt(ih, 0.0):
        return False
    for k in range(4):
        a, b = P[k], P[(k + 1) % 4]
        for l in range(4):
            c, d = Q[l], Q[(l + 1) % 4]
            acd = mg.gt((d[1] - a[1]) * (c[0] - a[0]), (c[1] - a[1]) * (d[0] - a[0]))
            bcd = mg.gt((d[1] - b[1]) * (c[0] - b[0]), (c[1] - b[1]) * (d[0] - b[0]))
            if acd != bcd:
                abc = mg.gt((c[1] - a[1]) * (b[0] - a[0]), (b[1] - a[1]) * (c[0] - a[0]))
                abd = mg.gt((d[1] - a[1]) * (b[0] - a[0]), (b[1] - a[1]) * (d[0] - a[0]))
                if abc != abd:
                    return True
    if _contains(P, Q, mg):
        return True
    return _contains(Q, P, mg)


def collision_rows(boxes, n_gt):
    """-> (bool [n, n] with the candidates' rows filled (row i, column j: collide(i, j), diagonal False), margin)"""
    cor = corners(boxes)
    n = cor.shape[0]
    mat = np.zeros((n, n), bool)
    mg = _Margin()
    for i in range(n_gt, n):
        for j in range(n):
            if j != i:
                mat[i, j] = collide_pair(cor[i], cor[j], mg)
    return mat, mg.m


def greedy(mat, n_gt, group):
    """sample_all's loop over sample_class_v2: per group, the boxes to avoid are the ground truth and the kept
    candidates of earlier groups; a candidate with a True in its row is dropped and its row and column cleared"""
    group = np.asarray(group, np.int64)
    keep = np.zeros(len(group), np.int32)
    avoid = list(range(n_gt))
    for g in np.unique(group):
        cand = [n_gt + int(i) for i in np.nonzero(group == g)[0]]
        idx = avoid + cand
        sub = mat[np.ix_(idx, idx)].copy()
        np.fill_diagonal(sub, False)
        for t in range(len(avoid), len(idx)):
            if sub[t].any():
                sub[t] = False
                sub[:, t] = False
            else:
                keep[idx[t] - n_gt] = 1
                avoid.append(idx[t])
    return keep


def collide(boxes, n_gt, group):
    """-> (keep int32 [n_s], count, margin): margin is the smallest |lhs - rhs| of any comparison made"""
    assert np.all(np.diff(np.asarray(group, np.int64)) >= 0)
    mat, margin = collision_rows(boxes, n_gt)
    keep = greedy(mat, n_gt, group)
    return keep, int(keep.sum()), margin


def _box(x, y, dx, dy, yaw):
    return [x, y, -1.0, dx, dy, 1.5, yaw]


def hand_scenes():
    """name -> (boxes float32 [n, 7], n_gt, group, keep): answers worked out by hand, see tests/test_gtdb_host.py"""
    big, small = _box(0, 0, 10, 8, 0.2), _box(0.5, 0.3, 1.0, 0.6, 1.0)
    s = {
        "crossing": ([_box(0, 0, 4, 1.2, 0.3), _box(0.3, -0.2, 3.5, 1.0, 1.7)], 1, [0], [0]),
        "small_in_large": ([big, small], 1, [0], [0]),
        "large_around_small": ([small, big], 1, [0], [0]),
        "standup_only": ([_box(0, 0, 4, 0.5, np.pi / 4), _box(1.0, -1.0, 0.6, 0.6, np.pi / 4)], 1, [0], [1]),
        "gap": ([_box(0, 0, 2, 2, 0.4), _box(5, 0, 2, 2, -0.4)], 1, [0], [1]),
        # candidate 0 touches only the later candidate 1 of its own group: 0 goes, then nothing live touches 1
        "later_of_own_group": ([_box(0, 0, 4, 2, 0.1), _box(1, 0.5, 4, 2, 0.5)], 0, [0, 0], [0, 1]),
        # candidate 0 touches the box to avoid and goes; candidate 1 (a later group) touches only candidate 0
        "rejected_of_earlier_group": ([_box(0, 0, 4, 2, 0.1), _box(3, 0, 4, 2, 0.3), _box(6, 0.2, 3, 2, -0.2)],
                                      1, [0, 1], [0, 1]),
    }
    return {k: (np.asarray(b, np.float32), n_gt, np.asarray(g, np.int32), np.asarray(keep, np.int32))
            for k, (b, n_gt, g, keep) in s.items()}


IDENTICAL = np.asarray([_box(2.0, -3.0, 4.0, 2.0, 0.0)] * 2, np.float32)   # every value dyadic, yaw 0: exact in float32


def random_scene(rs):
    """one scene of the GPU test's generator: n_gt in [0, 30), n_s in [1, 40), centres in +-20 m, extents
    0.5 .. 6 m, yaw in +-4, groups the sorted randint(0, 4)"""
    n_gt, n_s = int(rs.randint(0, 30)), int(rs.randint(1, 40))
    n = n_gt + n_s
    b = np.zeros((n, 7), np.float32)
    b[:, :2] = rs.uniform(-20, 20, (n, 2))
    b[:, 2] = -1.0
    b[:, 3:5] = rs.uniform(0.5, 6.0, (n, 2))
    b[:, 5] = 1.5
    b[:, 6] = rs.uniform(-4, 4, n)
    group = np.sort(rs.randint(0, 4, n_s)).astype(np.int32)
    return b, n_gt, group


# ---- the host side -----------------------------------------------------------------------------------------------
def box_corners(boxes):
    """LiDARInstance3DBoxes.corners in float64 [n, 8, 3]: (x0 y0 z0), (x0 y0 z1), (x0 y1 z1), (x0 y1 z0), then
    the same with x1; origin (0.5, 0.5, 0)"""
    b = np.asarray(boxes, np.float64)
    norm = np.array([[0, 0, 0], [0, 0, 1], [0, 1, 1], [0, 1, 0], [1, 0, 0], [1, 0, 1], [1, 1, 1], [1, 1, 0]], np.float64)
    loc = (norm - [0.5, 0.5, 0.0])[None] * b[:, None, 3:6]
    c, s = np.cos(b[:, 6])[:, None], np.sin(b[:, 6])[:, None]
    x = loc[..., 0] * c - loc[..., 1] * s + b[:, None, 0]
    y = loc[..., 0] * s + loc[..., 1] * c + b[:, None, 1]
    return np.stack([x, y, loc[..., 2] + b[:, None, 2]], -1)
