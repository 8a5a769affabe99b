"""Two independent references for the cmt_render_* contract of include/cmt_hip.h.

(a) ``Plane`` and ``points`` / ``segments`` / ``boxes`` / ``digits`` / ``resolve``: the header restated in numpy
    float32.  Every product, sum and quotient is ONE ``np.float32`` operation in the header's order, the walk is in
    Python ints.  Points, segments (both clips), digits and resolve contain no transcendental, so the device must
    equal this bit for bit; ``boxes`` takes sin / cos from numpy float32 and is bit-exact only where they are (yaw 0).
(b) ``boxes64``: float64 geometry for boxes (exact corners, exact projection, clip in float64), then the same
    integer walk.
"""
import math

import numpy as np

F = np.float32
FONT = ((0x0E, 0x11, 0x13, 0x15, 0x19, 0x11, 0x0E), (0x04, 0x0C, 0x04, 0x04, 0x04, 0x04, 0x0E),
        (0x0E, 0x11, 0x01, 0x02, 0x04, 0x08, 0x1F), (0x1F, 0x02, 0x04, 0x02, 0x01, 0x11, 0x0E),
        (0x02, 0x06, 0x0A, 0x12, 0x1F, 0x02, 0x02), (0x1F, 0x10, 0x1E, 0x01, 0x01, 0x11, 0x0E),
        (0x06, 0x08, 0x10, 0x1E, 0x11, 0x11, 0x0E), (0x1F, 0x01, 0x02, 0x04, 0x08, 0x08, 0x08),
        (0x0E, 0x11, 0x11, 0x0E, 0x11, 0x11, 0x0E), (0x0E, 0x11, 0x11, 0x0F, 0x01, 0x02, 0x0C))
BOX_EDGES = [(k, (k + 1) % 4) for k in range(4)] + [(k + 4, (k + 1) % 4 + 4) for k in range(4)] + \
            [(k, k + 4) for k in range(4)]


def okey(f):
    b = int(np.array(f, dtype=np.float32).view(np.uint32))
    return (~b & 0xFFFFFFFF) if b & 0x80000000 else b ^ 0x80000000


def pack(layer, order, rgb):
    return (int(layer) << 56) | ((int(order) & 0xFFFFFFFF) << 24) | (int(rgb) & 0xFFFFFF)


def fin(*vs):
    return all(math.isfinite(float(v)) for v in vs)


class Plane:
    """the uint64 [V][H][W] key plane: ``put`` is the atomic maximum"""

    def __init__(self, V, H, W):
        self.V, self.H, self.W = V, H, W
        self.k = np.zeros((V, H, W), dtype=np.uint64)

    def put(self, v, X, Y, key):
        if 0 <= X < self.W and 0 <= Y < self.H and key > int(self.k[v, Y, X]):
            self.k[v, Y, X] = np.uint64(key)


def row(m, r, x, y, z):
    with np.errstate(all="ignore"):
        return F(F(F(F(m[r][0]) * x) + F(F(m[r][1]) * y)) + F(F(m[r][2]) * z)) + F(m[r][3])


def walk(X0, Y0, X1, Y1):
    """the integer walk of the contract -> the list of its pixels"""
    dX, dY = X1 - X0, Y1 - Y0
    n = max(abs(dX), abs(dY))
    if n == 0:
        return [(X0, Y0)]
    return [(X0 + (2 * dX * k + n) // (2 * n), Y0 + (2 * dY * k + n) // (2 * n)) for k in range(n + 1)]


def _floor_clamp(f, lo, hi):
    return int(min(max(math.floor(float(f)), lo), hi))


def clip_ends(view, near, a, b, W, H, planar):
    """steps (1)-(3) of THE SEGMENT in float32 -> (X0, Y0, X1, Y1) or None"""
    with np.errstate(all="ignore"):
        if planar:
            ua, va, ub, vb = F(a[0]), F(a[1]), F(b[0]), F(b[1])
        else:
            a, b = [F(t) for t in a], [F(t) for t in b]
            if not fin(*a, *b):
                return None
            A = [row(view, r, *a) for r in range(4)]
            B = [row(view, r, *b) for r in range(4)]
            if not fin(*A, *B):
                return None
            near = F(near)
            ina, inb = bool(A[3] >= near), bool(B[3] >= near)
            if not ina and not inb:
                return None
            if ina != inb:
                t = F(F(near - A[3]) / F(B[3] - A[3]))
                c0 = F(A[0] + F(t * F(B[0] - A[0])))
                c1 = F(A[1] + F(t * F(B[1] - A[1])))
                if ina:
                    B[0], B[1], B[3] = c0, c1, near
                else:
                    A[0], A[1], A[3] = c0, c1, near
            ua, va, ub, vb = F(A[0] / A[3]), F(A[1] / A[3]), F(B[0] / B[3]), F(B[1] / B[3])
        dx, dy = F(ub - ua), F(vb - va)
        if not fin(ua, va, ub, vb, dx, dy):
            return None
        xmin = ymin = F(-1.0)
        xmax, ymax = F(W + 1), F(H + 1)
        t0, t1 = F(0.0), F(1.0)
        for p, q in ((F(-dx), F(ua - xmin)), (dx, F(xmax - ua)), (F(-dy), F(va - ymin)), (dy, F(ymax - va))):
            if p == 0:
                if q < 0:
                    return None
                continue
            r = F(q / p)
            if p < 0:
                if r > t1:
                    return None
                if r > t0:
                    t0 = r
            else:
                if r < t0:
                    return None
                if r < t1:
                    t1 = r
        xa, ya, xb, yb = ua, va, ub, vb
        if t0 > 0:
            xa, ya = F(ua + F(t0 * dx)), F(va + F(t0 * dy))
        if t1 < 1:
            xb, yb = F(ua + F(t1 * dx)), F(va + F(t1 * dy))
    return (_floor_clamp(xa, -2, W + 2), _floor_clamp(ya, -2, H + 2), _floor_clamp(xb, -2, W + 2),
            _floor_clamp(yb, -2, H + 2))


def draw_walk(pl, v, ends, thick, key):
    lo, hi = -((thick - 1) // 2), thick // 2
    for X, Y in walk(*ends):
        for j in range(lo, hi + 1):
            for i in range(lo, hi + 1):
                pl.put(v, X + i, Y + j, key)


def segment(pl, v, view, near, a, b, thick, key, planar=False):
    ends = clip_ends(view, near, a, b, pl.W, pl.H, planar)
    if ends is not None:
        draw_walk(pl, v, ends, thick, key)


def points(pl, views, near, layer, pts, lut, *, n=None, radius=0, near_wins=False, color_col=-1, lo=0.0, inv_span=1.0):
    pts = np.asarray(pts, dtype=np.float32)
    n = pts.shape[0] if n is None else min(max(int(n), 0), pts.shape[0])
    lo, inv_span = F(lo), F(inv_span)
    with np.errstate(all="ignore"):
        for i in range(n):
            x, y, z = pts[i, 0], pts[i, 1], pts[i, 2]
            if not fin(x, y, z):
                continue
            for v, m in enumerate(views):
                r3 = row(m, 3, x, y, z)
                if not r3 >= F(near):
                    continue
                r0, r1, d = row(m, 0, x, y, z), row(m, 1, x, y, z), row(m, 2, x, y, z)
                u, w = F(r0 / r3), F(r1 / r3)
                if not fin(d) or not (u >= 0 and u < F(pl.W) and w >= 0 and w < F(pl.H)):
                    continue
                X, Y = int(math.floor(float(u))), int(math.floor(float(w)))
                c = pts[i, color_col] if color_col >= 0 else d
                t = F(F(F(c - lo) * inv_span) * F(255.0))
                idx = 255 if t >= 255 else (int(math.floor(float(t))) if t >= 0 else 0)
                o = okey(d)
                key = pack(layer, (~o & 0xFFFFFFFF) if near_wins else o, int(lut[idx]))
                for j in range(-radius, radius + 1):
                    for e in range(-radius, radius + 1):
                        pl.put(v, X + e, Y + j, key)


def segments(pl, views, near, layer, p0, p1, rgb, *, rank=None, n=None, thickness=1, planar=False):
    S = len(p0)
    n = S if n is None else min(max(int(n), 0), S)
    for s in range(n):
        r = s if rank is None else max(int(rank[s]), 0)
        key = pack(layer, 0xFFFFFFFF - r, int(rgb[s]))
        for v in range(pl.V):
            segment(pl, v, None if planar else views[v], near, p0[s], p1[s], thickness, key, planar)


def box_valid(r):
    return fin(*r[:7]) and r[3] > 0 and r[4] > 0 and r[5] > 0


def box_corners32(r, z_origin):
    """the eight corners and the heading mark of the contract in float32 (sin / cos from numpy float32)"""
    x, y, z, dx, dy, dz, yaw = [F(t) for t in r[:7]]
    hx, hy = F(dx * F(0.5)), F(dy * F(0.5))
    s, c = F(np.sin(yaw)), F(np.cos(yaw))
    bot = F(z - F(F(z_origin) * dz))
    top = F(bot + dz)
    xy = []
    for sx, sy in ((-1, -1), (-1, 1), (1, 1), (1, -1)):
        lx, ly = F(sx * hx), F(sy * hy)
        xy.append((F(F(F(lx * c) - F(ly * s)) + x), F(F(F(lx * s) + F(ly * c)) + y)))
    corners = [(X, Y, bot) for X, Y in xy] + [(X, Y, top) for X, Y in xy]
    head = ((x, y, top), (F(F(hx * c) + x), F(F(hx * s) + y), top))
    return corners, head


def _box_rows(rows, count, scores, score_thr):
    rows = np.asarray(rows, dtype=np.float32)
    M = rows.shape[0]
    count = M if count is None else min(max(int(count), 0), M)
    for m in range(count):
        if scores is not None and not F(scores[m]) > F(score_thr):      # the threshold is a float32 of the args
            continue
        if box_valid(rows[m]):
            yield m, rows[m]


def _box_rgb(m, labels, class_rgb, rgb_default):
    if labels is not None and class_rgb is not None and 0 <= int(labels[m]) < len(class_rgb):
        return int(class_rgb[int(labels[m])])
    return int(rgb_default)


def boxes(pl, views, near, layer, rows, *, z_origin=0.5, count=None, labels=None, scores=None, score_thr=0.0,
          class_rgb=None, rgb_default=0xFFFFFF, thickness=1):
    for m, r in _box_rows(rows, count, scores, score_thr):
        key = pack(layer, 0xFFFFFFFF - m, _box_rgb(m, labels, class_rgb, rgb_default))
        corners, head = box_corners32(r, z_origin)
        for v in range(pl.V):
            for i, j in BOX_EDGES:
                segment(pl, v, views[v], near, corners[i], corners[j], thickness, key)
            segment(pl, v, views[v], near, head[0], head[1], thickness, key)


# ---- (b): float64 geometry -------------------------------------------------------------------------------------

def clip_ends64(view, near, a, b, W, H):
    m = np.asarray(view, dtype=np.float64)
    A = m @ np.array([*a, 1.0])
    B = m @ np.array([*b, 1.0])
    ina, inb = A[3] >= near, B[3] >= near
    if not ina and not inb:
        return None
    if ina != inb:
        t = (near - A[3]) / (B[3] - A[3])
        C = A + t * (B - A)
        C[3] = near
        if ina:
            B = C
        else:
            A = C
    ua, va, ub, vb = A[0] / A[3], A[1] / A[3], B[0] / B[3], B[1] / B[3]
    dx, dy = ub - ua, vb - va
    t0, t1 = 0.0, 1.0
    for p, q in ((-dx, ua + 1.0), (dx, W + 1.0 - ua), (-dy, va + 1.0), (dy, H + 1.0 - va)):
        if p == 0:
            if q < 0:
                return None
            continue
        r = q / p
        if p < 0:
            if r > t1:
                return None
            t0 = max(t0, r)
        else:
            if r < t0:
                return None
            t1 = min(t1, r)
    xa, ya = (ua + t0 * dx, va + t0 * dy) if t0 > 0 else (ua, va)
    xb, yb = (ua + t1 * dx, va + t1 * dy) if t1 < 1 else (ub, vb)
    return (_floor_clamp(xa, -2, W + 2), _floor_clamp(ya, -2, H + 2), _floor_clamp(xb, -2, W + 2),
            _floor_clamp(yb, -2, H + 2))


def box_corners64(r, z_origin):
    x, y, z, dx, dy, dz, yaw = [float(t) for t in r[:7]]
    hx, hy, s, c = dx / 2, dy / 2, math.sin(yaw), math.cos(yaw)
    bot = z - z_origin * dz
    top = bot + dz
    xy = [(sx * hx * c - sy * hy * s + x, sx * hx * s + sy * hy * c + y) for sx, sy in ((-1, -1), (-1, 1), (1, 1), (1, -1))]
    corners = [(X, Y, bot) for X, Y in xy] + [(X, Y, top) for X, Y in xy]
    return corners, ((x, y, top), (hx * c + x, hx * s + y, top))


def boxes64(pl, views, near, layer, rows, *, z_origin=0.5, count=None, labels=None, scores=None, score_thr=0.0,
            class_rgb=None, rgb_default=0xFFFFFF, thickness=1):
    for m, r in _box_rows(rows, count, scores, score_thr):
        key = pack(layer, 0xFFFFFFFF - m, _box_rgb(m, labels, class_rgb, rgb_default))
        corners, head = box_corners64(r, z_origin)
        for v in range(pl.V):
            for a, b in [(corners[i], corners[j]) for i, j in BOX_EDGES] + [head]:
                ends = clip_ends64(views[v], near, a, b, pl.W, pl.H)
                if ends is not None:
                    draw_walk(pl, v, ends, thickness, key)


# ---- digits and resolve ----------------------------------------------------------------------------------------

def digits(pl, views, near, layer, values, anchors, *, rgb=None, rgb_one=0xFFFFFF, rank=None, scale=1, planar=False):
    with np.errstate(all="ignore"):
        for m, value in enumerate(values):
            value = int(value)
            if value < 0:
                continue
            r = m if rank is None else max(int(rank[m]), 0)
            key = pack(layer, 0xFFFFFFFF - r, int(rgb[m]) if rgb is not None else rgb_one)
            for v in range(pl.V):
                if planar:
                    u, w = F(anchors[m][0]), F(anchors[m][1])
                else:
                    x, y, z = [F(t) for t in anchors[m][:3]]
                    if not fin(x, y, z):
                        continue
                    r3 = row(views[v], 3, x, y, z)
                    if not r3 >= F(near):
                        continue
                    u, w = F(row(views[v], 0, x, y, z) / r3), F(row(views[v], 1, x, y, z) / r3)
                if not (u >= -65536 and u < 65536 and w >= -65536 and w < 65536):
                    continue
                X0, Y0 = int(math.floor(float(u))), int(math.floor(float(w)))
                for j, ch in enumerate(str(value)):
                    for cy in range(7):
                        for cx in range(5):
                            if (FONT[int(ch)][cy] >> (4 - cx)) & 1:
                                for l in range(scale):
                                    for i in range(scale):
                                        pl.put(v, X0 + (6 * j + cx) * scale + i, Y0 + cy * scale + l, key)


def resolve(pl, background=0, src=None):
    """-> uint8 [V][H][W][3]"""
    k = pl.k
    rgb = (k & np.uint64(0xFFFFFF)).astype(np.uint32)
    out = np.stack([(rgb >> 16) & 0xFF, (rgb >> 8) & 0xFF, rgb & 0xFF], axis=-1).astype(np.uint8)
    empty = k == 0
    if src is not None:
        out[empty] = np.asarray(src, dtype=np.uint8)[empty]
    else:
        out[empty] = [(background >> 16) & 0xFF, (background >> 8) & 0xFF, background & 0xFF]
    return out
