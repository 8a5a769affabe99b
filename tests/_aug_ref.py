"""The contracts of cmt_points_in_boxes, cmt_pts_augment and cmt_boxes_augment (include/cmt_hip.h) restated in
numpy, for the tests.

The transforms are float32 with every product and sum rounded on its own (numpy's float32 array arithmetic never
fuses; no ``@``, whose order a BLAS chooses).  The inside test is float64: the contract binds only points farther
than ``margin`` from every face plane, and ``inside_inputs`` builds such points and asserts that they are.
"""
import numpy as np

QNAN = np.uint32(0x7FC00000)
PI32 = np.float32(np.pi)
TWO_PI32 = np.float32(2 * np.pi)


def rot32(angle):
    """R of BasePoints.rotate(angle), built in float64 and rounded once"""
    c, s = np.cos(np.float64(angle)), np.sin(np.float64(angle))
    return np.array([[c, -s, 0], [s, c, 0], [0, 0, 1]], np.float64).astype(np.float32)


# ---- the inside test ---------------------------------------------------------------------------------------------
def face_distances(points, boxes):
    """float64 [N, M, 6]: the signed distances of every point to the six face planes of every box (positive on the
    box's side of the plane), and the local coordinates they come from"""
    p = np.asarray(points, np.float64)[:, None, :3]
    b = np.asarray(boxes, np.float64)[None, :, :]
    d = p - b[..., :3]
    c, s = np.cos(b[..., 6]), np.sin(b[..., 6])
    lx = d[..., 0] * c + d[..., 1] * s
    ly = -d[..., 0] * s + d[..., 1] * c
    hx, hy = b[..., 3] / 2, b[..., 4] / 2
    return np.stack([hx - lx, hx + lx, hy - ly, hy + ly, d[..., 2], b[..., 5] - d[..., 2]], -1)


def inside(points, boxes):
    """bool [N, M]: the open interior, float64; a NaN anywhere gives False"""
    points, boxes = np.asarray(points, np.float32), np.asarray(boxes, np.float32)
    if points.shape[0] == 0 or boxes.shape[0] == 0:
        return np.zeros((points.shape[0], boxes.shape[0]), bool)
    with np.errstate(invalid="ignore"):
        return np.all(face_distances(points, boxes) > 0, -1)


def margin(points, boxes):
    """the contract's margin per (point, box): 1e-4 * (1 + max |coordinate| of the point and the box centre)"""
    p = np.abs(np.asarray(points, np.float64)[:, None, :3]).max(-1)
    b = np.abs(np.asarray(boxes, np.float64)[None, :, :3]).max(-1)
    return 1e-4 * (1 + np.maximum(p, b))


def assert_clear_of_faces(points, boxes):
    """the condition on the test's inputs: every finite point is farther than the margin from every face plane of
    every finite box (checked on the CPU, in float64)"""
    points, boxes = np.asarray(points, np.float32), np.asarray(boxes, np.float32)
    if points.shape[0] == 0 or boxes.shape[0] == 0:
        return
    with np.errstate(invalid="ignore"):
        d = np.abs(face_distances(points, boxes))
        near = d <= margin(points, boxes)[..., None]     # NaN compares false: a NaN point or box binds nothing
    assert not near.any(), f"{int(near.sum())} point-face pairs lie inside the contract's margin"


def inside_inputs(rng, n, boxes, F=5, clear=1e-3):
    """n float32 points [n, F] around ``boxes`` (float32 [M, >= 7], finite, extents above 4 * clear), about half of
    them inside some box: each is drawn in one box's local frame at least ``clear`` metres from every face, mapped
    to the world in float64 and rounded.  Points that come within the contract's margin of a face of ANY box (boxes
    may overlap) are drawn again; the result is asserted clear."""
    boxes = np.asarray(boxes, np.float32)
    M = boxes.shape[0]
    out = np.zeros((n, F), np.float32)
    out[:, 3:] = rng.uniform(0, 255, (n, F - 3)).astype(np.float32)
    if M == 0:
        out[:, :3] = rng.uniform(-20, 20, (n, 3)).astype(np.float32)
        return out
    todo = np.arange(n)
    for _ in range(50):
        if todo.size == 0:
            break
        b = boxes[rng.integers(0, M, todo.size)].astype(np.float64)
        want_in = rng.random(todo.size) < 0.5
        h = np.stack([b[:, 3] / 2, b[:, 4] / 2, b[:, 5] / 2], 1)
        u = rng.uniform(-1, 1, (todo.size, 3))
        loc_in = u * (h - clear)                                        # at least `clear` inside every face
        axis = rng.integers(0, 3, todo.size)
        loc_out = u * (h + 2.0)
        beyond = np.sign(u[np.arange(todo.size), axis] + 1e-30) * (h[np.arange(todo.size), axis] + clear + np.abs(
            rng.normal(0, 1.0, todo.size)))
        loc_out[np.arange(todo.size), axis] = beyond                    # at least `clear` beyond one face
        loc = np.where(want_in[:, None], loc_in, loc_out)
        c, s = np.cos(b[:, 6]), np.sin(b[:, 6])
        w = np.stack([b[:, 0] + loc[:, 0] * c - loc[:, 1] * s, b[:, 1] + loc[:, 0] * s + loc[:, 1] * c,
                      b[:, 2] + h[:, 2] + loc[:, 2]], 1).astype(np.float32)
        out[todo, :3] = w
        d = np.abs(face_distances(w, boxes))
        bad = (d <= 2 * margin(w, boxes)[..., None]).any((1, 2))
        todo = todo[bad]
    assert todo.size == 0, "could not place every point clear of every face"
    assert_clear_of_faces(out, boxes)
    return out


def points_in_boxes(points, boxes, count=None):
    """-> (box_of_point int32 [N], count_per_box int32 [M])"""
    points = np.asarray(points, np.float32)
    m = inside(points, boxes)
    if count is not None:
        m[max(0, min(int(count), points.shape[0])):] = False
    first = np.where(m.any(1), m.argmax(1), -1).astype(np.int32) if m.shape[1] else np.full(points.shape[0], -1, np.int32)
    return first, m.sum(0).astype(np.int32)


# ---- the transforms ----------------------------------------------------------------------------------------------
def rotate_xyz(xyz, R):
    """p'_k = fl32(fl32(fl32(x * R[k, 0]) + fl32(y * R[k, 1])) + fl32(z * R[k, 2]))"""
    R = np.asarray(R, np.float32)
    x, y, z = (xyz[:, k].astype(np.float32) for k in range(3))
    out = np.empty((xyz.shape[0], 3), np.float32)
    for k in range(3):
        out[:, k] = (x * R[k, 0] + y * R[k, 1]) + z * R[k, 2]
    return out


def xform_xyz(xyz, params):
    """rotation, scale, translation and the flips on [n, 3] float32"""
    p = np.array(xyz, np.float32, copy=True)
    with np.errstate(invalid="ignore", over="ignore"):
        if params.get("angle") is not None:
            p = rotate_xyz(p, rot32(params["angle"]))
        if params.get("scale") is not None:
            p = p * np.float32(params["scale"])
        if params.get("trans") is not None:
            p = p + np.asarray(params["trans"], np.float32).reshape(1, 3)
    if params.get("flip_h"):
        p[:, 1] = -p[:, 1]
    if params.get("flip_v"):
        p[:, 0] = -p[:, 0]
    return p


def range_mask(xyz, rng):
    rng = np.asarray(rng, np.float32)
    with np.errstate(invalid="ignore"):
        return np.all((xyz > rng[:3]) & (xyz < rng[3:]), axis=1)


def augment_points(src, params, count=None, paste=None, paste_boxes=None, paste_first=False, rng=None, order=None):
    """-> the kept rows [count, F] float32 in slot order"""
    src = np.asarray(src, np.float32)
    F = src.shape[1]
    n_src = src.shape[0]
    paste = np.zeros((0, F), np.float32) if paste is None else np.asarray(paste, np.float32)
    n_in = n_src + paste.shape[0]
    alive = np.ones(n_src, bool)
    if count is not None:
        alive[max(0, min(int(count), n_src)):] = False
    if paste_boxes is not None and len(paste_boxes):
        alive &= ~inside(src, np.asarray(paste_boxes, np.float32)[:, :7]).any(1)
    rows = np.concatenate([paste, src] if paste_first else [src, paste], 0)
    keep = np.concatenate([np.ones(paste.shape[0], bool), alive] if paste_first else [alive, np.ones(paste.shape[0], bool)])
    rows = rows.copy()
    rows[:, :3] = xform_xyz(rows[:, :3], params)
    if rng is not None:
        keep &= range_mask(rows[:, :3], rng)
    if order is None:
        visit = np.arange(n_in)
    else:
        visit = np.asarray(order, np.int64)
        visit = visit[(visit >= 0) & (visit < n_in)]
    visit = visit[keep[visit]]
    return rows[visit]


def padded(kept, n, F):
    """the whole expected destination as uint32 words: kept rows, then quiet NaN"""
    out = np.full((n, F), QNAN, np.uint32)
    out[:kept.shape[0]] = np.ascontiguousarray(kept, np.float32).view(np.uint32)
    return out


def limit_yaw(yaw):
    """yaw - floor(yaw / P + 0.5) * P in float32, P = fl32(2 pi)"""
    yaw = np.asarray(yaw, np.float32)
    return yaw - np.floor(yaw / TWO_PI32 + np.float32(0.5)) * TWO_PI32


def augment_boxes(boxes, labels, params, rng=None, num_classes=10, gravity=False):
    """-> (kept boxes [count, D] float32, kept labels int64) in input order"""
    b = np.array(boxes, np.float32, copy=True)
    labels = np.asarray(labels, np.int64)
    D = b.shape[1]
    with np.errstate(invalid="ignore", over="ignore"):
        if params.get("angle") is not None:
            R = rot32(params["angle"])
            b[:, 6] = b[:, 6] + np.float32(params["angle"])
            if D == 9:
                vx, vy = b[:, 7].copy(), b[:, 8].copy()
                b[:, 7] = vx * R[0, 0] + vy * R[0, 1]
                b[:, 8] = vx * R[1, 0] + vy * R[1, 1]
        b[:, :3] = xform_xyz(b[:, :3], params)
        if params.get("scale") is not None:
            s = np.float32(params["scale"])
            b[:, 3:6] = b[:, 3:6] * s
            b[:, 7:] = b[:, 7:] * s
        if params.get("flip_h"):
            b[:, 8:9] = -b[:, 8:9]
            b[:, 6] = -b[:, 6]
        if params.get("flip_v"):
            b[:, 7:8] = -b[:, 7:8]
            b[:, 6] = -b[:, 6] + PI32
        keep = (labels >= 0) & (labels < num_classes)
        if rng is not None:
            r = np.asarray(rng, np.float32)
            keep &= (b[:, 0] > r[0]) & (b[:, 1] > r[1]) & (b[:, 0] < r[3]) & (b[:, 1] < r[4])
        b[:, 6] = limit_yaw(b[:, 6])
        if gravity:
            b[:, 2] = b[:, 2] + b[:, 5] * np.float32(0.5)
    return b[keep], labels[keep]
