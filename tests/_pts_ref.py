"""The contract of cmt_pts_prepare (include/cmt_hip.h) restated in numpy, for the tests.

Steps 2 and 5 are written element by element so that the order of the products and sums is the contract's (no
``@``: a BLAS chooses its own order and may fuse).  numpy's float64 / float32 scalar-array arithmetic rounds every
operation once and never fuses, which is what the contract asks for.
"""
import numpy as np

QNAN = np.uint32(0x7FC00000)


def rigid(rng, max_trans):
    """a seeded rigid transform, float64: any yaw, roll and pitch within 0.05 rad, translation within max_trans"""
    yaw, pitch, roll = rng.uniform(-np.pi, np.pi), rng.uniform(-0.05, 0.05), rng.uniform(-0.05, 0.05)
    cz, sz, cy, sy, cx, sx = np.cos(yaw), np.sin(yaw), np.cos(pitch), np.sin(pitch), np.cos(roll), np.sin(roll)
    rz = np.array([[cz, -sz, 0], [sz, cz, 0], [0, 0, 1.0]])
    ry = np.array([[cy, 0, sy], [0, 1.0, 0], [-sy, 0, cy]])
    rx = np.array([[1.0, 0, 0], [0, cx, -sx], [0, sx, cx]])
    return rz.dot(ry).dot(rx), rng.uniform(-max_trans, max_trans, 3)


def seg(points, rotation=None, translation=None, remove_close=0.0, time_col=None, time=None):
    """a segment dict in prepare_points' form, from numpy rows"""
    return dict(points=np.ascontiguousarray(points, dtype=np.float32), rotation=rotation, translation=translation,
                remove_close=remove_close, time_col=time_col, time=time)


def sweep_xform(xyz, rot, trans):
    """step 2: float64 products and sums left to right, one rounding to float32, then the float64 add"""
    rot = np.asarray(rot, np.float64).reshape(3, 3)
    trans = np.asarray(trans, np.float64).reshape(3)
    x, y, z = (xyz[:, k].astype(np.float64) for k in range(3))
    out = np.empty((xyz.shape[0], 3), np.float32)
    for k in range(3):
        q = ((x * rot[k, 0] + y * rot[k, 1]) + z * rot[k, 2]).astype(np.float32)
        out[:, k] = (q.astype(np.float64) + trans[k]).astype(np.float32)
    return out


def agent_xform(xyz, rot32, trans32):
    """step 5: float32 products and sums left to right, every one rounded"""
    r = np.asarray(rot32, np.float32).reshape(3, 3)
    t = np.asarray(trans32, np.float32).reshape(3)
    x, y, z = (xyz[:, k].astype(np.float32) for k in range(3))
    out = np.empty((xyz.shape[0], 3), np.float32)
    for k in range(3):
        out[:, k] = ((x * r[k, 0] + y * r[k, 1]) + z * r[k, 2]) + t[k]
    return out


def range_mask(xyz, rng):
    rng = np.asarray(rng, np.float32)
    with np.errstate(invalid="ignore"):
        return np.all((xyz > rng[:3]) & (xyz < rng[3:]), axis=1)


def reference(segments, use_dim, agent=None, rng=None):
    """-> (kept rows [count, F_out] float32 in input order, keep mask over all n_total rows).
    ``agent``: None or (rot 3 x 3, trans 3), rounded to float32 here; ``rng``: None or 6 values."""
    use = list(use_dim)
    rows, masks = [], []
    with np.errstate(invalid="ignore", over="ignore"):
        for s in segments:
            p = np.array(s["points"], dtype=np.float32, copy=True)
            r = np.float32(1.0 if s.get("remove_close") is True else (s.get("remove_close") or 0.0))
            keep = ~((np.abs(p[:, 0]) < r) & (np.abs(p[:, 1]) < r))
            if s.get("rotation") is not None or s.get("translation") is not None:
                rot = np.eye(3) if s.get("rotation") is None else s["rotation"]
                trans = np.zeros(3) if s.get("translation") is None else s["translation"]
                p[:, :3] = sweep_xform(p[:, :3], rot, trans)
            if s.get("time_col") is not None:
                p[:, s["time_col"]] = np.float32(s["time"])
            o = np.ascontiguousarray(p[:, use])
            if agent is not None:
                o[:, :3] = agent_xform(o[:, :3], np.asarray(agent[0]).astype(np.float32),
                                       np.asarray(agent[1]).astype(np.float32))
            if rng is not None:
                keep &= range_mask(o[:, :3], rng)
            rows.append(o)
            masks.append(keep)
    allrows = np.concatenate(rows, 0) if rows else np.zeros((0, len(use)), np.float32)
    mask = np.concatenate(masks, 0) if masks else np.zeros((0,), bool)
    return allrows[mask], mask


def padded(segments, use_dim, agent=None, rng=None):
    """the whole expected destination as uint32 words: kept rows, then quiet NaN"""
    kept, mask = reference(segments, use_dim, agent, rng)
    out = np.full((mask.size, len(list(use_dim))), QNAN, np.uint32)
    out[:kept.shape[0]] = kept.view(np.uint32)
    return out, int(kept.shape[0])
