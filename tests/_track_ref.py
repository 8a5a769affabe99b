"""The tracker contract of include/cmt_hip.h restated in numpy, for the tests.

Three separate functions, so each device stage can be fed the other stages' actual outputs:
``predict_cost`` (cmt_track_predict) and ``update`` (cmt_track_update), every operation a single float32 operation
in the contract's order, and ``assign`` (scipy on the float32 cost matrix).  ``run_scene`` is the same algorithm in
float64 over a whole scene, for the id-purity property.
"""
import numpy as np
from scipy.optimize import linear_sum_assignment

F = np.float32
BIG = F(1.0e6)
PI_F, TWO_PI_F = F(3.1415927), F(6.2831855)


def fresh_state(T, H):
    ti = np.zeros((T, 8), np.int32)
    ti[:, 0] = -1
    return dict(trk_f=np.zeros((T, 16), F), trk_i=ti, hist=np.zeros((T, H, 3), F), counters=np.zeros(4, np.int32))


def copy_state(st):
    return {k: v.copy() for k, v in st.items()}


def pose_yaw(pose):
    """atan2(R10, R00) in float64, rounded once"""
    p = np.asarray(pose, np.float64)
    return F(np.arctan2(p[1, 0], p[0, 0]))


def predict_cost(st, det, scores, labels, count, dt, q_pos, q_vel, score_thr, gate2, pose=None, pose_yaw_f=None,
                 cost_init=None):
    """-> dict(det_w, det_ok, live, n_live, n_det, cost [T, D], desc); ``st`` is predicted in place.
    ``cost_init``: the value of the entries the contract does not write."""
    tf, ti = st["trk_f"], st["trk_i"]
    T, D = tf.shape[0], det.shape[0]
    gate2 = np.asarray(gate2, F)
    ncls = gate2.shape[0]
    dt, q_pos, q_vel, score_thr = F(dt), F(q_pos), F(q_vel), F(score_thr)
    n_det = D if count is None else min(max(int(count), 0), D)
    with np.errstate(all="ignore"):
        det_w = np.ascontiguousarray(det[:, :9]).astype(F).copy()
        if pose is not None:
            m = np.asarray(pose, F)
            x, y, z, vx, vy = (det[:, k].astype(F) for k in (0, 1, 2, 7, 8))
            for a in range(3):
                det_w[:, a] = ((m[a, 0] * x + m[a, 1] * y) + m[a, 2] * z) + m[a, 3]
            det_w[:, 7] = m[0, 0] * vx + m[0, 1] * vy
            det_w[:, 8] = m[1, 0] * vx + m[1, 1] * vy
            yaw = det[:, 6].astype(F) + F(pose_yaw_f)
            hi, lo = yaw >= PI_F, yaw < -PI_F
            yaw = np.where(hi, yaw - TWO_PI_F, np.where(lo, yaw + TWO_PI_F, yaw)).astype(F)
            det_w[:, 6] = yaw
        fin = np.isfinite(det_w).all(1)
        det_ok = ((np.arange(D) < n_det) & fin & (labels >= 0) & (labels < ncls) & (scores >= score_thr)).astype(np.int32)
        alive = ti[:, 0] >= 0
        qp, qv = q_pos * dt, q_vel * dt
        for p_, v_, pp in ((0, 7, 10), (1, 8, 13)):
            Ppp, Ppv, Pvv = tf[alive, pp].copy(), tf[alive, pp + 1].copy(), tf[alive, pp + 2].copy()
            tf[alive, p_] = tf[alive, p_] + dt * tf[alive, v_]
            t1 = Ppv + dt * Pvv
            tf[alive, pp] = (Ppp + dt * (Ppv + t1)) + qp
            tf[alive, pp + 1] = t1
            tf[alive, pp + 2] = Pvv + qv
        ti[alive, 4] += 1
        live = np.nonzero(alive)[0].astype(np.int32)
        n_live = live.shape[0]
        cost = np.full((T, D), np.nan if cost_init is None else cost_init, F)
        if n_live and n_det:
            ex = tf[live, 0][:, None] - det_w[None, :n_det, 0]
            ey = tf[live, 1][:, None] - det_w[None, :n_det, 1]
            d2 = (ex * ex + ey * ey).astype(F)
            lab = labels[:n_det]
            g = np.where(det_ok[:n_det] != 0, gate2[np.clip(lab, 0, ncls - 1)], F(0))
            ok = (det_ok[None, :n_det] != 0) & (lab[None, :] == ti[live, 1][:, None]) & (d2 < g[None, :])
            cost[:n_live, :n_det] = np.where(ok, d2, BIG)
    assert tf.dtype == F and det_w.dtype == F and cost.dtype == F
    return dict(det_w=det_w, det_ok=det_ok, live=live, n_live=n_live, n_det=n_det, cost=cost,
                desc=np.array([0, n_live, n_det, D], np.int64))


def assign(cost, n_live, n_det):
    """scipy on the float32 matrix -> (match_g [n_live], match_q [n_det], total in float64, ascending row order)"""
    mg, mq = np.full(n_live, -1, np.int32), np.full(n_det, -1, np.int32)
    total = 0.0
    if n_live and n_det:
        rows, cols = linear_sum_assignment(cost[:n_live, :n_det].astype(np.float64))
        mg[rows], mq[cols] = cols, rows
        for r in np.sort(rows):
            total += float(cost[r, mg[r]])
    return mg, mq, total


def _axis_update(f, ip, iv, ipp, zp, zv, use_velocity, r_pos, r_vel):
    pos, vel, Ppp, Ppv, Pvv = f[ip], f[iv], f[ipp], f[ipp + 1], f[ipp + 2]
    if use_velocity:
        Spp, Spv, Svv = Ppp + r_pos, Ppv, Pvv + r_vel
        det = Spp * Svv - Spv * Spv
        K00 = (Ppp * Svv - Ppv * Spv) / det
        K01 = (Ppv * Spp - Ppp * Spv) / det
        K10 = (Ppv * Svv - Pvv * Spv) / det
        K11 = (Pvv * Spp - Ppv * Spv) / det
        yp, yv = zp - pos, zv - vel
        f[ip] = pos + (K00 * yp + K01 * yv)
        f[iv] = vel + (K10 * yp + K11 * yv)
        f[ipp] = Ppp - (K00 * Ppp + K01 * Ppv)
        f[ipp + 1] = Ppv - (K00 * Ppv + K01 * Pvv)
        f[ipp + 2] = Pvv - (K10 * Ppv + K11 * Pvv)
    else:
        S = Ppp + r_pos
        K0, K1 = Ppp / S, Ppv / S
        y = zp - pos
        f[ip] = pos + K0 * y
        f[iv] = vel + K1 * y
        f[ipp] = Ppp - K0 * Ppp
        f[ipp + 1] = Ppv - K0 * Ppv
        f[ipp + 2] = Pvv - K1 * Ppv


def update(st, live, n_live, n_det, cost, match_g, match_q, det_w, scores, labels, det_ok, *, use_velocity, r_pos,
           r_vel, p0_pos, p0_vel, birth_thr, max_age, dtype=F):
    """cmt_track_update on ``st`` in place -> (det_track [D], det_slot [D]).  Scalars of ``dtype`` (float32: every
    operation a single float32 operation, numpy scalars do not promote)."""
    tf, ti, hist, cnt = st["trk_f"], st["trk_i"], st["hist"], st["counters"]
    T, H, D = tf.shape[0], hist.shape[1], det_w.shape[0]
    r_pos, r_vel, p0_pos, p0_vel, birth_thr = (dtype(v) for v in (r_pos, r_vel, p0_pos, p0_vel, birth_thr))
    n_live, n_det = min(max(int(n_live), 0), T), min(max(int(n_det), 0), D)
    true_live = np.nonzero(ti[:, 0] >= 0)[0]
    n_live = min(n_live, true_live.shape[0])
    slot_match, dslot = np.full(T, -1, np.int64), np.full(D, -1, np.int64)
    big = dtype(BIG)
    for r in range(n_live):
        s = int(true_live[r])
        if int(live[r]) != s:
            continue
        j = int(match_g[r])
        if j < 0 or j >= n_det or int(match_q[j]) != r or det_ok[j] == 0 or not cost[r, j] < big:
            continue
        slot_match[s], dslot[j] = j, s
    with np.errstate(all="ignore"):
        for s in range(T):
            if ti[s, 0] < 0:
                continue
            j = int(slot_match[s])
            if j >= 0:
                f, d = tf[s], det_w[j]
                _axis_update(f, 0, 7, 10, d[0], d[7], use_velocity, r_pos, r_vel)
                _axis_update(f, 1, 8, 13, d[1], d[8], use_velocity, r_pos, r_vel)
                f[2:7] = d[2:7]
                f[9] = scores[j]
                ti[s, 2] += 1
                ti[s, 3], ti[s, 5] = 0, j
                hist[s, ti[s, 6] % H] = f[:3]
                ti[s, 6] += 1
            else:
                ti[s, 3] += 1
                ti[s, 5] = -1
                if ti[s, 3] > max_age:
                    ti[s, 0] = -1
    free = np.nonzero(ti[:, 0] < 0)[0]
    det_track, det_slot = np.full(D, -1, np.int32), np.full(D, -1, np.int32)
    m = dslot >= 0
    det_slot[m] = dslot[m]
    det_track[m] = ti[dslot[m], 0]
    next_id, k = int(cnt[1]), 0
    for j in range(n_det):
        if det_ok[j] == 0 or dslot[j] >= 0 or not scores[j] >= birth_thr:
            continue
        if k < free.shape[0]:
            s, d = int(free[k]), det_w[j]
            tf[s, :7] = d[:7]
            tf[s, 7:9] = d[7:9] if use_velocity else 0
            tf[s, 9] = scores[j]
            tf[s, 10:16] = (p0_pos, 0, p0_vel, p0_pos, 0, p0_vel)
            ti[s] = (next_id + k, labels[j], 1, 0, 0, j, 1, 0)
            hist[s, 0] = d[:3]
            det_track[j], det_slot[j] = next_id + k, s
        k += 1
    placed = min(k, free.shape[0])
    cnt[0] = T - free.shape[0] + placed
    cnt[1] = next_id + placed
    cnt[2] += k - placed
    cnt[3] += 1
    return det_track, det_slot


def history(st, s):
    """the unrolled ring of slot s, oldest first"""
    H = st["hist"].shape[1]
    n = int(st["trk_i"][s, 6])
    if n <= H:
        return st["hist"][s, :n].copy()
    return np.roll(st["hist"][s], -(n % H), axis=0).copy()


def run_scene(frames, ncls, *, gate=2.0, score_thr=0.1, birth_thr=0.3, max_age=3, use_velocity=False, q_pos=0.5,
              q_vel=1.0, r_pos=0.1, r_vel=1.0, p0_pos=1.0, p0_vel=10.0, max_tracks=256, history_len=16, dt=0.1):
    """The whole algorithm in float64 over ``frames`` (a list of (boxes [n, 9], scores [n], labels [n])); the first
    frame uses dt = 0 -> the list of det_track arrays and the final state."""
    D = max(len(f[1]) for f in frames)
    st = fresh_state(max_tracks, history_len)
    st["trk_f"], st["hist"] = st["trk_f"].astype(np.float64), st["hist"].astype(np.float64)
    gate2 = np.full(ncls, gate * gate, np.float64)
    out = []
    for t, (boxes, scores, labels) in enumerate(frames):
        n = len(scores)
        det = np.zeros((D, 9), np.float64)
        sc, lab = np.zeros(D, np.float64), np.zeros(D, np.int32)
        det[:n], sc[:n], lab[:n] = boxes, scores, labels
        tf, ti = st["trk_f"], st["trk_i"]
        step = 0.0 if t == 0 else dt
        alive = ti[:, 0] >= 0
        for p_, v_, pp in ((0, 7, 10), (1, 8, 13)):
            Ppp, Ppv, Pvv = tf[alive, pp].copy(), tf[alive, pp + 1].copy(), tf[alive, pp + 2].copy()
            tf[alive, p_] += step * tf[alive, v_]
            t1 = Ppv + step * Pvv
            tf[alive, pp] = Ppp + step * (Ppv + t1) + q_pos * step
            tf[alive, pp + 1] = t1
            tf[alive, pp + 2] = Pvv + q_vel * step
        ti[alive, 4] += 1
        live = np.nonzero(alive)[0]
        det_ok = ((np.arange(D) < n) & np.isfinite(det).all(1) & (lab >= 0) & (lab < ncls) & (sc >= score_thr)).astype(np.int32)
        cost = np.full((max_tracks, D), 1.0e6)
        if len(live) and n:
            d2 = (tf[live, 0][:, None] - det[None, :n, 0]) ** 2 + (tf[live, 1][:, None] - det[None, :n, 1]) ** 2
            ok = (det_ok[None, :n] != 0) & (lab[None, :n] == ti[live, 1][:, None]) & (d2 < gate2[np.clip(lab[:n], 0, ncls - 1)][None])
            cost[:len(live), :n] = np.where(ok, d2, 1.0e6)
        mg, mq, _ = assign(cost, len(live), n)
        trk, _ = update(st, live, len(live), n, cost, mg, mq, det, sc, lab, det_ok, use_velocity=use_velocity,
                        r_pos=r_pos, r_vel=r_vel, p0_pos=p0_pos, p0_vel=p0_vel, birth_thr=birth_thr, max_age=max_age,
                        dtype=np.float64)
        out.append(trk[:n].copy())
    return out, st


def ids_per_object(frames, tracks):
    """{object: the set of track ids its boxes carried} over ``synthetic.moving_scene`` frames and their det_track rows"""
    ids = {}
    for f, t in zip(frames, tracks):
        for o, k in zip(f["object"][:f["count"]], t[:f["count"]]):
            if o >= 0:
                ids.setdefault(int(o), set()).add(int(k))
    return ids
