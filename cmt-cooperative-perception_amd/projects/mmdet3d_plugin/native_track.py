"""The multi-object tracker on the device: cmt_track_predict and cmt_track_update (include/cmt_hip.h) with cmt_lsap
between them, and ``Tracker``, which gives the boxes of successive frames stable track ids.

``track_predict`` and ``track_update`` are the thin wrappers of the two calls.  ``Tracker.step`` takes one frame's
decoded boxes as ``cmt_box_decode`` leaves them on the device (boxes, scores, labels, count), runs predict ->
cmt_lsap -> update on buffers allocated once, and returns the track id of every detection row, still on the device:
five small launches, no host read and no synchronisation.  ``Tracker.tracks`` is the one place that reads the state
back.  The motion model is a constant-velocity Kalman filter per ground-plane axis, the association minimises the
sum of squared centre distances over pairs of equal class inside a per-class gate.

Like native_aug.py: argument checks raise ValueError before the device check, tensors must live on a HIP device,
there is no CPU fallback.
"""
import ctypes
import math

import numpy as np
import torch

from . import native as N
from ._argcheck import (count_word, nonneg as _nonneg, pose_arguments, positive as _positive, same_device, strided_rows,
                        tensor as _t)
from .native import _check, _p, _stream, lib

__all__ = ["MAX_TRACKS", "MAX_DETS", "MAX_HISTORY", "MAX_CLASSES", "BIG", "MAX_GATE2", "new_state", "track_predict",
           "track_update", "Tracker", "tracker_from_config"]

MAX_TRACKS, MAX_DETS = N.TRACK_MAX_TRACKS, N.TRACK_MAX_DETS
MAX_HISTORY, MAX_CLASSES = N.TRACK_MAX_HISTORY, N.TRACK_MAX_CLASSES
BIG = N.TRACK_BIG
MAX_GATE2 = 1.0e5      # a squared gate must stay below it: every gated cost is then far below BIG


def _same_device(dev, **ts):
    same_device(dev, "the tracker needs tensors", **ts)


def _caps(T, D, H=None, ncls=None):
    if not 1 <= T <= MAX_TRACKS:
        raise ValueError(f"track slots must be 1..{MAX_TRACKS}, got {T}")
    if not 1 <= D <= MAX_DETS:
        raise ValueError(f"detection rows must be 1..{MAX_DETS}, got {D}")
    if H is not None and not 1 <= H <= MAX_HISTORY:
        raise ValueError(f"history must be 1..{MAX_HISTORY}, got {H}")
    if ncls is not None and not 1 <= ncls <= MAX_CLASSES:
        raise ValueError(f"classes must be 1..{MAX_CLASSES}, got {ncls}")


def new_state(max_tracks, history, device):
    """A fresh tracker state on ``device``: dict(trk_f [T, 16] fp32, trk_i [T, 8] int32, hist [T, H, 3] fp32,
    counters [4] int32), every id -1 and everything else zero."""
    _caps(int(max_tracks), 1, int(history))
    trk_i = torch.zeros((max_tracks, 8), dtype=torch.int32, device=device)
    trk_i[:, 0] = -1
    return dict(trk_f=torch.zeros((max_tracks, 16), dtype=torch.float32, device=device), trk_i=trk_i,
                hist=torch.zeros((max_tracks, history, 3), dtype=torch.float32, device=device),
                counters=torch.zeros(4, dtype=torch.int32, device=device))


def _state(state, need_hist):
    if not isinstance(state, dict) or any(k not in state for k in ("trk_f", "trk_i", "hist", "counters")):
        raise ValueError("state must be the dict of new_state (trk_f, trk_i, hist, counters)")
    trk_f = _t(state["trk_f"], "trk_f", torch.float32, (None, 16))
    T = int(trk_f.shape[0])
    trk_i = _t(state["trk_i"], "trk_i", torch.int32, (T, 8))
    hist = _t(state["hist"], "hist", torch.float32, (T, None, 3)) if need_hist else state["hist"]
    counters = _t(state["counters"], "counters", torch.int32, (4,))
    return trk_f, trk_i, hist, counters, T


def track_predict(state, det, scores, labels, count, gate2, work, *, dt, q_pos, q_vel, score_thr, pose=None,
                  gate2_host=None):
    """cmt_track_predict.  ``state``: the dict of ``new_state``; ``det`` fp32 [D, >= 9] (rows may be a view with a
    row stride: ``det.stride(0)`` is passed), ``scores`` fp32 [D], ``labels`` int32 [D], ``count`` None or a device
    int32 of one element; ``gate2`` device fp32 [ncls], the squared gates, with ``gate2_host`` their host copy (the
    wrapper refuses an entry >= 1e5 or not finite there; None reads ``gate2`` back, once, for the check);
    ``work``: dict(det_w [D, 9] fp32, det_ok [D] int32, live [T] int32, cost [T, D] fp32, lsap_desc [1, 4] int64), all
    written.  No host read with ``gate2_host`` given."""
    trk_f, trk_i, _, _, T = _state(state, False)
    D, ld = strided_rows(det, "det", 9, rows="D")
    gate2 = _t(gate2, "gate2", torch.float32, (None,))
    ncls = int(gate2.shape[0])
    _caps(T, D, None, ncls)
    scores = _t(scores, "scores", torch.float32, (D,))
    labels = _t(labels, "labels", torch.int32, (D,))
    count_word(count)
    g = np.asarray(gate2.cpu() if gate2_host is None else gate2_host, dtype=np.float64).reshape(-1)
    if g.shape[0] != ncls or not np.isfinite(g).all() or (g < 0).any() or (g >= MAX_GATE2).any():
        raise ValueError(f"gate2 needs {ncls} finite entries in [0, {MAX_GATE2:g})")
    dt, q_pos, q_vel = _nonneg(dt, "dt"), _nonneg(q_pos, "q_pos"), _nonneg(q_vel, "q_vel")
    if math.isnan(float(score_thr)):
        raise ValueError("score_thr must not be NaN")
    det_w = _t(work["det_w"], "det_w", torch.float32, (D, 9))
    det_ok = _t(work["det_ok"], "det_ok", torch.int32, (D,))
    live = _t(work["live"], "live", torch.int32, (T,))
    cost = _t(work["cost"], "cost", torch.float32, (T, D))
    desc = _t(work["lsap_desc"], "lsap_desc", torch.int64, (1, 4))
    a = N.TrackPredictArgs()
    if pose is not None:
        m, yaw = pose if isinstance(pose, tuple) else pose_arguments(pose)
        a.has_pose, a.pose_yaw = 1, yaw
        for k in range(12):
            a.pose[k] = m[k]
    dev = trk_f.device
    _same_device(dev, trk_i=trk_i, det=det, scores=scores, labels=labels, count=count, gate2=gate2, det_w=det_w,
                 det_ok=det_ok, live=live, cost=cost, lsap_desc=desc)
    a.T, a.D, a.ld, a.ncls = T, D, ld, ncls
    a.dt, a.q_pos, a.q_vel, a.score_thr = dt, q_pos, q_vel, float(score_thr)
    a.trk_f, a.trk_i, a.det, a.scores, a.labels, a.count = _p(trk_f), _p(trk_i), _p(det), _p(scores), _p(labels), _p(count)
    a.gate2, a.det_w, a.det_ok, a.live, a.cost, a.lsap_desc = _p(gate2), _p(det_w), _p(det_ok), _p(live), _p(cost), _p(desc)
    _check(lib().cmt_track_predict(ctypes.byref(a), _stream()), "cmt_track_predict")


def track_update(state, work, match_g, match_q, scores, labels, det_track, det_slot, *, use_velocity, r_pos, r_vel,
                 p0_pos, p0_vel, birth_thr, max_age):
    """cmt_track_update.  ``work`` as ``track_predict`` wrote it, ``match_g`` int32 [T] and ``match_q`` int32 [D] as
    cmt_lsap wrote them, the ``scores`` and ``labels`` of ``track_predict``; ``det_track`` and ``det_slot`` int32 [D]
    are written.  No host read."""
    trk_f, trk_i, hist, counters, T = _state(state, True)
    scores = _t(scores, "scores", torch.float32, (None,))
    D, H = int(scores.shape[0]), int(hist.shape[1])
    _caps(T, D, H)
    labels = _t(labels, "labels", torch.int32, (D,))
    det_w = _t(work["det_w"], "det_w", torch.float32, (D, 9))
    det_ok = _t(work["det_ok"], "det_ok", torch.int32, (D,))
    live = _t(work["live"], "live", torch.int32, (T,))
    cost = _t(work["cost"], "cost", torch.float32, (T, D))
    desc = _t(work["lsap_desc"], "lsap_desc", torch.int64, (1, 4))
    match_g = _t(match_g, "match_g", torch.int32, (T,))
    match_q = _t(match_q, "match_q", torch.int32, (D,))
    det_track = _t(det_track, "det_track", torch.int32, (D,))
    det_slot = _t(det_slot, "det_slot", torch.int32, (D,))
    r_pos, r_vel = _positive(r_pos, "r_pos"), _positive(r_vel, "r_vel")
    p0_pos, p0_vel = _nonneg(p0_pos, "p0_pos"), _nonneg(p0_vel, "p0_vel")
    if math.isnan(float(birth_thr)):
        raise ValueError("birth_thr must not be NaN")
    if int(max_age) < 0:
        raise ValueError(f"max_age must not be negative, got {max_age}")
    dev = trk_f.device
    _same_device(dev, trk_i=trk_i, hist=hist, counters=counters, scores=scores, labels=labels, det_w=det_w, det_ok=det_ok,
                 live=live, cost=cost, lsap_desc=desc, match_g=match_g, match_q=match_q, det_track=det_track,
                 det_slot=det_slot)
    a = N.TrackUpdateArgs()
    a.T, a.D, a.H, a.use_velocity, a.max_age = T, D, H, int(bool(use_velocity)), int(max_age)
    a.r_pos, a.r_vel, a.p0_pos, a.p0_vel, a.birth_thr = r_pos, r_vel, p0_pos, p0_vel, float(birth_thr)
    a.trk_f, a.trk_i, a.hist, a.counters = _p(trk_f), _p(trk_i), _p(hist), _p(counters)
    a.live, a.lsap_desc, a.cost, a.match_g, a.match_q = _p(live), _p(desc), _p(cost), _p(match_g), _p(match_q)
    a.det_w, a.scores, a.labels, a.det_ok = _p(det_w), _p(scores), _p(labels), _p(det_ok)
    a.det_track, a.det_slot = _p(det_track), _p(det_slot)
    _check(lib().cmt_track_update(ctypes.byref(a), _stream()), "cmt_track_update")


class Tracker:
    """Stable track ids for the boxes of successive frames, on the device.

    ``class_names``: the classes of the labels (a track only takes boxes of its class); ``gate``: metres, one value
    or a dict {class name: metres} (classes it leaves out take 2.0): a box farther than it from a track's predicted
    centre cannot match it; boxes below ``score_thr`` are ignored, an unmatched box at or above ``birth_thr`` starts
    a track; a track without a box for more than ``max_age`` frames in a row ends; ``tracks()`` reports those with
    at least ``min_hits`` boxes.  ``use_velocity``: the boxes' velocity columns are measurements (and the initial
    velocity of a new track); False is for heads that learn no velocity (the TUMTraf annotations have none): the
    filter then estimates it from positions.  ``q_*`` process noise per second, ``r_*`` measurement variance,
    ``p0_*`` the variance of a new track.  THE DEFAULTS ARE PLAIN SETTINGS, not tuned on any dataset.

    The state, the cost matrix, cmt_lsap's workspace and the match arrays are allocated here, once."""

    def __init__(self, class_names, device, max_tracks=256, max_dets=300, history=16, gate=2.0, score_thr=0.1,
                 birth_thr=0.3, max_age=3, min_hits=2, use_velocity=False, q_pos=0.5, q_vel=1.0, r_pos=0.1, r_vel=1.0,
                 p0_pos=1.0, p0_vel=10.0):
        self.class_names = tuple(class_names)
        T, D, H, ncls = int(max_tracks), int(max_dets), int(history), len(self.class_names)
        _caps(T, D, H, ncls)
        if isinstance(gate, dict):
            unknown = set(gate) - set(self.class_names)
            if unknown:
                raise ValueError(f"gate names unknown classes {sorted(unknown)}")
            gates = [float(gate.get(n, 2.0)) for n in self.class_names]
        else:
            gates = [float(gate)] * ncls
        self._gate2_host = [float(np.float32(np.float32(g) * np.float32(g))) for g in gates]
        if any(not math.isfinite(g) or g < 0 for g in gates) or any(g >= MAX_GATE2 for g in self._gate2_host):
            raise ValueError(f"gates must be finite, not negative and below {math.sqrt(MAX_GATE2):.0f} m, got {gates}")
        self.q_pos, self.q_vel = _nonneg(q_pos, "q_pos"), _nonneg(q_vel, "q_vel")
        self.r_pos, self.r_vel = _positive(r_pos, "r_pos"), _positive(r_vel, "r_vel")
        self.p0_pos, self.p0_vel = _nonneg(p0_pos, "p0_pos"), _nonneg(p0_vel, "p0_vel")
        if math.isnan(float(score_thr)) or math.isnan(float(birth_thr)):
            raise ValueError("score_thr and birth_thr must not be NaN")
        if int(max_age) < 0 or int(min_hits) < 1:
            raise ValueError("max_age must not be negative and min_hits at least 1")
        self.score_thr, self.birth_thr = float(score_thr), float(birth_thr)
        self.max_age, self.min_hits, self.use_velocity = int(max_age), int(min_hits), bool(use_velocity)
        self.max_tracks, self.max_dets, self.history = T, D, H
        self.device = dev = torch.device(device)
        if dev.type != "cuda":
            raise ValueError("the tracker lives on a HIP device (no CPU fallback)")
        lib()
        self.state = new_state(T, H, dev)
        self.device = dev = self.state["trk_f"].device   # with its index: what the frames' tensors report
        self.gate2 = torch.tensor(self._gate2_host, dtype=torch.float32, device=dev)
        i32 = dict(dtype=torch.int32, device=dev)
        self.work = dict(det_w=torch.zeros((D, 9), dtype=torch.float32, device=dev), det_ok=torch.zeros(D, **i32),
                         live=torch.zeros(T, **i32), cost=torch.zeros((T, D), dtype=torch.float32, device=dev),
                         lsap_desc=torch.zeros((1, 4), dtype=torch.int64, device=dev))
        self.match_g, self.match_q = torch.full((T,), -1, **i32), torch.full((D,), -1, **i32)
        self.status = torch.zeros(1, **i32)
        self.det_track, self.det_slot = torch.full((D,), -1, **i32), torch.full((D,), -1, **i32)
        self._ws_bytes = int(lib().cmt_lsap_workspace_bytes(1, T, D))
        self._ws = torch.empty(max(self._ws_bytes, 4) // 4, dtype=torch.float32, device=dev)
        a = self._lsap = N.LsapArgs()
        a.P, a.max_nq, a.max_ngt = 1, T, D
        a.cost, a.cost_elems, a.desc = self.work["cost"].data_ptr(), T * D, self.work["lsap_desc"].data_ptr()
        a.match_q, a.ld_q, a.match_g, a.ld_g = self.match_q.data_ptr(), D, self.match_g.data_ptr(), T
        a.status, a.workspace, a.workspace_bytes = self.status.data_ptr(), self._ws.data_ptr(), self._ws_bytes
        # the two calls' argument structs, built once: every buffer but the frame's four is the tracker's own, so a
        # step only checks and sets those (the thin wrappers above check everything on every call)
        st, wk = self.state, self.work
        pa = self._predict = N.TrackPredictArgs()
        pa.T, pa.D, pa.ncls = T, D, ncls
        pa.q_pos, pa.q_vel, pa.score_thr = self.q_pos, self.q_vel, self.score_thr
        pa.trk_f, pa.trk_i, pa.gate2 = _p(st["trk_f"]), _p(st["trk_i"]), _p(self.gate2)
        pa.det_w, pa.det_ok, pa.live, pa.cost, pa.lsap_desc = (_p(wk[k]) for k in ("det_w", "det_ok", "live", "cost", "lsap_desc"))
        ua = self._update = N.TrackUpdateArgs()
        ua.T, ua.D, ua.H, ua.use_velocity, ua.max_age = T, D, H, int(self.use_velocity), self.max_age
        ua.r_pos, ua.r_vel, ua.p0_pos, ua.p0_vel, ua.birth_thr = self.r_pos, self.r_vel, self.p0_pos, self.p0_vel, self.birth_thr
        ua.trk_f, ua.trk_i, ua.hist, ua.counters = (_p(st[k]) for k in ("trk_f", "trk_i", "hist", "counters"))
        ua.live, ua.lsap_desc, ua.cost, ua.det_w, ua.det_ok = (_p(wk[k]) for k in ("live", "lsap_desc", "cost", "det_w", "det_ok"))
        ua.match_g, ua.match_q, ua.det_track, ua.det_slot = _p(self.match_g), _p(self.match_q), _p(self.det_track), _p(self.det_slot)
        self._last_ts = None
        self.frames = 0

    def reset(self):
        """a fresh state in the same buffers (stream-ordered, no host read)"""
        for k in ("trk_f", "hist", "counters"):
            self.state[k].zero_()
        self.state["trk_i"].zero_()
        self.state["trk_i"][:, 0] = -1
        self._last_ts = None
        self.frames = 0

    def step(self, boxes, scores, labels, count=None, *, timestamp=None, dt=None, pose=None):
        """One frame -> ``det_track`` int32 [max_dets] on the device: the track id of every detection row, -1 for a
        row that belongs to no track (below ``score_thr``, or unmatched and below ``birth_thr``, or beyond
        ``count``).  The tensor is the tracker's own buffer: the next step overwrites it.

        ``boxes`` fp32 [max_dets, >= 9], ``scores`` fp32 [max_dets], ``labels`` int32 [max_dets] and ``count`` (None
        or a device int32 of one element: the valid rows) as ``cmt_box_decode`` writes them for one sample.  ``dt``
        (seconds) or ``timestamp`` (seconds; dt is the difference to the previous step's) says how far the tracks
        move; the first step uses 0, and so does a step with neither.  A negative dt raises.  ``pose``: a 4 x 4
        rigid transform of the boxes into the frame the tracks live in (say sensor -> world).
        No host read and no synchronisation: predict, cmt_lsap and update are launched on the current stream."""
        if dt is None:
            dt = 0.0 if (timestamp is None or self._last_ts is None) else float(timestamp) - self._last_ts
        dt = float(dt)
        if not math.isfinite(dt) or dt < 0:
            raise ValueError(f"dt must be finite and not negative, got {dt} (timestamps must not run backwards)")
        if self.frames == 0:
            dt = 0.0   # nothing to move yet
        D, dev = self.max_dets, self.device
        n, ld = strided_rows(boxes, "boxes", 9, rows="max_dets")
        if n != D:
            raise ValueError(f"boxes must have max_dets = {D} rows, got {boxes.shape[0]}")
        scores = _t(scores, "scores", torch.float32, (D,))
        labels = _t(labels, "labels", torch.int32, (D,))
        count_word(count)
        _same_device(dev, boxes=boxes, scores=scores, labels=labels, count=count)
        pa, ua, L, stream = self._predict, self._update, lib(), _stream()
        pa.has_pose = 0
        if pose is not None:
            m, pa.pose_yaw = pose_arguments(pose)
            pa.has_pose = 1
            for k in range(12):
                pa.pose[k] = m[k]
        pa.dt, pa.ld = dt, ld
        pa.det, pa.scores, pa.labels, pa.count = _p(boxes), _p(scores), _p(labels), _p(count)
        ua.scores, ua.labels = pa.scores, pa.labels
        _check(L.cmt_track_predict(ctypes.byref(pa), stream), "cmt_track_predict")
        _check(L.cmt_lsap(ctypes.byref(self._lsap), stream), "cmt_lsap")
        _check(L.cmt_track_update(ctypes.byref(ua), stream), "cmt_track_update")
        if timestamp is not None:
            self._last_ts = float(timestamp)
        self.frames += 1
        return self.det_track

    def tracks(self, confirmed=True):
        """The live tracks -> dict(ids int32 [n], labels int32 [n], boxes fp32 [n, 9] (x y z dx dy dz yaw vx vy),
        scores fp32 [n], hits, misses, age int32 [n], slots int32 [n], history: a list of n arrays [m, 3], the last
        m = min(hist_n, history) positions of the track, oldest first), in ascending slot order.  ``confirmed``:
        only tracks with hits >= min_hits.  This is the one host read of the tracker (one copy of the state)."""
        flat = torch.cat([self.state["trk_f"].reshape(-1).view(torch.int32), self.state["trk_i"].reshape(-1),
                          self.state["hist"].reshape(-1).view(torch.int32)]).cpu().numpy()
        T, H = self.max_tracks, self.history
        tf = flat[:T * 16].view(np.float32).reshape(T, 16)
        ti = flat[T * 16:T * 24].reshape(T, 8)
        hist = flat[T * 24:].view(np.float32).reshape(T, H, 3)
        keep = ti[:, 0] >= 0
        if confirmed:
            keep &= ti[:, 2] >= self.min_hits
        slots = np.nonzero(keep)[0].astype(np.int32)
        history = []
        for s in slots:
            n = int(ti[s, 6])
            history.append(hist[s, :n].copy() if n <= H else np.roll(hist[s], -(n % H), axis=0).copy())
        return dict(ids=ti[slots, 0].copy(), labels=ti[slots, 1].copy(), boxes=tf[slots, :9].copy(),
                    scores=tf[slots, 9].copy(), hits=ti[slots, 2].copy(), misses=ti[slots, 3].copy(),
                    age=ti[slots, 4].copy(), slots=slots, history=history)


def tracker_from_config(cfg, device, **overrides):
    """A ``Tracker`` over the class names of a head config (``cfg['tasks']``, all tasks in order: the label space of
    the decoded boxes) or of a whole model config (``cfg['pts_bbox_head']`` / ``cfg['model']``)."""
    for key in ("model", "pts_bbox_head"):
        if isinstance(cfg, dict) and key in cfg and "tasks" not in cfg:
            cfg = cfg[key]
    if not isinstance(cfg, dict) or "tasks" not in cfg:
        raise ValueError("the config has no 'tasks' (a head config, or a model config with pts_bbox_head)")
    names = [n for t in cfg["tasks"] for n in t["class_names"]]
    return Tracker(names, device, **overrides)
