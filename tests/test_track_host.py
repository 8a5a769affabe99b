"""Host side of the tracker (native_track.py): the ABI of cmt_track_predict / cmt_track_update and their argument
errors (every one before any device work, with null or made-up pointers), the wrappers' ValueErrors, the numpy
restatement of tests/_track_ref.py against cases worked out by hand, the OpenLABEL keyword arguments, and the
id-purity property on the float64 reference.  No test here needs a device.
"""
import ctypes

import numpy as np
import pytest
import torch

import _track_ref as R

EINVAL, ENOTSUP = 1001, 1002
F = np.float32
KW = dict(use_velocity=False, r_pos=0.1, r_vel=1.0, p0_pos=1.0, p0_vel=10.0, birth_thr=0.3, max_age=3)


def _lib():
    from projects.mmdet3d_plugin import native
    if not native.available():
        pytest.skip("libcmt_hip.so not built")
    return native, native.lib()


# ---- ABI ---------------------------------------------------------------------------------------------------------
def test_track_abi():
    native, L = _lib()
    from projects.mmdet3d_plugin import native_track as NT
    assert L.cmt_abi_version() == 25
    for key, cls in (("track_predict", native.TrackPredictArgs), ("track_update", native.TrackUpdateArgs)):
        assert native.STRUCTS[key] is cls
        assert getattr(L, f"cmt_{key}_args_size")() == ctypes.sizeof(cls), key
        assert hasattr(L, f"cmt_{key}")
    assert ctypes.sizeof(native.TrackPredictArgs) == 6 * 4 + 4 * 4 + 14 * 4 + 12 * 8
    assert ctypes.sizeof(native.TrackUpdateArgs) == 6 * 4 + 6 * 4 + 15 * 8
    assert (NT.MAX_TRACKS, NT.MAX_DETS, NT.MAX_HISTORY, NT.MAX_CLASSES, NT.BIG) == (512, 1024, 32, 32, 1.0e6)


def test_null_structs_are_rejected():
    _, L = _lib()
    for name in ("cmt_track_predict", "cmt_track_update"):
        assert getattr(L, name)(None, None) == EINVAL
        assert name in L.cmt_last_error().decode()


def _predict_args(native, **kw):
    a = native.TrackPredictArgs()
    a.T, a.D, a.ld, a.ncls = 4, 4, 9, 3
    a.dt, a.q_pos, a.q_vel, a.score_thr = 0.1, 0.5, 1.0, 0.1
    for k, v in kw.items():
        if k == "pose":
            for i, x in enumerate(v):
                a.pose[i] = x
        else:
            setattr(a, k, v)
    return a


GOOD_PTRS = dict(trk_f=0x1000, trk_i=0x1000, det=0x1000, scores=0x1000, labels=0x1000, gate2=0x1000, det_w=0x1000,
                 det_ok=0x1000, live=0x1000, cost=0x1000)   # never dereferenced: a later check fails first


@pytest.mark.parametrize("kw,code,text", [
    (dict(T=0), EINVAL, "T and D"), (dict(D=0), EINVAL, "T and D"), (dict(T=-3), EINVAL, "T and D"),
    (dict(ncls=0), EINVAL, "ncls must"), (dict(ncls=-1), EINVAL, "ncls must"),
    (dict(T=513), ENOTSUP, "T above 512"), (dict(D=1025), ENOTSUP, "D above 1024"), (dict(ncls=33), ENOTSUP, "ncls above 32"),
    (dict(ld=8), EINVAL, "ld must"),
    (dict(dt=-0.1), EINVAL, "dt must"), (dict(dt=float("nan")), EINVAL, "dt must"), (dict(dt=float("inf")), EINVAL, "dt must"),
    (dict(q_pos=-1.0), EINVAL, "q_pos and q_vel"), (dict(q_vel=float("nan")), EINVAL, "q_pos and q_vel"),
    (dict(score_thr=float("nan")), EINVAL, "score_thr"),
    (dict(has_pose=1, pose=[float("nan")] + [0.0] * 11), EINVAL, "pose and pose_yaw"),
    (dict(has_pose=1, pose_yaw=float("inf")), EINVAL, "pose and pose_yaw"),
    (dict(), EINVAL, "the state"), (dict(trk_f=0x1000), EINVAL, "the state"), (dict(trk_f=0x1002, trk_i=0x1000), EINVAL, "the state"),
    (dict(trk_f=0x1000, trk_i=0x1000), EINVAL, "det, scores, labels and gate2"),
    (dict(GOOD_PTRS, gate2=0x1001), EINVAL, "det, scores, labels and gate2"),
    (dict(GOOD_PTRS, count=0x1002), EINVAL, "count must"),
    (dict(GOOD_PTRS), EINVAL, "lsap_desc"),                                   # null descriptor
    (dict(GOOD_PTRS, lsap_desc=0x1004), EINVAL, "lsap_desc"),                 # 4-byte aligned is not enough
    (dict(GOOD_PTRS, lsap_desc=0x1008, cost=0), EINVAL, "det_w, det_ok, live, cost"),
])
def test_predict_argument_errors(kw, code, text):
    """the pointers are null or made-up numbers: every case must return before any device work"""
    native, L = _lib()
    assert L.cmt_track_predict(ctypes.byref(_predict_args(native, **kw)), None) == code
    msg = L.cmt_last_error().decode()
    assert "cmt_track_predict" in msg and text in msg, msg


@pytest.mark.parametrize("kw,code,text", [
    (dict(T=0), EINVAL, "T and D"), (dict(D=-1), EINVAL, "T and D"),
    (dict(H=0), EINVAL, "H must"), (dict(H=-2), EINVAL, "H must"),
    (dict(T=513), ENOTSUP, "T above 512"), (dict(D=1025), ENOTSUP, "D above 1024"), (dict(H=33), ENOTSUP, "H above 32"),
    (dict(max_age=-1), EINVAL, "max_age"),
    (dict(r_pos=0.0), EINVAL, "r_pos and r_vel"), (dict(r_vel=-1.0), EINVAL, "r_pos and r_vel"),
    (dict(r_pos=float("nan")), EINVAL, "r_pos and r_vel"),
    (dict(p0_pos=-1.0), EINVAL, "p0_pos and p0_vel"), (dict(p0_vel=float("inf")), EINVAL, "p0_pos and p0_vel"),
    (dict(birth_thr=float("nan")), EINVAL, "birth_thr"),
    (dict(), EINVAL, "the state"), (dict(trk_f=0x1000, trk_i=0x1000, hist=0x1000), EINVAL, "the state"),
    (dict(trk_f=0x1000, trk_i=0x1000, hist=0x1000, counters=0x1001), EINVAL, "the state"),
    (dict(trk_f=0x1000, trk_i=0x1000, hist=0x1000, counters=0x1000), EINVAL, "live, cost, match_g, match_q"),
    (dict(trk_f=0x1000, trk_i=0x1000, hist=0x1000, counters=0x1000, live=0x1000, lsap_desc=0x1004, cost=0x1000,
          match_g=0x1000, match_q=0x1000), EINVAL, "live, cost, match_g, match_q"),
    (dict(trk_f=0x1000, trk_i=0x1000, hist=0x1000, counters=0x1000, live=0x1000, lsap_desc=0x1008, cost=0x1000,
          match_g=0x1000, match_q=0x1000), EINVAL, "det_w, scores, labels and det_ok"),
    (dict(trk_f=0x1000, trk_i=0x1000, hist=0x1000, counters=0x1000, live=0x1000, lsap_desc=0x1008, cost=0x1000,
          match_g=0x1000, match_q=0x1000, det_w=0x1000, scores=0x1000, labels=0x1000, det_ok=0x1000, det_track=0x1000),
     EINVAL, "det_track and det_slot"),
])
def test_update_argument_errors(kw, code, text):
    native, L = _lib()
    a = native.TrackUpdateArgs()
    a.T, a.D, a.H, a.max_age = 4, 4, 2, 3
    a.r_pos, a.r_vel, a.p0_pos, a.p0_vel, a.birth_thr = 0.1, 1.0, 1.0, 10.0, 0.3
    for k, v in kw.items():
        setattr(a, k, v)
    assert L.cmt_track_update(ctypes.byref(a), None) == code
    msg = L.cmt_last_error().decode()
    assert "cmt_track_update" in msg and text in msg, msg


def _cpu_state(T=4, H=2):
    ti = torch.zeros((T, 8), dtype=torch.int32)
    ti[:, 0] = -1
    return dict(trk_f=torch.zeros((T, 16)), trk_i=ti, hist=torch.zeros((T, H, 3)), counters=torch.zeros(4, dtype=torch.int32))


def _cpu_work(T=4, D=5):
    return dict(det_w=torch.zeros((D, 9)), det_ok=torch.zeros(D, dtype=torch.int32), live=torch.zeros(T, dtype=torch.int32),
                cost=torch.zeros((T, D)), lsap_desc=torch.zeros((1, 4), dtype=torch.int64))


def test_wrapper_argument_errors():
    """every ValueError comes before the device check: CPU tensors are enough to see them"""
    from projects.mmdet3d_plugin import native_track as NT
    st, wk = _cpu_state(), _cpu_work()
    det, sc, lab, g = torch.zeros((5, 9)), torch.zeros(5), torch.zeros(5, dtype=torch.int32), torch.full((3,), 4.0)
    kw = dict(dt=0.1, q_pos=0.5, q_vel=1.0, score_thr=0.1, gate2_host=[4.0] * 3)
    bad = [
        (dict(det=torch.zeros((5, 8))), "det must"), (dict(det=torch.zeros((5, 9), dtype=torch.float64)), "det must"),
        (dict(det=torch.zeros((1025, 9))), "detection rows"), (dict(sc=torch.zeros(4)), "scores must"),
        (dict(lab=torch.zeros(5, dtype=torch.int64)), "labels must"), (dict(g=torch.zeros(33)), "classes must"),
        (dict(count=torch.zeros(2, dtype=torch.int32)), "count must"), (dict(count=torch.zeros(1)), "count must"),
        (dict(kw=dict(kw, dt=-0.1)), "dt must"), (dict(kw=dict(kw, q_pos=float("nan"))), "q_pos must"),
        (dict(kw=dict(kw, score_thr=float("nan"))), "score_thr"),
        (dict(kw=dict(kw, gate2_host=[4.0, 1.0e5, 4.0])), "gate2 needs"), (dict(kw=dict(kw, gate2_host=[4.0, 4.0])), "gate2 needs"),
        (dict(kw=dict(kw, gate2_host=None), g=torch.tensor([4.0, float("nan"), 1.0])), "gate2 needs"),
        (dict(kw=dict(kw, pose=np.eye(3))), "pose must"),
        (dict(st=dict(st, trk_f=torch.zeros((4, 15)))), "trk_f must"), (dict(st=dict(st, trk_i=torch.zeros((5, 8), dtype=torch.int32))), "trk_i must"),
        (dict(st=dict(trk_f=st["trk_f"])), "state must"),
        (dict(wk=dict(wk, cost=torch.zeros((4, 6)))), "cost must"), (dict(wk=dict(wk, lsap_desc=torch.zeros((1, 4), dtype=torch.int32))), "lsap_desc must"),
        (dict(), "HIP device"),                                                  # all good: the device check is last
    ]
    for ch, text in bad:
        a = dict(st=st, det=det, sc=sc, lab=lab, count=None, g=g, wk=wk, kw=kw)
        a.update(ch)
        with pytest.raises(ValueError, match=text):
            NT.track_predict(a["st"], a["det"], a["sc"], a["lab"], a["count"], a["g"], a["wk"], **a["kw"])
    mg, mq = torch.zeros(4, dtype=torch.int32), torch.zeros(5, dtype=torch.int32)
    dt_, ds_ = torch.zeros(5, dtype=torch.int32), torch.zeros(5, dtype=torch.int32)
    bad = [
        (dict(mg=torch.zeros(5, dtype=torch.int32)), "match_g must"), (dict(mq=torch.zeros(5)), "match_q must"),
        (dict(dt_=torch.zeros(4, dtype=torch.int32)), "det_track must"),
        (dict(st=dict(st, hist=torch.zeros((4, 33, 3)))), "history must"), (dict(st=dict(st, hist=torch.zeros((4, 2, 4)))), "hist must"),
        (dict(kw=dict(KW, max_age=-1)), "max_age"), (dict(kw=dict(KW, r_pos=0.0)), "r_pos must"),
        (dict(kw=dict(KW, p0_vel=-1.0)), "p0_vel must"), (dict(kw=dict(KW, birth_thr=float("nan"))), "birth_thr"),
        (dict(), "HIP device"),
    ]
    for ch, text in bad:
        a = dict(st=st, wk=wk, mg=mg, mq=mq, sc=sc, lab=lab, dt_=dt_, ds_=ds_, kw=KW)
        a.update(ch)
        with pytest.raises(ValueError, match=text):
            NT.track_update(a["st"], a["wk"], a["mg"], a["mq"], a["sc"], a["lab"], a["dt_"], a["ds_"], **a["kw"])
    for kw2, text in ((dict(max_tracks=513), "track slots"), (dict(max_dets=0), "detection rows"), (dict(history=33), "history must"),
                      (dict(gate={"tram": 1.0}), "unknown classes"), (dict(gate=400.0), "gates must"), (dict(gate=-1.0), "gates must"),
                      (dict(min_hits=0), "min_hits"), (dict(r_vel=0.0), "r_vel must"), (dict(), "HIP device")):
        with pytest.raises(ValueError, match=text):
            NT.Tracker(["car", "bus"], "cpu", **kw2)
    with pytest.raises(ValueError, match="classes must"):
        NT.Tracker([], "cpu")
    with pytest.raises(ValueError, match="no 'tasks'"):
        NT.tracker_from_config(dict(type="x"), "cpu")
    m, yaw = NT.pose_arguments(np.array([[0.0, -1.0, 0, 5], [1.0, 0.0, 0, 6], [0, 0, 1.0, 7], [0, 0, 0, 1]]))
    assert m == [0.0, -1.0, 0.0, 5.0, 1.0, 0.0, 0.0, 6.0, 0.0, 0.0, 1.0, 7.0] and yaw == float(F(np.pi / 2))


# ---- the restatement against hand-worked cases ----------------------------------------------------------------------
def _state(T, H, tracks):
    """tracks: (slot, id, label, x, y) with P = (1, 0, 10) per axis"""
    st = R.fresh_state(T, H)
    for s, i, lab, x, y in tracks:
        st["trk_f"][s, [0, 1]] = (x, y)
        st["trk_f"][s, 10:16] = (1, 0, 10, 1, 0, 10)
        st["trk_i"][s] = (i, lab, 1, 0, 0, -1, 1, 0)
        st["hist"][s, 0] = (x, y, 0)
        st["counters"][:2] = (st["counters"][0] + 1, max(st["counters"][1], i + 1))
    return st


def _dets(rows):
    """rows: (x, y, score, label)"""
    det = np.zeros((len(rows), 9), F)
    det[:, 3:6] = (4.0, 2.0, 1.5)
    for j, (x, y, _, _) in enumerate(rows):
        det[j, :2] = (x, y)
    return det, np.array([r[2] for r in rows], F), np.array([r[3] for r in rows], np.int32)


def _frame(st, rows, count=None, gate2=(4.0, 4.0), dt=0.0, **kw):
    det, sc, lab = _dets(rows)
    pc = R.predict_cost(st, det, sc, lab, count, dt, 0.5, 1.0, 0.1, gate2)
    mg, mq, total = R.assign(pc["cost"], pc["n_live"], pc["n_det"])
    trk, slot = R.update(st, pc["live"], pc["n_live"], pc["n_det"], pc["cost"], mg, mq, pc["det_w"], sc, lab, pc["det_ok"],
                         **dict(KW, **kw))
    return pc, mg, mq, trk, slot


def test_optimum_is_not_the_nearest_per_row():
    st = _state(4, 2, [(0, 7, 0, 0.0, 0.0), (2, 9, 0, 1.0, 0.0)])
    pc, mg, mq, trk, slot = _frame(st, [(0.9, 0.0, 0.9, 0), (-1.5, 0.0, 0.9, 0)])
    c = pc["cost"]
    assert pc["live"].tolist() == [0, 2] and pc["desc"].tolist() == [0, 2, 2, 2]
    assert c[0, 0] == F(0.9) * F(0.9) and c[0, 1] == F(2.25) and c[1, 1] == R.BIG    # row 1, box 1: 6.25 is beyond the gate
    assert c[1, 0] == (F(1.0) - F(0.9)) * (F(1.0) - F(0.9))
    assert np.argmin(c[:2, :2], 1).tolist() == [0, 0]                                # both rows prefer box 0
    assert mg.tolist() == [1, 0] and mq.tolist() == [1, 0]                           # the optimum gives it to row 1
    assert trk.tolist() == [9, 7] and slot.tolist() == [2, 0]
    assert st["trk_i"][0].tolist() == [7, 0, 2, 0, 1, 1, 2, 0] and st["trk_i"][2].tolist() == [9, 0, 2, 0, 1, 0, 2, 0]
    # position-only filter by hand: K0 = 1 / 1.1, x = 0 + K0 * (-1.5)
    K0 = F(1) / (F(1) + F(0.1))
    assert st["trk_f"][0, 0] == F(0) + K0 * (F(-1.5) - F(0)) and st["trk_f"][0, 10] == F(1) - K0 * F(1)
    assert st["counters"].tolist() == [2, 10, 0, 1]


def test_class_mismatch_gate_edge_and_score_edge():
    st = _state(4, 2, [(1, 0, 0, 0.0, 0.0)])
    rows = [(0.5, 0.0, 0.9, 1),                 # inside the gate, another class
            (2.0, 0.0, 0.9, 0),                 # d2 == gate2 exactly: not matched (strict)
            (0.0, 1.5, F(0.1), 0),              # score == score_thr: kept, matches
            (0.1, 0.0, 0.05, 0)]                # below score_thr: nearest, but ignored
    pc, mg, mq, trk, slot = _frame(st, rows)
    assert pc["det_ok"].tolist() == [1, 1, 1, 0]
    assert pc["cost"][0].tolist() == [R.BIG, R.BIG, F(2.25), R.BIG]
    assert mg.tolist() == [2] and trk.tolist() == [1, 2, 0, -1] and slot.tolist() == [0, 2, 1, -1]   # births: ids 1, 2
    assert st["trk_i"][0, 1] == 1 and st["trk_i"][2, 1] == 0 and st["counters"].tolist() == [3, 3, 0, 1]


def test_birth_order_ids_and_state():
    st = R.fresh_state(4, 2)
    pc, mg, mq, trk, slot = _frame(st, [(0, 0, 0.5, 0), (5, 5, 0.2, 1), (9, 9, 0.9, 1), (20, 20, 0.9, 0)], count=3,
                                   use_velocity=True)
    assert pc["n_live"] == 0 and pc["det_ok"].tolist() == [1, 1, 1, 0]            # the row beyond count is no detection
    assert trk.tolist() == [0, -1, 1, -1] and slot.tolist() == [0, -1, 1, -1]     # 0.2 is below birth_thr
    assert st["trk_i"][:2].tolist() == [[0, 0, 1, 0, 0, 0, 1, 0], [1, 1, 1, 0, 0, 2, 1, 0]] and (st["trk_i"][2:, 0] == -1).all()
    assert st["trk_f"][1].tolist() == [9, 9, 0, 4, 2, 1.5, 0, 0, 0, F(0.9), 1, 0, 10, 1, 0, 10]
    assert st["hist"][1].tolist() == [[9, 9, 0], [0, 0, 0]] and st["counters"].tolist() == [2, 2, 0, 1]


def test_slot_freed_and_reused_in_one_call():
    st = _state(2, 2, [(0, 4, 0, 0.0, 0.0), (1, 5, 0, 50.0, 0.0)])
    st["trk_i"][0, 3] = 3                                                         # misses == max_age: one more ends it
    pc, mg, mq, trk, slot = _frame(st, [(50.2, 0.0, 0.9, 0), (80.0, 0.0, 0.9, 0)])
    assert trk.tolist() == [5, 6] and slot.tolist() == [1, 0]                     # the new track takes the slot freed now
    assert st["trk_i"][0].tolist() == [6, 0, 1, 0, 0, 1, 1, 0] and st["counters"].tolist() == [2, 7, 0, 1]
    st = _state(2, 2, [(0, 4, 0, 0.0, 0.0)])
    _frame(st, [(90.0, 0.0, 0.2, 0)], max_age=0)                                  # max_age 0: the first miss ends it
    assert st["trk_i"][0, 0] == -1 and st["trk_i"][0, 3] == 1 and st["counters"].tolist() == [0, 5, 0, 1]


def test_births_beyond_the_free_slots_are_dropped():
    st = R.fresh_state(1, 2)
    pc, mg, mq, trk, slot = _frame(st, [(0, 0, 0.9, 0), (10, 0, 0.9, 0), (20, 0, 0.9, 0)])
    assert trk.tolist() == [0, -1, -1] and slot.tolist() == [0, -1, -1] and st["counters"].tolist() == [1, 1, 2, 1]
    pc, mg, mq, trk, slot = _frame(st, [(0.1, 0, 0.9, 0), (10, 0, 0.9, 0)])
    assert trk.tolist() == [0, -1] and st["counters"].tolist() == [1, 1, 3, 2]    # a dropped birth uses no id


def test_ring_wraps():
    st = R.fresh_state(2, 2)
    xs = [0.0, 0.3, 0.5, 0.9]
    for x in xs:
        _frame(st, [(x, 0.0, 0.9, 0)], dt=0.1)
    assert st["trk_i"][0, 6] == 4 and st["trk_i"][0, 2] == 4 and st["trk_i"][0, 4] == 3
    h = R.history(st, 0)
    assert h.shape == (2, 3) and h[1, 0] == st["trk_f"][0, 0] and h[0, 0] < h[1, 0]   # oldest first, the newest is the state
    assert (st["hist"][0, 1] == h[1]).all() and (st["hist"][0, 0] == h[0]).all()      # entry 3 went to 3 % 2


def test_inconsistent_match_tables_move_nothing():
    base = _state(4, 2, [(0, 0, 0, 0.0, 0.0), (3, 1, 0, 10.0, 0.0)])
    det, sc, lab = _dets([(0.1, 0.0, 0.2, 0), (10.1, 0.0, 0.2, 0)])                   # below birth_thr: no births either
    pc = R.predict_cost(base, det, sc, lab, None, 0.0, 0.5, 1.0, 0.1, (4.0, 4.0))
    for mg, mq, want in (([0, 1], [0, 1], [0, 1]), ([0, 1], [1, 0], [-1, -1]), ([0, 0], [1, 1], [-1, -1]),
                         ([5, -7], [0, 1], [-1, -1]), ([1, 0], [1, 0], [-1, -1]), ([0, 1], [0, 9], [0, -1])):
        st = R.copy_state(base)
        trk, _ = R.update(st, pc["live"], 2, 2, pc["cost"], np.array(mg, np.int32), np.array(mq, np.int32), pc["det_w"], sc,
                          lab, pc["det_ok"], **KW)
        assert trk.tolist() == want, (mg, mq)                                        # [1, 0]: both pairs are beyond the gate
    st = R.copy_state(base)
    trk, _ = R.update(st, np.array([3, 0], np.int32), 2, 2, pc["cost"], np.array([0, 1], np.int32), np.array([0, 1], np.int32),
                      pc["det_w"], sc, lab, pc["det_ok"], **KW)
    assert trk.tolist() == [-1, -1] and st["trk_i"][[0, 3], 3].tolist() == [1, 1]    # a live table that is not the live list


def test_pose_and_yaw_wrap():
    st = R.fresh_state(2, 2)
    det, sc, lab = _dets([(1.0, 2.0, 0.9, 0), (3.0, 4.0, 0.9, 0)])
    det[:, 6], det[:, 7], det[:, 8] = (3.0, -3.0), 1.0, 0.0
    pose = np.array([[0.0, -1.0, 0, 5], [1.0, 0.0, 0, 6], [0, 0, 1.0, 7], [0, 0, 0, 1]])
    pc = R.predict_cost(st, det, sc, lab, None, 0.0, 0.5, 1.0, 0.1, (4.0,), pose=pose[:3], pose_yaw_f=R.pose_yaw(pose))
    assert pc["det_w"][0, :3].tolist() == [3.0, 7.0, 7.0] and pc["det_w"][:, 7:].tolist() == [[0, 1], [0, 1]]
    assert pc["det_w"][0, 6] == (F(3.0) + F(np.pi / 2)) - F(6.2831855) and pc["det_w"][1, 6] == F(-3.0) + F(np.pi / 2)
    assert (pc["det_w"][:, 3:6] == det[:, 3:6]).all()


# ---- OpenLABEL -------------------------------------------------------------------------------------------------------
def test_boxes_to_detections_track_ids():
    from projects.mmdet3d_plugin.core import openlabel as OL
    boxes = np.array([[1, 2, 0, 4, 2, 1.5, 0.3, 0, 0], [5, 6, 0, 4, 2, 1.5, -0.2, 0, 0], [9, 9, 0, 1, 1, 1, 0, 0, 0]], F)
    sc, lab = np.array([0.9, 0.4, 0.7], F), np.array([0, 1, 0])

    def counter():
        n = [0]

        def fn():
            n[0] += 1
            return f"u{n[0]:03d}-x"
        return fn
    plain = OL.boxes_to_detections(boxes, sc, lab, ["car", "bus"], uuid_fn=counter())
    assert [d.uuid for d in plain] == ["u001-x", "u002-x", "u003-x"] and [d.pos_history for d in plain] == [[], [], []]
    same = OL.boxes_to_detections(boxes, sc, lab, ["car", "bus"], uuid_fn=counter(), track_ids=None, histories=None)
    doc = lambda ds: OL.detections_to_openlabel(ds, frame_id=3)   # noqa: E731
    assert doc(plain) == doc(same)
    OL.reset_track_uuids()
    fn = counter()
    f0 = OL.boxes_to_detections(boxes, sc, lab, ["car", "bus"], uuid_fn=fn, track_ids=[4, -1, 7],
                                histories={4: [[0, 0, 0], [1, 2, 0]]})
    f1 = OL.boxes_to_detections(boxes[::-1], sc[::-1], lab[::-1], ["car", "bus"], uuid_fn=fn, track_ids=np.array([7, 9, 4]))
    assert f0[0].uuid == f1[2].uuid and f0[2].uuid == f1[0].uuid and f0[0].id == 4 and f1[0].id == 7
    assert len({f0[0].uuid, f0[1].uuid, f0[2].uuid, f1[1].uuid}) == 4
    assert [q.tolist() for q in f0[0].pos_history] == [[0, 0, 0], [1, 2, 0]] and f0[2].pos_history == []
    vec = doc(f0)["openlabel"]["frames"]["3"]["objects"][f0[0].uuid]["object_data"]["cuboid"]["attributes"]["vec"]
    assert vec == [{"name": "track_history", "val": [0, 0, 0, 1, 2, 0]}]
    kept = OL.boxes_to_detections(boxes, sc, lab, ["car", "bus"], bbox_score=0.5, track_ids=[4, 5, 7],
                                  uuid_for_track=lambda k: f"t{k}")
    assert [d.uuid for d in kept] == ["t4", "t7"]
    with pytest.raises(ValueError, match="track_ids has"):
        OL.boxes_to_detections(boxes, sc, lab, ["car", "bus"], track_ids=[1, 2])


# ---- the scene and the property ---------------------------------------------------------------------------------------
def test_moving_scene_is_what_it_says():
    from projects.mmdet3d_plugin import synthetic as S
    fr = S.moving_scene(3)
    again = S.moving_scene(3)
    assert len(fr) == 30 and all((a["boxes"] == b["boxes"]).all() for a, b in zip(fr, again))
    gone = np.zeros(12, int)
    for t, f in enumerate(fr):
        assert f["boxes"].dtype == F and f["labels"].dtype == np.int32 and f["timestamp"] == pytest.approx(0.1 * t)
        obj = f["object"]
        assert (obj < 0).sum() == 2 and len(set(obj[obj >= 0])) == (obj >= 0).sum()
        seen = np.isin(np.arange(12), obj)
        gone = np.where(seen, 0, gone + 1)
        assert gone.max() <= 2
        real, false = f["boxes"][obj >= 0], f["boxes"][obj < 0]
        truth = np.stack([(obj[obj >= 0] % 4) * 10.0, (obj[obj >= 0] // 4) * 10.0], 1)
        assert np.abs(real[:, :2] - truth).max() <= 0.2 + 1.0 * 0.1 * t + 1e-5       # noise plus at most 1 m/s
        assert np.hypot(*(false[:, None, :2] - real[None, :, :2]).T).min() >= 5.0 - 0.2 * np.sqrt(2) - 1e-5
    padded = S.moving_scene(3, pad_to=40)
    assert all(p["boxes"].shape == (40, 9) and p["count"] == f["count"] and (p["boxes"][:f["count"]] == f["boxes"]).all()
               for p, f in zip(padded, fr))


@pytest.mark.parametrize("use_velocity", [False, True])
@pytest.mark.parametrize("seed", range(8))
def test_id_purity_of_the_float64_reference(seed, use_velocity):
    from projects.mmdet3d_plugin import synthetic as S
    fr = S.moving_scene(seed)
    tracks, st = R.run_scene([(f["boxes"], f["scores"], f["labels"]) for f in fr], 3, use_velocity=use_velocity)
    ids = R.ids_per_object(fr, tracks)
    assert len(ids) == 12 and all(len(v) == 1 and min(v) >= 0 for v in ids.values()), ids
    assert len({min(v) for v in ids.values()}) == 12                                  # and no id serves two objects
    assert 12 <= st["counters"][1] <= 12 + 2 * 30 and st["counters"][2] == 0 and st["counters"][3] == 30
