"""Host side of the rotated-box calls (native_iou.py): the ABI of cmt_box_iou / cmt_box_nms / cmt_box_concat and
their argument errors (every one before any device work, with null or made-up pointers), the wrappers' ValueErrors,
the float64 restatement of tests/_iou_ref.py against answers worked out by hand, nms_from_test_cfg, IoU3DCost, and
the tolerance measurement: the float32 restatement against float64 over the device test's inputs.  No test here needs
a device.
"""
import ctypes
import json
import math
import os

import numpy as np
import pytest
import torch

import _iou_ref as R

EINVAL = 1001
F = np.float32
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def _lib():
    from projects.mmdet3d_plugin import native
    if not native.available():
        pytest.skip("libcmt_hip.so not built")
    return native, native.lib()


# ---- ABI -------------------------------------------------------------------------------------------------------------
def test_iou_abi():
    native, L = _lib()
    from projects.mmdet3d_plugin import native_iou as NI
    assert L.cmt_abi_version() == 25
    for key, cls in (("box_iou", native.BoxIouArgs), ("box_nms", native.BoxNmsArgs), ("box_concat", native.BoxConcatArgs)):
        assert native.STRUCTS[key] is cls
        assert getattr(L, f"cmt_{key}_args_size")() == ctypes.sizeof(cls), key
        assert hasattr(L, f"cmt_{key}")
    assert ctypes.sizeof(native.BoxIouArgs) == 6 * 4 + 2 * 4 + 8 + 6 * 8
    assert ctypes.sizeof(native.BoxNmsArgs) == 4 * 4 + 4 * 4 + 8 * 8 + 8
    assert ctypes.sizeof(native.BoxConcatArgs) == 4 * 4 + 3 * 8 * 4 + 8 * 12 * 4 + 4 * 8 * 8 + 5 * 8
    assert (NI.NMS_MAX, NI.CONCAT_MAX) == (2048, 8)


def test_nms_workspace_bytes():
    _, L = _lib()
    assert L.cmt_box_nms_workspace_bytes(0) == 16
    assert L.cmt_box_nms_workspace_bytes(1) == 16 + 4 * 64 + 64 * 8
    assert L.cmt_box_nms_workspace_bytes(65) == 16 + 4 * 128 + 128 * 2 * 8
    assert L.cmt_box_nms_workspace_bytes(2048) == 16 + 4 * 2048 + 2048 * 2048 // 8
    assert L.cmt_box_nms_workspace_bytes(2049) == -1 and L.cmt_box_nms_workspace_bytes(-1) == -1


def test_null_structs_are_rejected():
    _, L = _lib()
    for name in ("cmt_box_iou", "cmt_box_nms", "cmt_box_concat"):
        assert getattr(L, name)(None, None) == EINVAL
        assert name in L.cmt_last_error().decode()


P = 0x1000   # a made-up pointer: never dereferenced, a later check fails first or the call launches nothing


def _iou_args(native, **kw):
    a = native.BoxIouArgs()
    a.N, a.M, a.lda, a.ldb, a.ldo, a.z_origin = 4, 5, 7, 7, 5, 0.5
    for k, v in kw.items():
        setattr(a, k, v)
    return a


@pytest.mark.parametrize("kw,text", [
    (dict(N=-1), "N and M"), (dict(M=-2), "N and M"),
    (dict(lda=6), "lda and ldb"), (dict(ldb=0), "lda and ldb"),
    (dict(z_origin=0.25), "z_origin"), (dict(z_origin=float("nan")), "z_origin"),
    (dict(), "both be null"),
    (dict(bev=P, aligned=1), "aligned needs"),
    (dict(bev=P, ldo=4), "ldo must"),
    (dict(bev=P, N=1 << 30, M=1 << 30, ldo=1 << 30), "tiles"),
    (dict(bev=P + 2), "bev and iou3d must be 4-byte"), (dict(bev=P, iou3d=P + 1), "bev and iou3d must be 4-byte"),
    (dict(bev=P, n_a=P + 2), "n_a and n_b"), (dict(bev=P, n_b=P + 3), "n_a and n_b"),
    (dict(bev=P), "a and b"), (dict(bev=P, a=P), "a and b"), (dict(bev=P, a=P, b=P + 2), "a and b"),
])
def test_iou_argument_errors(kw, text):
    native, L = _lib()
    assert L.cmt_box_iou(ctypes.byref(_iou_args(native, **kw)), None) == EINVAL
    msg = L.cmt_last_error().decode()
    assert "cmt_box_iou" in msg and text in msg, msg


def test_iou_empty_sets_launch_nothing():
    native, L = _lib()
    assert L.cmt_box_iou(ctypes.byref(_iou_args(native, N=0, bev=P)), None) == 0
    assert L.cmt_box_iou(ctypes.byref(_iou_args(native, M=0, ldo=0, iou3d=P)), None) == 0


def _nms_args(native, **kw):
    a = native.BoxNmsArgs()
    a.N, a.ld, a.iou_thr, a.score_thr, a.z_origin = 8, 7, 0.2, 0.0, 0.5
    for k, v in kw.items():
        setattr(a, k, v)
    return a


NMS_PTRS = dict(boxes=P, scores=P, keep_idx=P, keep_count=P, workspace=P, workspace_bytes=1 << 20)


@pytest.mark.parametrize("kw,text", [
    (dict(N=2049), "N must be 0..2048"), (dict(N=-1), "N must be 0..2048"),
    (dict(ld=6), "ld must"),
    (dict(z_origin=1.0), "z_origin"),
    (dict(iou_thr=-0.1), "iou_thr"), (dict(iou_thr=float("nan")), "iou_thr"), (dict(iou_thr=float("inf")), "iou_thr"),
    (dict(score_thr=float("nan")), "score_thr"),
    (dict(keep_dtype=2), "keep_dtype"),
    (dict(), "boxes and scores"), (dict(boxes=P), "boxes and scores"), (dict(boxes=P, scores=P + 2), "boxes and scores"),
    (dict(boxes=P, scores=P, labels=P + 1), "labels and count"), (dict(boxes=P, scores=P, count=P + 2), "labels and count"),
    (dict(boxes=P, scores=P), "keep_idx"), (dict(boxes=P, scores=P, keep_idx=P + 2), "keep_idx"),
    (dict(boxes=P, scores=P, keep_idx=P, keep=P + 1, keep_dtype=1), "int32 keep"),
    (dict(boxes=P, scores=P, keep_idx=P), "keep_count"), (dict(boxes=P, scores=P, keep_idx=P, keep_count=P + 2), "keep_count"),
    (dict(boxes=P, scores=P, keep_idx=P, keep_count=P), "workspace must"),
    (dict(boxes=P, scores=P, keep_idx=P, keep_count=P, workspace=P + 4), "workspace must"),
    (dict(NMS_PTRS, workspace_bytes=16 + 4 * 64 + 64 * 8 - 1), "workspace_bytes"),
    (dict(NMS_PTRS, N=2048, workspace_bytes=2048 * 2048 // 8), "workspace_bytes"),
])
def test_nms_argument_errors(kw, text):
    native, L = _lib()
    assert L.cmt_box_nms(ctypes.byref(_nms_args(native, **kw)), None) == EINVAL
    msg = L.cmt_last_error().decode()
    assert "cmt_box_nms" in msg and text in msg, msg


def _concat_args(native, K=2, ptrs=True, **kw):
    a = native.BoxConcatArgs()
    a.K, a.cols, a.ld_out = K, 9, 9
    for k in range(min(max(K, 0), 8)):
        a.n[k], a.ld[k] = 3, 9
        if ptrs:
            a.boxes[k], a.scores[k], a.labels[k] = P, P, P
    for key, v in kw.items():
        if isinstance(v, tuple):        # (index, value) into an array member
            if key == "transform":
                a.has_transform[v[0]] = 1
                for t in range(12):
                    a.transform[v[0]][t] = v[1][t]
            else:
                getattr(a, key)[v[0]] = v[1]
        else:
            setattr(a, key, v)
    return a


IDENT = [1.0, 0, 0, 0, 0, 1.0, 0, 0, 0, 0, 1.0, 0]


@pytest.mark.parametrize("kw,text", [
    (dict(K=9), "K must be 1..8"), (dict(K=0), "K must be 1..8"),
    (dict(cols=6), "cols must"), (dict(cols=17), "cols must"),
    (dict(ld_out=8), "ld_out"),
    (dict(n=(1, -1)), "capacity must not be negative"),
    (dict(ld=(0, 8)), "source's ld"),
    (dict(ptrs=False), "boxes, scores and labels"), (dict(scores=(1, P + 2)), "boxes, scores and labels"),
    (dict(labels=(0, None)), "boxes, scores and labels"),
    (dict(count=(1, P + 1)), "source's count"),
    (dict(transform=(0, [float("nan")] + IDENT[1:])), "transform must be finite"),
    (dict(transform=(1, IDENT[:11] + [float("inf")])), "transform must be finite"),
    (dict(n=(0, 1 << 30)), "total capacity"),
    (dict(), "out_boxes, out_scores"), (dict(out_boxes=P, out_scores=P, out_labels=P, out_source=P + 2), "out_boxes, out_scores"),
    (dict(out_boxes=P, out_scores=P, out_labels=P, out_source=P), "out_count"),
    (dict(out_boxes=P, out_scores=P, out_labels=P, out_source=P, out_count=P + 1), "out_count"),
])
def test_concat_argument_errors(kw, text):
    native, L = _lib()
    assert L.cmt_box_concat(ctypes.byref(_concat_args(native, **kw)), None) == EINVAL
    msg = L.cmt_last_error().decode()
    assert "cmt_box_concat" in msg and text in msg, msg


# ---- the wrappers ----------------------------------------------------------------------------------------------------
def test_wrappers_refuse_bad_arguments_and_host_tensors():
    _lib()
    from projects.mmdet3d_plugin import native_iou as NI
    from projects.mmdet3d_plugin.core.post_processing import fuse_detections
    b = torch.zeros((4, 7))
    s, lab = torch.zeros(4), torch.zeros(4, dtype=torch.int32)
    with pytest.raises(ValueError, match="no CPU fallback"):
        NI.box_iou(b, b)
    with pytest.raises(ValueError, match="no CPU fallback"):
        NI.nms_rotated(b, s, 0.2)
    with pytest.raises(ValueError, match="no CPU fallback"):
        NI.concat_detections([(b, s, lab)])
    with pytest.raises(ValueError, match="no CPU fallback"):
        fuse_detections([(b, s, lab)], iou_thr=0.2)
    with pytest.raises(ValueError, match="mode must"):
        NI.box_iou(b, b, mode="giou")
    with pytest.raises(ValueError, match=">= 7"):
        NI.box_iou(torch.zeros((4, 6)), b)
    with pytest.raises(ValueError, match=">= 7"):
        NI.box_iou(b.double(), b)
    with pytest.raises(ValueError, match="z_origin"):
        NI.box_iou(b, b, z_origin=1.0)
    with pytest.raises(ValueError, match="aligned needs"):
        NI.box_iou(b, torch.zeros((5, 7)), aligned=True)
    with pytest.raises(ValueError, match="n_a must"):
        NI.box_iou(b, b, n_a=torch.zeros(1, dtype=torch.int64))
    with pytest.raises(ValueError, match="writes 2"):
        NI.box_iou(b, b, mode="both", out=torch.zeros((4, 4)))
    with pytest.raises(ValueError, match="out must"):
        NI.box_iou(b, b, out=torch.zeros((4, 3)))
    with pytest.raises(ValueError, match="at most 2048"):
        NI.nms_rotated(torch.zeros((2049, 7)), torch.zeros(2049), 0.2)
    with pytest.raises(ValueError, match="scores must"):
        NI.nms_rotated(b, torch.zeros(3), 0.2)
    with pytest.raises(ValueError, match="labels must"):
        NI.nms_rotated(b, s, 0.2, labels=lab.long())
    with pytest.raises(ValueError, match="iou_thr"):
        NI.nms_rotated(b, s, -1.0)
    with pytest.raises(ValueError, match="score_thr"):
        NI.nms_rotated(b, s, 0.2, score_thr=float("nan"))
    with pytest.raises(ValueError, match="1..8 sources"):
        NI.concat_detections([(b, s, lab)] * 9)
    with pytest.raises(ValueError, match="1..8 sources"):
        NI.concat_detections([])
    with pytest.raises(ValueError, match="poses has"):
        NI.concat_detections([(b, s, lab)], poses=[None, None])
    with pytest.raises(ValueError, match="must be \\(boxes"):
        NI.concat_detections([(b, s)])
    with pytest.raises(ValueError, match="0..2048"):
        NI.nms_workspace(4096, "cpu")


# ---- the float64 restatement against answers worked out by hand --------------------------------------------------------
def box(x=0.0, y=0.0, z=0.0, dx=4.0, dy=2.0, dz=1.5, yaw=0.0):
    return np.array([[x, y, z, dx, dy, dz, yaw]], np.float64)


def iou64(a, b, zo=0.5):
    e, t = R.iou_pairs(a, b, zo, np.float64)
    return float(e[0]), float(t[0])


@pytest.mark.parametrize("yaw", [0.0, 0.3, -2.9, 6.5])
def test_known_answers(yaw):
    c, s = math.cos(yaw), math.sin(yaw)
    a = box(12.0, -7.0, 0.5, 4.0, 2.0, 1.5, yaw)
    assert iou64(a, a) == pytest.approx((1.0, 1.0), abs=1e-12)
    # the same box turned by pi / 2: the overlap is a square of the short side
    q = box(12.0, -7.0, 0.5, 4.0, 2.0, 1.5, yaw + math.pi / 2)
    want = (2.0 * 2.0) / (2 * 8.0 - 4.0)            # = (min / max) / (2 - min / max) with min / max = 1 / 2
    assert iou64(a, q)[0] == pytest.approx(want, abs=1e-12)
    assert want == pytest.approx(0.5 / (2 - 0.5))
    # shifted by half its length along its own axis: 1 / 3
    h = box(12.0 + 2.0 * c, -7.0 + 2.0 * s, 0.5, 4.0, 2.0, 1.5, yaw)
    assert iou64(a, h) == pytest.approx((1 / 3, 1 / 3), abs=1e-12)
    # nested: the area ratio, the volume ratio
    n = box(12.0 + 0.5 * c, -7.0 + 0.5 * s, 0.5, 2.0, 1.0, 0.75, yaw + math.pi)
    assert iou64(a, n) == pytest.approx((2.0 / 8.0, 1.5 / 12.0), abs=1e-12)
    # half the height in common: 3D = (A h / 2) / (2 A h - A h / 2) = 1 / 3, BEV 1
    up = box(12.0, -7.0, 0.5 + 0.75, 4.0, 2.0, 1.5, yaw)
    assert iou64(a, up) == pytest.approx((1.0, 1 / 3), abs=1e-12)
    # the same pair with z the bottom: the same overlap
    assert iou64(a, up, 0.0) == pytest.approx((1.0, 1 / 3), abs=1e-12)
    # far apart
    assert iou64(a, box(40.0, 3.0, 0.5, 4.0, 2.0, 1.5, 1.0)) == (0.0, 0.0)


def test_touching_boxes_do_not_overlap():
    a = box(1.0, 2.0, 0.0, 4.0, 2.0, 1.5, 0.0)
    assert iou64(a, box(5.0, 2.0, 0.0, 4.0, 2.0, 1.5, 0.0)) == (0.0, 0.0)        # a shared edge
    assert iou64(a, box(1.0, 4.0, 0.0, 4.0, 2.0, 1.5, 0.0)) == (0.0, 0.0)
    assert iou64(a, box(5.0, 4.0, 0.0, 4.0, 2.0, 1.5, 0.0)) == (0.0, 0.0)        # a shared corner
    bev, v3 = iou64(a, box(1.0, 2.0, 1.5, 4.0, 2.0, 1.5, 0.0))                   # stacked: a shared face
    assert bev == pytest.approx(1.0, abs=1e-12) and v3 == 0.0


def test_z_origin():
    a, b = box(z=0.0, dz=2.0), box(z=1.0, dz=2.0)
    assert iou64(a, b, 0.5)[1] == pytest.approx(1 / 3) and iou64(a, b, 0.0)[1] == pytest.approx(1 / 3)
    c = box(z=1.0, dz=4.0)        # centre: [-1, 3] against [-1, 1]: contains a; bottom: [1, 5] against [0, 2]
    assert iou64(a, c, 0.5)[1] == pytest.approx(0.5) and iou64(a, c, 0.0)[1] == pytest.approx(1 / 5)


def test_invalid_rows_overlap_nothing():
    a = np.repeat(box(), 5, 0)
    b = a.copy()
    b[0, 1], b[1, 6], b[2, 3], b[3, 5], b[4, 4] = np.nan, np.inf, 0.0, -1.0, -np.inf
    for x, y in ((a, b), (b, a)):
        e, t = R.iou_pairs(x, y)
        assert (e == 0).all() and (t == 0).all()


def test_symmetry_of_the_float64_restatement():
    """iou(a, b) clips b in a's frame, iou(b, a) clips a in b's: two different computations of one number"""
    a, b = R.aligned_case()
    for x, y in zip(R.iou_pairs(a, b), R.iou_pairs(b, a)):
        assert np.abs(x - y).max() < 1e-12
    bev, v3 = R.iou_pairs(a, b)
    assert (bev > 0.999).sum() >= R.ALIGNED_PAIRS // 5 and (bev == 0).sum() > 0 and ((bev > 0.05) & (bev < 0.95)).sum() > 1000
    assert (bev <= 1 + 1e-12).all() and (v3 <= bev + 1e-12).all()


def test_matrix_equals_pairs():
    a, b = R.matrix_case(3)
    bev, v3 = R.iou_matrix(a, b)
    pb, p3 = R.iou_matrix(a, b, prune=True)
    assert np.array_equal(bev, pb) and np.array_equal(v3, p3)
    for i in (0, 17, 129):
        e, t = R.iou_pairs(np.repeat(a[i:i + 1], len(b), 0), b)
        assert np.array_equal(e, bev[i]) and np.array_equal(t, v3[i])


# ---- the tolerance -----------------------------------------------------------------------------------------------------
def test_float32_restatement_tolerance(parity_log):
    """The worst |float32 restatement - float64| over every input set of the device test: identical, quarter-turned,
    nested, touching and random pairs at scene offsets up to 150 m, yaw in +-7 rad.  1e-5 is a condition of the
    frame-local design, not the bar: the device test's bar is 8 times the measured value."""
    e32 = R.measure_e32()
    print(f"E32 = {e32:.3e}")
    parity_log.append(f"box_iou float32 restatement vs float64: {e32:.3e} (condition 1e-5)")
    assert e32 < 1e-5


# ---- the NMS loop and concat of the restatement ------------------------------------------------------------------------
def test_nms_restatement_chain_and_ties():
    b = np.repeat(box(), 3, 0)
    b[1, 0], b[2, 0] = 1.5, 3.0               # iou(0, 1) = iou(1, 2) = 2.5 / 5.5, iou(0, 2) = 1 / 7
    s = np.array([0.9, 0.8, 0.7])
    assert R.nms(b, s, 0.3) == [0, 2]          # 1 goes, so it cannot take 2 with it
    assert R.nms(b, s, 0.1) == [0]
    assert R.nms(b, s, 0.5) == [0, 1, 2]
    assert R.nms(b, np.array([0.5, 0.5, 0.5]), 0.3) == [0, 2]
    assert R.nms(b, np.array([0.0, -0.0, 0.5]), 0.3) == [2, 0]
    assert R.nms(b, np.array([0.9, np.nan, 0.7]), 0.3) == [0, 2]
    assert R.nms(b, s, 0.3, score_thr=0.75) == [0]
    assert R.nms(b, s, 0.3, count=2) == [0]
    assert R.nms(b, s, 0.3, labels=np.array([0, 1, 0])) == [0, 1, 2]
    assert R.margins(b, s, 0.3) == pytest.approx(min(abs(2.5 / 5.5 - 0.3), abs(1 / 7 - 0.3)))


def test_concat_restatement():
    b = np.zeros((2, 9))
    b[0] = (1, 2, 3, 4, 2, 1, 0.1, 1, 0)
    pose = np.eye(4)
    pose[:2, :2] = [[0, -1], [1, 0]]
    pose[:3, 3] = (10, 20, 30)
    ob, os_, ol, osrc = R.concat([(b, [0.5, 0.6], [1, 2], 1), (b, [0.7, 0.8], [3, 4])], [pose, None])
    assert np.allclose(ob[0], (8, 21, 33, 4, 2, 1, 0.1 + math.pi / 2, 0, 1))
    assert (ob[1] == 0).all() and os_[1] == -np.inf and ol[1] == -1
    assert np.array_equal(ob[2:], b) and list(osrc) == [0, 0, 1, 1] and list(ol) == [1, -1, 3, 4]


# ---- settings ----------------------------------------------------------------------------------------------------------
def test_nms_from_test_cfg():
    from projects.mmdet3d_plugin import synthetic as S
    from projects.mmdet3d_plugin.core.post_processing import nms_from_test_cfg
    with open(os.path.join(GOLDEN, "reference_test_cfg_nms.json")) as fh:
        ref = json.load(fh)["configs"]
    assert len(ref) == 13
    for name, cfg in ref.items():
        assert nms_from_test_cfg(cfg) is None, name
        assert nms_from_test_cfg(dict(pts=cfg)) is None, name
        assert nms_from_test_cfg(dict(cfg, nms_type="rotate")) == dict(iou_thr=0.2, use_rotate_nms=True), name
    for name in S.CONFIGS:
        assert nms_from_test_cfg(S.make_head_cfg(name)[0]["test_cfg"]) is None, name
    assert nms_from_test_cfg(dict(nms_type="circle", nms_thr=0.2)) is None
    with pytest.raises(ValueError, match="unknown nms_type"):
        nms_from_test_cfg(dict(nms_type="soft"))
    with pytest.raises(ValueError, match="needs nms_thr"):
        nms_from_test_cfg(dict(nms_type="rotate"))


def test_iou3d_cost():
    from projects.mmdet3d_plugin.core.bbox.match_costs import IoU3DCost
    iou = torch.tensor([[0.0, 0.25], [1.0, 0.5]])
    assert torch.equal(IoU3DCost(weight=2.0)(iou), torch.tensor([[-0.0, -0.5], [-2.0, -1.0]]))
    assert IoU3DCost(0.25).weight == 0.25
