"""Host side of the result pictures (native_render.py, core/visualizer): the ABI of cmt_render_* and its argument
errors (every one before any device work, with null or made-up pointers), the wrappers' ValueErrors, bev_view, the
PNG writer and reader, and tests/_render_ref.py's float32 restatement (a) against pictures worked out by hand.  No test
here needs a device.
"""
import ctypes
import os

import numpy as np
import pytest
import torch

import _render_ref as R

EINVAL = 1001
CALLS = ("points", "segments", "boxes", "digits", "resolve")
EYE = np.eye(4, dtype=np.float32)


@pytest.fixture(scope="module")
def NR():
    from projects.mmdet3d_plugin import native_render
    native_render.render_lib()
    return native_render


# ---- ABI ---------------------------------------------------------------------------------------------------------
def test_render_abi(NR):
    from projects.mmdet3d_plugin import native
    L = NR.render_lib()
    assert L.cmt_abi_version() == native.ABI_VERSION == 25
    for name in CALLS:
        assert hasattr(L, f"cmt_render_{name}")
        assert getattr(L, f"cmt_render_{name}_args_size")() == ctypes.sizeof(NR.STRUCTS[name]), name
    target = 4 * 4 + 2 * 4 + 8 * 16 * 4 + 8
    assert ctypes.sizeof(NR.RenderTarget) == target
    assert ctypes.sizeof(NR.RenderPointsArgs) == target + 6 * 4 + 2 * 4 + 3 * 8
    assert ctypes.sizeof(NR.RenderSegmentsArgs) == target + 4 * 4 + 5 * 8
    assert ctypes.sizeof(NR.RenderBoxesArgs) == target + 4 * 4 + 2 * 4 + 2 * 4 + 5 * 8
    assert ctypes.sizeof(NR.RenderDigitsArgs) == target + 4 * 4 + 2 * 4 + 4 * 8
    assert ctypes.sizeof(NR.RenderResolveArgs) == 4 * 4 + 2 * 4 + 3 * 8
    hdr = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "cmt_hip.h")).read()
    assert "result pictures: top view and camera overlays (render.hip; additive to ABI 25)" in hdr
    for name, value in (("CMT_RENDER_MAX_VIEWS", NR.MAX_VIEWS), ("CMT_RENDER_MAX_SIZE", NR.MAX_SIZE),
                        ("CMT_RENDER_MAX_ITEMS", NR.MAX_ITEMS)):
        assert f"#define {name} {value}\n" in hdr
    # the font of the header is the font of the reference
    for g in R.FONT:
        assert "{" + ",".join(f"0x{b:02X}" for b in g) + "}" in hdr


def _target(t, **over):
    t.V, t.H, t.W, t.layer, t.near, t.plane = 1, 5, 7, 0, 0.1, 0x10000
    for e in range(16):
        t.view[0][e] = float(EYE.reshape(-1)[e])
    for k, v in over.items():
        if k == "view":
            t.view[v[0]][v[1]] = v[2]
        else:
            setattr(t, k, v)


def _good(NR, name):
    """a struct the call accepts up to the launch (made-up aligned pointers: never passed on unbroken)"""
    a = NR.STRUCTS[name]()
    P = 0x10000
    if name == "points":
        _target(a.t)
        a.N, a.ld, a.radius, a.color_col, a.lo, a.inv_span, a.points, a.lut = 4, 4, 0, -1, 0.0, 1.0, P, P
    elif name == "segments":
        _target(a.t)
        a.S, a.thickness, a.p0, a.p1, a.rgb = 3, 1, P, P, P
    elif name == "boxes":
        _target(a.t)
        a.M, a.ld, a.thickness, a.z_origin, a.boxes = 3, 7, 1, 0.5, P
    elif name == "digits":
        _target(a.t)
        a.M, a.scale, a.values, a.anchors = 3, 1, P, P
    else:
        a.V, a.H, a.W, a.plane, a.out = 1, 5, 7, P, P
    return a


TARGET_ERRORS = [dict(V=0), dict(V=9), dict(H=0), dict(H=4097), dict(W=0), dict(W=4097), dict(layer=-1), dict(layer=256),
                 dict(near=float("nan")), dict(near=float("inf")), dict(plane=None), dict(plane=0x10004)]
OWN_ERRORS = {
    "points": [dict(N=-1), dict(ld=2), dict(color_col=-2), dict(color_col=4), dict(radius=-1), dict(radius=3),
               dict(lo=float("nan")), dict(inv_span=float("inf")), dict(points=None), dict(lut=None), dict(points=0x10002),
               dict(lut=0x10001), dict(n=0x10002)],
    "segments": [dict(S=-1), dict(S=1 << 20), dict(thickness=0), dict(thickness=4), dict(p0=None), dict(p1=None),
                 dict(rgb=None), dict(p0=0x10002), dict(rank=0x10001), dict(n=0x10003)],
    "boxes": [dict(M=-1), dict(M=1 << 20), dict(ld=6), dict(z_origin=0.25), dict(thickness=0), dict(thickness=4),
              dict(score_thr=float("nan")), dict(ncls=-1), dict(boxes=None), dict(boxes=0x10002), dict(count=0x10002),
              dict(labels=0x10001), dict(scores=0x10002), dict(class_rgb=0x10002)],
    "digits": [dict(M=-1), dict(M=1 << 20), dict(scale=0), dict(scale=5), dict(values=None), dict(anchors=None),
               dict(values=0x10002), dict(anchors=0x10002), dict(rgb=0x10001), dict(rank=0x10002)],
    "resolve": [dict(V=0), dict(V=9), dict(H=0), dict(H=4097), dict(W=0), dict(W=4097), dict(plane=None),
                dict(plane=0x10004), dict(out=None)],
}


@pytest.mark.parametrize("name", CALLS)
def test_c_argument_errors_before_any_device_work(NR, name):
    L = NR.render_lib()
    fn = getattr(L, f"cmt_render_{name}")
    assert fn(None, None) == EINVAL and f"cmt_render_{name}" in L.cmt_last_error().decode()
    cases = [("own", e) for e in OWN_ERRORS[name]]
    if name != "resolve":
        cases += [("target", e) for e in TARGET_ERRORS] + [("target", dict(view=(0, 5, float("nan"))))]
    for where, over in cases:
        a = _good(NR, name)
        for k, v in over.items():
            if where == "target":
                _target(a.t, **{k: v})
            else:
                setattr(a, k, v)
        assert fn(ctypes.byref(a), None) == EINVAL, (name, over)
        assert f"cmt_render_{name}" in L.cmt_last_error().decode()
    if name in ("segments", "digits"):   # a planar call reads no view: a NaN entry passes the checks up to the count
        a = _good(NR, name)
        a.planar = 1
        a.t.view[0][5] = float("nan")
        setattr(a, "S" if name == "segments" else "M", 0)
        assert fn(ctypes.byref(a), None) == 0
    if name != "resolve":                # a count of 0 is a valid call that launches nothing
        a = _good(NR, name)
        setattr(a, {"points": "N", "segments": "S", "boxes": "M", "digits": "M"}[name], 0)
        assert fn(ctypes.byref(a), None) == 0


# ---- the wrappers' ValueErrors (host tensors: the checks come before the device check) ---------------------------
def _plane(V=1, H=5, W=7):
    return torch.zeros((V, H, W), dtype=torch.int64)


def test_wrapper_value_errors(NR):
    pl, pts, lut = _plane(), torch.zeros((4, 5)), torch.zeros(256, dtype=torch.int32)
    i3 = torch.zeros(3, dtype=torch.int32)
    bad = [
        lambda: NR.new_plane(0, 5, 7, "cpu"), lambda: NR.new_plane(9, 5, 7, "cpu"), lambda: NR.new_plane(1, 4097, 7, "cpu"),
        lambda: NR.render_points(pl.int(), EYE, pts, lut), lambda: NR.render_points(pl[0], EYE, pts, lut),
        lambda: NR.render_points(pl, np.zeros((2, 4, 4)), pts, lut),
        lambda: NR.render_points(pl, EYE * np.nan, pts, lut),
        lambda: NR.render_points(pl, EYE, pts[:, :2], lut), lambda: NR.render_points(pl, EYE, pts.double(), lut),
        lambda: NR.render_points(pl, EYE, pts, lut[:255]), lambda: NR.render_points(pl, EYE, pts, lut.long()),
        lambda: NR.render_points(pl, EYE, pts, lut, radius=3), lambda: NR.render_points(pl, EYE, pts, lut, radius=-1),
        lambda: NR.render_points(pl, EYE, pts, lut, color_col=5), lambda: NR.render_points(pl, EYE, pts, lut, color_col=-2),
        lambda: NR.render_points(pl, EYE, pts, lut, span=0.0), lambda: NR.render_points(pl, EYE, pts, lut, lo=float("nan")),
        lambda: NR.render_points(pl, EYE, pts, lut, n=3), lambda: NR.render_points(pl, EYE, pts, lut, layer=256),
        lambda: NR.render_points(pl, EYE, pts, lut, near=float("inf")),
        lambda: NR.render_segments(pl, EYE, torch.zeros((3, 2)), torch.zeros((3, 3)), i3),
        lambda: NR.render_segments(pl, EYE, torch.zeros((3, 3)), torch.zeros((2, 3)), i3),
        lambda: NR.render_segments(pl, EYE, torch.zeros((3, 3)), torch.zeros((3, 3)), i3.long()),
        lambda: NR.render_segments(pl, EYE, torch.zeros((3, 3)), torch.zeros((3, 3)), i3, rank=i3[:2]),
        lambda: NR.render_segments(pl, EYE, torch.zeros((3, 3)), torch.zeros((3, 3)), i3, thickness=4),
        lambda: NR.render_segments(pl, None, torch.zeros((3, 3)), torch.zeros((3, 3)), i3, planar=True),
        lambda: NR.render_boxes(pl, EYE, torch.zeros((3, 6))), lambda: NR.render_boxes(pl, EYE, torch.zeros((3, 7)), z_origin=1.0),
        lambda: NR.render_boxes(pl, EYE, torch.zeros((3, 7)), labels=i3.long()),
        lambda: NR.render_boxes(pl, EYE, torch.zeros((3, 7)), scores=torch.zeros(2)),
        lambda: NR.render_boxes(pl, EYE, torch.zeros((3, 7)), score_thr=float("nan")),
        lambda: NR.render_boxes(pl, EYE, torch.zeros((3, 7)), rgb_default=1 << 24),
        lambda: NR.render_boxes(pl, EYE, torch.zeros((3, 7)), thickness=0),
        lambda: NR.render_boxes(pl, EYE, torch.zeros((3, 7)), count=torch.zeros(2, dtype=torch.int32)),
        lambda: NR.render_digits(pl, EYE, i3.long(), torch.zeros((3, 3))),
        lambda: NR.render_digits(pl, EYE, i3, torch.zeros((3, 2))), lambda: NR.render_digits(pl, EYE, i3, torch.zeros((3, 3)), scale=5),
        lambda: NR.render_digits(pl, EYE, i3, torch.zeros((3, 3)), rgb=-1),
        lambda: NR.render_digits(pl, EYE, i3, torch.zeros((3, 3)), rgb=i3[:2]),
        lambda: NR.render_resolve(pl.int()), lambda: NR.render_resolve(pl, background=1 << 24),
        lambda: NR.render_resolve(pl, src=torch.zeros((1, 5, 7, 4), dtype=torch.uint8)),
        lambda: NR.render_resolve(pl, out=torch.zeros((1, 5, 7, 3))),
    ]
    for k, f in enumerate(bad):
        with pytest.raises(ValueError):
            f()
            pytest.fail(f"case {k} raised nothing")
    # a good call on host tensors: the last check is the device's
    with pytest.raises(ValueError, match="HIP device"):
        NR.render_points(pl, EYE, pts, lut)
    with pytest.raises(ValueError, match="HIP device"):
        NR.render_resolve(pl)


def test_visualizer_value_errors_and_show():
    from projects.mmdet3d_plugin.core.visualizer import Visualizer, show_results
    with pytest.raises(ValueError):
        Visualizer(["car"], [0, 0, 0, 1, 1], device="cpu")
    with pytest.raises(ValueError):
        Visualizer(["car"], [0, 0, 0, 1, 1, 1], bev_size=(5000, 10), device="cpu")
    with pytest.raises(NotImplementedError, match="display"):
        show_results(None, {}, [], "x", show=True)
    from projects.mmdet3d_plugin.models.detectors import CmtCoopDetector, CmtDetector
    import inspect
    assert list(inspect.signature(CmtDetector.show_results).parameters) == ["self", "data", "result", "out_dir", "show", "score_thr"]
    assert list(inspect.signature(CmtCoopDetector.show_results).parameters)[-1] == "gt_bboxes"


def test_cli_flags(capsys):
    import importlib.util
    from conftest import PKG
    spec = importlib.util.spec_from_file_location("cmt_test_cli_render", os.path.join(PKG, "tools", "test.py"))
    cli = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(cli)
    a = cli.parse_args(["cmt_lidar_nus", "--synthetic", "--show-dir", "pics"])      # an operation of its own
    assert a.show_dir == "pics" and a.show_score_thr is None and not a.show
    assert cli.parse_args(["cmt_lidar_nus", "--synthetic", "--eval", "bbox"]).show_dir is None
    for argv in (["--show"], ["--show", "--show-dir", "pics"], ["--show", "--eval", "bbox"]):
        with pytest.raises(SystemExit) as e:
            cli.parse_args(["cmt_lidar_nus", "--synthetic"] + argv)
        assert e.value.code == 2 and "--show-dir" in capsys.readouterr().err
    with pytest.raises(SystemExit) as e:                                             # still: no operation at all
        cli.parse_args(["cmt_lidar_nus", "--synthetic"])
    assert e.value.code == 2 and '"--out", "--eval" or "--format-only"' in capsys.readouterr().err


# ---- bev_view, luts, palette -------------------------------------------------------------------------------------
@pytest.mark.parametrize("mpp,size", [(0.25, 432), (0.5, 216)])
def test_bev_view_exact(NR, mpp, size):
    pcr = [-54.0, -54.0, -5.0, 54.0, 54.0, 3.0]
    m = NR.bev_view(pcr, size, size)
    assert m.dtype == np.float32 and m.shape == (4, 4)
    s = 1.0 / mpp
    assert m.tolist() == [[s, 0, 0, 54.0 * s], [0, -s, 0, 54.0 * s], [0, 0, 1, 0], [0, 0, 0, 1]]
    # every grid position lands exactly on its pixel corner through the header's float32 row formula
    for x, y in ((-54.0, 54.0), (0.0, 0.0), (53.75, -53.5), (-12.25, 7.5)):
        x32, y32, z32 = np.float32(x), np.float32(y), np.float32(1.0)
        assert float(R.row(m, 0, x32, y32, z32)) == (x + 54.0) * s
        assert float(R.row(m, 1, x32, y32, z32)) == (54.0 - y) * s
        assert float(R.row(m, 2, x32, y32, z32)) == 1.0 and float(R.row(m, 3, x32, y32, z32)) == 1.0
    with pytest.raises(ValueError):
        NR.bev_view([0, 0, 0, 0, 1, 1], 8, 8)
    cam = NR.camera_view(np.arange(16.0).reshape(4, 4))
    assert cam.dtype == np.float32 and cam.tolist() == [[0, 1, 2, 3], [4, 5, 6, 7], [8, 9, 10, 11], [8, 9, 10, 11]]
    with pytest.raises(ValueError):
        NR.camera_view(np.zeros((3, 4)))


def test_luts_and_palette(NR):
    for lut in (NR.height_lut(0), NR.height_lut(1), NR.depth_lut()):
        assert lut.dtype == np.int32 and lut.shape == (256,) and (lut >= 0).all() and (lut <= 0xFFFFFF).all()
    assert not np.array_equal(NR.height_lut(0), NR.height_lut(1))
    pal = NR.class_palette(14)
    assert pal.dtype == np.int32 and pal.shape == (14,) and pal[12] == pal[0] and len(set(pal[:12].tolist())) == 12
    assert NR.GT_RGB not in pal.tolist()


# ---- PNG ---------------------------------------------------------------------------------------------------------
def test_png_round_trip(tmp_path):
    from projects.mmdet3d_plugin.core.visualizer import read_png, write_png
    rng = np.random.default_rng(0)
    for shape in ((1, 1, 3), (5, 7, 3), (37, 53, 3)):
        img = rng.integers(0, 256, shape, dtype=np.uint8)
        path = str(tmp_path / f"p{shape[1]}.png")
        write_png(path, torch.from_numpy(img))
        assert np.array_equal(read_png(path), img)
    for bad in (img.astype(np.float32), img[:, :, :2], img[0]):
        with pytest.raises(ValueError):
            write_png(path, bad)
    junk = str(tmp_path / "junk.png")
    open(junk, "wb").write(b"not a png")
    with pytest.raises(ValueError):
        read_png(junk)


def test_png_is_read_by_pillow(tmp_path):
    Image = pytest.importorskip("PIL.Image")
    from projects.mmdet3d_plugin.core.visualizer import write_png
    img = np.random.default_rng(1).integers(0, 256, (9, 13, 3), dtype=np.uint8)
    path = str(tmp_path / "p.png")
    write_png(path, img)
    with Image.open(path) as im:
        assert im.mode == "RGB" and np.array_equal(np.asarray(im), img)


# ---- reference (a) against pictures worked out by hand -----------------------------------------------------------
def test_key_packing_and_okey(NR):
    assert R.pack(2, 0xFFFFFFFF, 0x123456) == (2 << 56) | (0xFFFFFFFF << 24) | 0x123456
    assert R.pack(255, 1, 0xFFFFFF) == (255 << 56) | (1 << 24) | 0xFFFFFF < 1 << 64
    fmax, den = np.finfo(np.float32).max, np.float32(1e-45)
    vals = [-fmax, np.float32(-1.0), -np.finfo(np.float32).tiny, -den, np.float32(-0.0), np.float32(0.0), den,
            np.finfo(np.float32).tiny, np.float32(1.0), fmax]
    keys = [R.okey(v) for v in vals]
    assert keys == sorted(keys) and len(set(keys)) == len(keys)
    assert all(0 < k < 0xFFFFFFFF for k in keys)
    assert R.okey(np.float32(-0.0)) + 1 == R.okey(np.float32(0.0)) == 0x80000000
    assert R.okey(-np.inf) > 0 and R.okey(np.inf) < 0xFFFFFFFF


def test_ref_one_point():
    pl = R.Plane(1, 5, 7)
    lut = np.arange(256, dtype=np.int64) * 0x010101
    # identity view: u = x, v = y, d = z; the point (3.5, 2.25) lies in pixel (3, 2)
    R.points(pl, [EYE], 0.1, 0, np.array([[3.5, 2.25, 0.5, 9.0]], np.float32), lut, color_col=-1, lo=0.0, inv_span=1.0)
    want = np.zeros((1, 5, 7), dtype=np.uint64)
    want[0, 2, 3] = R.pack(0, R.okey(np.float32(0.5)), 127 * 0x010101)     # floor(0.5 * 255) = 127
    assert np.array_equal(pl.k, want)
    img = R.resolve(pl, background=0x0A0B0C)
    assert img.shape == (1, 5, 7, 3) and img[0, 2, 3].tolist() == [127, 127, 127] and img[0, 0, 0].tolist() == [10, 11, 12]
    # on the right and lower edge (u == W, v == H) nothing; at 0 the first pixel; behind the view nothing
    pl = R.Plane(1, 5, 7)
    R.points(pl, [EYE], 0.1, 0, np.array([[7.0, 1.0, 1.0], [1.0, 5.0, 1.0], [0.0, 0.0, 1.0], [np.nan, 1.0, 1.0]], np.float32), lut)
    assert np.count_nonzero(pl.k) == 1 and pl.k[0, 0, 0] != 0
    far = EYE.copy()
    far[3] = [0, 0, 1, 0]                                                   # row 3 = z: a camera along z
    pl = R.Plane(1, 5, 7)
    R.points(pl, [far], 0.1, 0, np.array([[1.0, 1.0, 0.05], [1.0, 1.0, -2.0]], np.float32), lut)
    assert not pl.k.any()


def test_ref_rectangle_and_diagonal():
    pl = R.Plane(1, 8, 10)
    p0 = [(2.5, 1.5), (6.5, 1.5), (6.5, 5.5), (2.5, 5.5)]
    p1 = p0[1:] + p0[:1]
    R.segments(pl, None, 0.1, 3, p0, p1, [0xFF0000] * 4, planar=True)
    want = np.zeros((8, 10), dtype=bool)
    want[1, 2:7] = want[5, 2:7] = True
    want[1:6, 2] = want[1:6, 6] = True
    assert np.array_equal(pl.k[0] != 0, want)
    # ranks: segment 0 lies on top at the shared corner (2, 1)
    assert int(pl.k[0, 1, 2]) == R.pack(3, 0xFFFFFFFF, 0xFF0000) and int(pl.k[0, 5, 6]) == R.pack(3, 0xFFFFFFFF - 1, 0xFF0000)
    pl = R.Plane(1, 8, 10)
    R.segments(pl, None, 0.1, 0, [(1.2, 1.7)], [(5.9, 5.1)], [0x00FF00], planar=True)      # (1, 1) -> (5, 5)
    assert sorted(zip(*np.nonzero(pl.k[0]))) == [(i, i) for i in range(1, 6)]
    # the same through a camera view: row 3 = z, ends at depth 2 with doubled coordinates
    cam = EYE.copy()
    cam[3] = [0, 0, 1, 0]
    pl2 = R.Plane(1, 8, 10)
    R.segments(pl2, [cam], 0.1, 0, [(2.4, 3.4, 2.0)], [(11.8, 10.2, 2.0)], [0x00FF00])
    assert np.array_equal(pl2.k, pl.k)
    # thickness 3 at the border is clipped to the picture
    pl = R.Plane(1, 4, 4)
    R.segments(pl, None, 0.1, 0, [(0.5, 0.5)], [(0.5, 0.5)], [1], planar=True, thickness=3)
    assert sorted(zip(*np.nonzero(pl.k[0]))) == [(0, 0), (0, 1), (1, 0), (1, 1)]
    pl = R.Plane(1, 4, 4)
    R.segments(pl, None, 0.1, 0, [(1.5, 1.5)], [(1.5, 1.5)], [1], planar=True, thickness=2)
    assert sorted(zip(*np.nonzero(pl.k[0]))) == [(1, 1), (1, 2), (2, 1), (2, 2)]


def test_ref_digit_eight_and_number():
    pl = R.Plane(1, 9, 14)
    R.digits(pl, None, 0.1, 4, [8], [(1.0, 1.0)], planar=True)
    rows = ["01110", "10001", "10001", "01110", "10001", "10001", "01110"]
    want = np.zeros((9, 14), dtype=bool)
    for cy, bits in enumerate(rows):
        for cx, b in enumerate(bits):
            want[1 + cy, 1 + cx] = b == "1"
    assert np.array_equal(pl.k[0] != 0, want)
    assert [f"{b:05b}" for b in R.FONT[8]] == rows
    # "10" : the 1 at column 0, the 0 at column 6; -1 draws nothing; scale 2 doubles every cell
    pl = R.Plane(1, 9, 14)
    R.digits(pl, None, 0.1, 4, [10, -1], [(0.0, 0.0), (0.0, 0.0)], planar=True)
    got = pl.k[0] != 0
    assert got[:7, :5].sum() == sum(bin(b).count("1") for b in R.FONT[1]) and not got[:, 5].any()
    assert got[:7, 6:11].sum() == sum(bin(b).count("1") for b in R.FONT[0]) and not got[:, 11:].any() and not got[7:].any()
    big = R.Plane(1, 20, 30)
    R.digits(big, None, 0.1, 4, [8], [(2.0, 2.0)], planar=True, scale=2)
    assert np.array_equal((big.k[0] != 0)[2:16, 2:12], np.kron(want[1:8, 1:6], np.ones((2, 2), dtype=bool)))


def test_walk_is_the_same_from_either_end():
    rng = np.random.default_rng(5)
    ends = rng.integers(-40, 40, (2000, 4))
    for X0, Y0, X1, Y1 in ends.tolist() + [[0, 0, 0, 0], [0, 0, 7, 0], [3, 9, 3, -2], [0, 0, 1, 2], [0, 0, 2, 1]]:
        fwd, back = R.walk(X0, Y0, X1, Y1), R.walk(X1, Y1, X0, Y0)
        assert fwd == back[::-1]
        assert fwd[0] == (X0, Y0) and fwd[-1] == (X1, Y1) and len(fwd) == max(abs(X1 - X0), abs(Y1 - Y0)) + 1
        assert all(max(abs(a[0] - b[0]), abs(a[1] - b[1])) == 1 for a, b in zip(fwd, fwd[1:]))


def test_ref_a_and_b_agree_on_exact_boxes():
    """yaw 0 and -0, centres and sizes on the 0.25 m grid, a power-of-two view: every operation is exact in both"""
    from projects.mmdet3d_plugin import native_render as NRm
    view = NRm.bev_view([-8.0, -8.0, -4.0, 8.0, 8.0, 4.0], 64, 64)
    rows = np.array([[1.25, -2.5, 0.5, 4.0, 2.0, 1.5, 0.0], [-3.0, 3.25, 0.0, 2.5, 1.25, 2.0, -0.0]], np.float32)
    a, b = R.Plane(1, 64, 64), R.Plane(1, 64, 64)
    R.boxes(a, [view], 0.5, 2, rows, labels=[0, 1], class_rgb=[0x111111, 0x222222])
    R.boxes64(b, [view], 0.5, 2, rows, labels=[0, 1], class_rgb=[0x111111, 0x222222])
    assert a.k.any() and np.array_equal(a.k, b.k)
