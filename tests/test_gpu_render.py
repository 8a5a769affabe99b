"""cmt_render_* / Visualizer / --show-dir on the device against tests/_render_ref.py.

Points, segments, digits and resolve contain no transcendental: the key plane and the resolved picture equal the
float32 restatement (a) bit for bit.  Boxes equal (a) and the float64 geometry (b) bit for bit where every operation is
exact (yaw +-0, the 0.25 m grid, power-of-two scales); with random yaw every line pixel of the device lies within
Chebyshev distance 1 of a line pixel of (b) and the reverse.  That 1 is derived: corner coordinates below 4096 px
carry an error far below 1e-3 px (a handful of float32 roundings, sinf / cosf at a few ulp), so a floored end moves by
at most one pixel, and a one-pixel shift of an end moves the walk's pixel set by at most one pixel (checked on 4 000
random segments with every +-1 shift of the four end coordinates: worst distance 1).
Every buffer stands between guard words that must stay intact.
"""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import _render_ref as R
from conftest import PKG

pytestmark = pytest.mark.gpu

H, W = 37, 53
GUARD = 64          # elements of guard on either side of every buffer
LUT = (np.arange(256, dtype=np.int64) * 0x010203 % 0xFFFFFF + 1).astype(np.int32)


@pytest.fixture(scope="module")
def NR(dev):
    from projects.mmdet3d_plugin import native_render
    native_render.render_lib()
    return native_render


class Guarded:
    """device buffers between guard words; ``check`` asserts every guard is intact"""

    def __init__(self, dev):
        self.dev, self.held = dev, []

    def put(self, arr, cols=None):
        """``arr`` (numpy) -> a device tensor between guards; ``cols``: the view shows only the first ``cols`` columns"""
        arr = np.ascontiguousarray(arr)
        t = torch.from_numpy(arr.reshape(-1).copy())
        fill = {torch.float32: 12345.0, torch.uint8: 0xA5}.get(t.dtype, 0x5A5A5A5A)
        flat = torch.full((t.numel() + 2 * GUARD,), fill, dtype=t.dtype)
        flat[GUARD:GUARD + t.numel()] = t
        flat = flat.to(self.dev)
        self.held.append((flat, t.numel(), fill))
        inner = flat[GUARD:GUARD + t.numel()].view(arr.shape)
        return inner if cols is None else inner[:, :cols]

    def plane(self, V, h=H, w=W):
        return self.put(np.zeros((V, h, w), dtype=np.int64))

    def check(self):
        for flat, n, fill in self.held:
            g = torch.cat([flat[:GUARD], flat[GUARD + n:]]).cpu()
            assert bool((g == fill).all()), "a guard word was overwritten"


def keys(plane):
    return plane.cpu().numpy().view(np.uint64)


ORTHO = np.array([[2, 0, 0, 26.5], [0, -2, 0, 18.5], [0, 0, 1, 0], [0, 0, 0, 1]], dtype=np.float32)


def cam_views():
    from projects.mmdet3d_plugin import synthetic as S
    from projects.mmdet3d_plugin import native_render
    return np.stack([native_render.camera_view(S.camera_lidar2img(y, f=30.0, cx=26.5, cy=18.5)) for y in (0.0, 90.0)])


# ---- points ------------------------------------------------------------------------------------------------------
def _cloud(n, seed, camera):
    rng = np.random.default_rng(seed)
    p = np.zeros((n, 8), dtype=np.float32)
    # a 0.25 m grid and four heights: many points share a pixel at equal depth, so the rgb tie rule decides
    p[:, 0] = np.round(rng.uniform(-15, 15, n) * 4) / 4
    p[:, 1] = np.round(rng.uniform(-11, 11, n) * 4) / 4
    p[:, 2] = rng.integers(0, 4, n) * 0.5 - 1.0
    p[:, 3] = rng.uniform(-0.2, 1.2, n)          # the colour column, beyond [lo, lo + span] on both sides
    p[:, 4:] = 777.0
    special = [(13.25, 0.0), (-13.25, 0.0), (0.0, -9.25), (0.0, 9.25), (13.0, 9.0), (-13.25, 9.25)]   # on the edges
    for k, (x, y) in enumerate(special[:max(0, n - 4)]):
        p[k + 1, :2] = (x, y)
    if n >= 10:
        p[7, 0], p[8, 1], p[9, 2] = np.nan, np.inf, -np.inf
        p[6, 3] = np.nan                            # a NaN colour is index 0
    if camera and n >= 14:
        p[10, :3] = (-5.0, 1.0, 1.0)                # behind camera 0
        p[11, :3] = (0.05, 0.0, 1.5)                # before the near plane of camera 0
        p[12, :3] = (5.0, 0.0, 1.5)                 # on the axis of camera 0: the picture's centre
        p[13, :3] = (5.0, 0.0, 1.5)
    return p


@pytest.mark.parametrize("n", [1, 63, 64, 65, 1000])
@pytest.mark.parametrize("camera", [False, True])
def test_points(NR, dev, n, camera):
    views = cam_views() if camera else ORTHO[None]
    V = len(views)
    near = 0.1 if camera else 0.5
    cloud = _cloud(n, n + camera, camera)
    count = n - n // 4
    for radius in (0, 2):
        kw = dict(radius=radius, near_wins=camera, color_col=-1 if camera else 3, lo=0.0 if camera else 0.1,
                  span=20.0 if camera else 0.8)
        inv = float(np.float32(1.0) / np.float32(kw["span"]))
        want = R.Plane(V, H, W)
        R.points(want, views, near, 0, cloud[:, :6], LUT, n=count, radius=radius, near_wins=camera,
                 color_col=kw["color_col"], lo=kw["lo"], inv_span=inv)
        assert want.k.any() or n == 1
        g = Guarded(dev)
        pts, lut, cnt = g.put(cloud, cols=6), g.put(LUT), g.put(np.array([count], dtype=np.int32))
        planes = []
        for rep in range(2):
            pl = g.plane(V)
            NR.render_points(pl, views, pts, lut, n=cnt, near=near, **kw)
            planes.append(keys(pl))
        assert np.array_equal(planes[0], want.k)
        assert np.array_equal(planes[1], planes[0])
        img = NR.render_resolve(pl, background=0x102030)
        assert np.array_equal(img.cpu().numpy(), R.resolve(want, background=0x102030))
        # the same points in reverse order, all of them: the plane does not depend on the order
        full, rev = g.plane(V), g.plane(V)
        NR.render_points(full, views, pts, lut, near=near, **kw)
        NR.render_points(rev, views, g.put(cloud[::-1], cols=6), lut, near=near, **kw)
        assert np.array_equal(keys(full), keys(rev))
        g.check()


# ---- segments ----------------------------------------------------------------------------------------------------
def _planar_segments():
    rng = np.random.default_rng(3)
    p0 = rng.uniform(-10, 63, (65, 2)).astype(np.float32)
    p1 = rng.uniform(-10, 50, (65, 2)).astype(np.float32)
    fixed = [((-20.0, 10.0), (80.0, 25.0)),              # both ends outside, the middle inside
             ((-1e6, -1e6), (1e6, 1e6 + 30.0)),          # a million pixels away on both sides
             ((1e6, 5.0), (2e6, 6.0)),                   # outside on one side: nothing
             ((10.5, 10.5), (10.5, 10.5)),               # length zero, inside
             ((-5.0, -5.0), (-5.0, -5.0)),               # length zero, outside
             ((0.5, 0.5), (52.5, 0.5)), ((52.5, 0.5), (52.5, 36.5)),   # along the border: thickness 3 is clipped
             ((np.nan, 1.0), (5.0, 5.0)), ((1.0, 1.0), (np.inf, 5.0)),
             ((3.0, 30.0), (40.0, 30.0)), ((40.0, 30.0), (3.0, 30.0)),  # the same pixels, ranks collide below
             ((-3e38, 0.0), (3e38, 10.0))]               # dx overflows: dropped
    for k, (a, b) in enumerate(fixed):
        p0[k], p1[k] = a, b
    rgb = rng.integers(1, 1 << 24, 65).astype(np.int32)
    rank = rng.integers(0, 8, 65).astype(np.int32)       # many equal ranks: the rgb decides
    rank[5] = -3                                         # a negative rank counts as 0
    return p0, p1, rgb, rank


@pytest.mark.parametrize("S_", [0, 1, 65])
def test_segments_planar(NR, dev, S_):
    p0, p1, rgb, rank = [a[:S_] for a in _planar_segments()]
    for thick, use_rank, V in ((1, True, 1), (3, False, 2), (2, True, 1)):
        want = R.Plane(V, H, W)
        R.segments(want, None, 0.1, 3, p0, p1, rgb, rank=rank if use_rank else None, thickness=thick, planar=True)
        g = Guarded(dev)
        pl = g.plane(V)
        NR.render_segments(pl, None, g.put(p0), g.put(p1), g.put(rgb), rank=g.put(rank) if use_rank else None,
                           thickness=thick, planar=True)
        assert np.array_equal(keys(pl), want.k)
        assert want.k.any() == (S_ > 0)
        g.check()


def test_segments_camera(NR, dev):
    views = cam_views()
    rng = np.random.default_rng(4)
    p0 = np.stack([rng.uniform(-6, 12, 65), rng.uniform(-6, 12, 65), rng.uniform(-1, 3, 65)], 1).astype(np.float32)
    p1 = np.stack([rng.uniform(-6, 12, 65), rng.uniform(-6, 12, 65), rng.uniform(-1, 3, 65)], 1).astype(np.float32)
    p0[0], p1[0] = (-4.0, 0.5, 1.0), (8.0, -0.5, 2.0)        # one end behind camera 0
    p0[1], p1[1] = (-4.0, 0.5, 1.0), (-8.0, -0.5, 2.0)       # both behind camera 0
    p0[2], p1[2] = (0.1, 0.0, 1.5), (6.0, 1.0, 1.5)          # an end exactly on the near plane
    p0[3], p1[3] = (5.0, -40.0, 1.5), (5.0, 40.0, 1.5)       # both ends outside the picture, the middle inside
    p0[4], p1[4] = (np.nan, 0.0, 0.0), (5.0, 0.0, 0.0)
    rgb = rng.integers(1, 1 << 24, 65).astype(np.int32)
    count = 60
    for thick in (1, 3):
        want = R.Plane(2, H, W)
        R.segments(want, views, 0.1, 3, p0, p1, rgb, n=count, thickness=thick)
        g = Guarded(dev)
        pl = g.plane(2)
        NR.render_segments(pl, views, g.put(p0), g.put(p1), g.put(rgb), n=g.put(np.array([count], np.int32)), thickness=thick)
        assert want.k[0].any() and want.k[1].any()
        assert np.array_equal(keys(pl), want.k)
        g.check()


# ---- boxes -------------------------------------------------------------------------------------------------------
def _near(a, b, inner=False):
    """every set pixel of a has a set pixel of b within Chebyshev distance 1.  ``inner``: only the pixels of a that are
    not on the picture's outermost ring are held to it (the partner of a ring pixel may lie outside the picture)"""
    if inner:
        a = a.copy()
        a[..., 0, :] = a[..., -1, :] = a[..., :, 0] = a[..., :, -1] = False
    grown = np.zeros_like(b)
    Hh, Ww = b.shape[-2:]
    for dy in (-1, 0, 1):
        for dx in (-1, 0, 1):
            ys, yd = slice(max(dy, 0), Hh + min(dy, 0)), slice(max(-dy, 0), Hh + min(-dy, 0))
            xs, xd = slice(max(dx, 0), Ww + min(dx, 0)), slice(max(-dx, 0), Ww + min(-dx, 0))
            grown[..., yd, xd] |= b[..., ys, xs]
    return bool((~a | grown).all())


def test_boxes_exact(NR, dev):
    view = NR.bev_view([-8.0, -8.0, -4.0, 8.0, 8.0, 4.0], 64, 64)[None]
    rows = np.array([[1.25, -2.5, 0.5, 4.0, 2.0, 1.5, 0.0, 9, 9], [-3.0, 3.25, 0.0, 2.5, 1.25, 2.0, -0.0, 9, 9],
                     [1.0, -2.0, 0.0, 6.0, 3.0, 1.0, 0.0, 9, 9]], np.float32)
    over = np.array([[2.0, -2.5, 0.5, 2.0, 4.0, 1.5, 0.0], [-3.0, 3.0, 0.0, 1.0, 3.0, 2.0, -0.0]], np.float32)
    labels, palette = np.array([0, 1, 7], np.int32), np.array([0x111111, 0x222222], np.int32)
    a, b = R.Plane(1, 64, 64), R.Plane(1, 64, 64)
    for ref, pl in ((R.boxes, a), (R.boxes64, b)):
        ref(pl, view, 0.5, 1, rows, labels=labels, class_rgb=palette, rgb_default=0x00FF00)
        ref(pl, view, 0.5, 2, over, z_origin=0.0, rgb_default=0xFF00FF, thickness=2)
    g = Guarded(dev)
    pl = g.plane(1, 64, 64)
    NR.render_boxes(pl, view, g.put(over), z_origin=0.0, rgb_default=0xFF00FF, layer=2, near=0.5, thickness=2)
    NR.render_boxes(pl, view, g.put(rows, cols=7), labels=g.put(labels), class_rgb=g.put(palette), rgb_default=0x00FF00,
                    layer=1, near=0.5)
    got = keys(pl)
    assert np.array_equal(got, a.k) and np.array_equal(got, b.k)
    # layer 2 lies over layer 1 where they cross
    lo, hi = R.Plane(1, 64, 64), R.Plane(1, 64, 64)
    R.boxes(lo, view, 0.5, 1, rows, rgb_default=1)
    R.boxes(hi, view, 0.5, 2, over, z_origin=0.0, rgb_default=2, thickness=2)
    cross = (lo.k != 0) & (hi.k != 0)
    assert cross.any() and ((got[cross] >> np.uint64(56)) == 2).all()
    assert ((got[(lo.k != 0) & (hi.k == 0)] >> np.uint64(56)) == 1).all()
    g.check()


def _inside(corners, view, Hh, Ww, margin=2.0):
    m = np.asarray(view, dtype=np.float64)
    for c in corners:
        r = m @ np.array([*c, 1.0])
        u, v = r[0] / r[3], r[1] / r[3]
        if not (r[3] > 0.5 and margin <= u <= Ww - margin and margin <= v <= Hh - margin):
            return False
    return True


@pytest.mark.parametrize("camera", [False, True])
def test_boxes_random_yaw(NR, dev, camera):
    from projects.mmdet3d_plugin import synthetic as S
    rng = np.random.default_rng(11 + camera)
    if camera:
        Hh, Ww, near = 128, 256, 0.1
        view = NR.camera_view(S.camera_lidar2img(0.0, f=100.0, cx=128.0, cy=64.0))[None]
    else:
        Hh, Ww, near = 128, 128, 0.5
        view = NR.bev_view([-32.0, -32.0, -5.0, 32.0, 32.0, 3.0], Hh, Ww)[None]
    rows = []
    while len(rows) < 40:
        if camera:
            x = rng.uniform(10, 40)
            r = [x, rng.uniform(-0.4, 0.4) * x, rng.uniform(-0.5, 1.5)]
        else:
            r = [rng.uniform(-25, 25), rng.uniform(-25, 25), rng.uniform(-2, 1)]
        r += [rng.uniform(1, 4), rng.uniform(1, 4), rng.uniform(1, 2), rng.uniform(-np.pi, np.pi)]
        r = np.array(r, np.float32)
        corners, head = R.box_corners64(r, 0.5)
        if _inside(corners, view[0], Hh, Ww):      # all corners inside the picture, two pixels from its border
            rows.append(r)
    rows = np.stack(rows)
    want = R.Plane(1, Hh, Ww)
    R.boxes64(want, view, near, 2, rows)
    g = Guarded(dev)
    pl = g.plane(1, Hh, Ww)
    NR.render_boxes(pl, view, g.put(rows), near=near)
    got, ref = keys(pl) != 0, want.k != 0
    assert ref.sum() > 40 * 10
    assert _near(got, ref) and _near(ref, got)
    g.check()


@pytest.mark.parametrize("camera", [False, True])
def test_boxes_clipped(NR, dev, camera):
    """Boxes across the picture's border and across the camera's near plane: the box kernel's segments go through the
    near clip and Liang-Barsky.  Against (b) with the same criterion as above, derived the same way: the clipped ends
    are a few more float32 operations on coordinates below 4096 px, so a floored end still moves by at most one pixel.
    A pixel on the outermost ring may have its partner outside the picture, so the ring is not held to the criterion."""
    from projects.mmdet3d_plugin import synthetic as S
    rng = np.random.default_rng(21 + camera)
    rows = []
    if camera:
        Hh, Ww, near = 128, 256, 0.1
        view = NR.camera_view(S.camera_lidar2img(0.0, f=100.0, cx=128.0, cy=64.0))[None]
        for k in range(24):
            if k < 8:        # across the near plane: the box reaches behind the camera
                r = [rng.uniform(0.8, 2.0), rng.uniform(-1.5, 1.5), rng.uniform(0.0, 1.0), rng.uniform(3.0, 4.0),
                     rng.uniform(1.0, 2.0), rng.uniform(1.0, 2.0), rng.uniform(-0.3, 0.3)]
            else:            # across the left, right, upper or lower border
                x = rng.uniform(6, 30)
                r = [x, rng.choice([-1.0, 1.0]) * rng.uniform(1.1, 1.5) * x, rng.uniform(-0.5, 1.5), rng.uniform(2, 4),
                     rng.uniform(2, 4), rng.uniform(1, 2), rng.uniform(-np.pi, np.pi)]
                if k % 2:
                    r[0], r[1], r[5] = rng.uniform(2.5, 4.0), rng.uniform(-1.0, 1.0), 4.0
            rows.append(r)
    else:
        Hh, Ww, near = 128, 128, 0.5
        view = NR.bev_view([-32.0, -32.0, -5.0, 32.0, 32.0, 3.0], Hh, Ww)[None]
        for k in range(24):
            c = [rng.choice([-1.0, 1.0]) * rng.uniform(30.5, 33.5), rng.uniform(-34, 34)][::1 if k % 2 else -1]
            rows.append(c + [rng.uniform(-2, 1), rng.uniform(2, 5), rng.uniform(2, 5), rng.uniform(1, 2),
                             rng.uniform(-np.pi, np.pi)])
    rows = np.array(rows, np.float32)
    want = R.Plane(1, Hh, Ww)
    R.boxes64(want, view, near, 2, rows)
    ref = want.k != 0
    ring = np.zeros_like(ref)
    ring[..., 0, :] = ring[..., -1, :] = ring[..., :, 0] = ring[..., :, -1] = True
    assert (ref & ring).sum() >= 8 and (ref & ~ring).sum() > 24 * 5     # lines do cross the border
    g = Guarded(dev)
    pl = g.plane(1, Hh, Ww)
    NR.render_boxes(pl, view, g.put(rows), near=near)
    got = keys(pl) != 0
    assert _near(got, ref, inner=True) and _near(ref, got, inner=True)
    g.check()


def test_boxes_that_draw_nothing(NR, dev):
    view = NR.bev_view([-8.0, -8.0, -4.0, 8.0, 8.0, 4.0], 64, 64)[None]
    good = np.array([[0.0, 0.0, 0.0, 4.0, 2.0, 1.5, 0.3]] * 4, np.float32)
    bad = good.copy()
    bad[0, 0], bad[1, 3], bad[2, 5], bad[3, 6] = np.nan, 0.0, -1.0, np.inf
    g = Guarded(dev)
    pl = g.plane(1, 64, 64)
    NR.render_boxes(pl, view, g.put(bad), near=0.5)
    NR.render_boxes(pl, view, g.put(good), count=g.put(np.array([0], np.int32)), near=0.5)
    NR.render_boxes(pl, view, g.put(good), count=g.put(np.array([-5], np.int32)), near=0.5)
    NR.render_boxes(pl, view, g.put(good), scores=g.put(np.array([0.3, 0.1, np.nan, -1.0], np.float32)), score_thr=0.3, near=0.5)
    NR.render_boxes(pl, view, torch.zeros((0, 7), device=dev), near=0.5)
    assert not keys(pl).any()
    # rows at or beyond count and at or below the threshold: only row 1 of four is drawn
    NR.render_boxes(pl, view, g.put(good), count=g.put(np.array([2], np.int32)),
                    scores=g.put(np.array([0.3, 0.31, 0.9, 0.9], np.float32)), score_thr=0.3, near=0.5)
    got = keys(pl)
    assert got.any() and set(((got[got != 0] >> np.uint64(24)) & np.uint64(0xFFFFFFFF)).tolist()) == {0xFFFFFFFF - 1}
    g.check()


# ---- digits ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("scale", [1, 3])
def test_digits(NR, dev, scale):
    values = np.array([0, 7, 10, 2147483647, -1, 8], np.int32)
    planar = np.array([[1.5, 1.0], [20.0, 1.2], [40.0, 2.0], [2.0, 12.0], [10.0, 25.0], [50.0, 28.0]], np.float32)  # the last is clipped on the right
    rgb = np.array([0xFF0000, 0x00FF00, 0x0000FF, 0xFFFF00, 0xFFFFFF, 0x00FFFF], np.int32)
    want = R.Plane(2, H, W)
    R.digits(want, None, 0.1, 4, values, planar, rgb=rgb, scale=scale, planar=True)
    g = Guarded(dev)
    pl = g.plane(2)
    NR.render_digits(pl, None, g.put(values), g.put(planar), rgb=g.put(rgb), scale=scale, planar=True)
    assert np.array_equal(keys(pl), want.k) and want.k[1].any()
    assert (want.k[0][:, W - 1] != 0).any()          # the clipped number reaches the last column
    # through the top view, one colour, ranks given
    anchors = np.array([[-13.0, 9.0, 0.0], [0.0, 0.0, 1.0], [5.25, -3.5, 0.0], [-12.0, 2.0, 0.0], [1.0, 1.0, 0.0],
                        [np.nan, 0.0, 0.0]], np.float32)
    rank = np.array([3, 3, 0, 1, 2, 0], np.int32)
    want = R.Plane(1, H, W)
    R.digits(want, ORTHO[None], 0.5, 4, values, anchors, rgb_one=0xABCDEF, rank=rank, scale=scale)
    pl = g.plane(1)
    NR.render_digits(pl, ORTHO[None], g.put(values), g.put(anchors), rgb=0xABCDEF, rank=g.put(rank), scale=scale, near=0.5)
    assert np.array_equal(keys(pl), want.k) and want.k.any()
    g.check()


# ---- resolve -----------------------------------------------------------------------------------------------------
def test_resolve(NR, dev):
    rng = np.random.default_rng(9)
    want = R.Plane(2, H, W)
    R.segments(want, None, 0.1, 1, [(0.0, 0.0), (52.0, 0.0)], [(52.0, 36.0), (0.0, 36.0)], [0x123456, 0xFEDCBA], planar=True)
    src = rng.integers(0, 256, (2, H, W, 3), dtype=np.uint8)
    g = Guarded(dev)
    pl = g.put(want.k.view(np.int64))
    out = g.put(np.zeros((2, H, W, 3), np.uint8))
    assert NR.render_resolve(pl, background=0x0A0B0C, out=out) is out
    assert np.array_equal(out.cpu().numpy(), R.resolve(want, background=0x0A0B0C))
    frames = g.put(src)
    res = NR.render_resolve(pl, src=frames, out=out)
    assert np.array_equal(res.cpu().numpy(), R.resolve(want, src=src)) and np.array_equal(frames.cpu().numpy(), src)
    res = NR.render_resolve(pl, src=frames, out=frames)          # in place
    assert res is frames and np.array_equal(frames.cpu().numpy(), R.resolve(want, src=src))
    g.check()


# ---- Visualizer, show_results ------------------------------------------------------------------------------------
PCR = [-54.0, -54.0, -5.0, 54.0, 54.0, 3.0]


def _has_colour(img, colours):
    px = (img[..., 0].astype(np.int64) << 16) | (img[..., 1].astype(np.int64) << 8) | img[..., 2]
    return bool(np.isin(px, np.asarray(colours, dtype=np.int64)).any())


def test_visualizer_on_a_coop_sample(NR, dev):
    from projects.mmdet3d_plugin import synthetic as S
    from projects.mmdet3d_plugin.core.visualizer import Visualizer
    names = ["CAR", "TRUCK", "BUS"]
    vis = Visualizer(names, PCR, bev_size=(160, 200), device=dev)
    clouds = [S.synthetic_points(3000, PCR, seed=k, device=dev) for k in (0, 1)]
    boxes, labels = S.synthetic_gt(1, PCR, 3, n=20, seed=2, device=dev)
    scores = torch.linspace(0.9, 0.05, 20, device=dev)
    count = torch.tensor([15], dtype=torch.int32, device=dev)
    ids = torch.arange(20, dtype=torch.int32, device=dev) - 1
    trails = [np.cumsum(np.ones((5, 3), np.float32), 0), np.zeros((1, 3), np.float32)]
    kw = dict(boxes=boxes[0], scores=scores, labels=labels[0], count=count, gt_boxes=boxes[0][:5] + 1.0, track_ids=ids,
              trails=trails, score_thr=0.2, z_origin=0.5)
    bev = vis.bev(clouds, **kw)
    assert bev.dtype == torch.uint8 and tuple(bev.shape) == (160, 200, 3) and bev.device == dev
    img = bev.cpu().numpy()
    assert _has_colour(img, NR.class_palette(3)) and _has_colour(img, [NR.GT_RGB, NR.DIGIT_RGB])
    assert torch.equal(vis.bev(clouds, **kw), bev)                  # bitwise repeatable
    assert not _has_colour(vis.bev(clouds).cpu().numpy(), NR.class_palette(3))
    frames = S.synthetic_frames(3, 90, 160, seed=3, device=dev)
    before = frames.clone()
    l2i = [S.camera_lidar2img(y, f=126.6, cx=80.0, cy=19.0) for y in S.INFRA_YAWS]
    cams = vis.cameras(frames, l2i, points=clouds, **kw)
    assert cams.dtype == torch.uint8 and tuple(cams.shape) == (3, 90, 160, 3)
    assert torch.equal(frames, before) and not torch.equal(cams, before)
    assert _has_colour(cams.cpu().numpy(), NR.class_palette(3))
    same = vis.cameras(frames, l2i, points=clouds, inplace=True, **kw)
    assert same.data_ptr() == frames.data_ptr() and torch.equal(frames, cams)


def test_show_results_writes_the_tensor(NR, dev, tmp_path):
    from projects.mmdet3d_plugin import build_detector
    from projects.mmdet3d_plugin import synthetic as S
    from projects.mmdet3d_plugin.core.visualizer import Visualizer, read_png
    cfg = S.make_detector_cfg("cmt_lidar_nus", num_query=32, num_layers=1, grid_size=[256, 256, 40])
    torch.manual_seed(0)
    model = build_detector(cfg)
    model.init_weights()
    model = model.eval().to(dev)
    pcr = cfg["pts_voxel_layer"]["point_cloud_range"]
    pts = [S.synthetic_points(2000, pcr, seed=5, device=dev)]
    data = dict(points=[pts], img_metas=[[dict(pts_filename="/data/sweeps/frame_0007.bin")]])
    with torch.no_grad():
        result = model(return_loss=False, **data)
    written = model.show_results(data, result, str(tmp_path), score_thr=None)
    assert [os.path.basename(p) for p in written] == ["frame_0007_bev.png"]
    names = [n for t in model.pts_bbox_head.class_names for n in t]
    r = result[0]["pts_bbox"]
    want = Visualizer(names, model.pts_bbox_head.pc_range, device=dev).bev(
        pts, boxes=r["boxes_3d"], scores=r["scores_3d"], labels=r["labels_3d"], z_origin=0.0)
    got = read_png(written[0])
    assert got.shape == (800, 800, 3) and np.array_equal(got, want.cpu().numpy())
    assert _has_colour(got, NR.class_palette(len(names)))
    with pytest.raises(NotImplementedError):
        model.show_results(data, result, str(tmp_path), show=True)


def test_visualizer_corner_cases(NR, dev):
    """trails without boxes are drawn; an invalid row with a finite centre gets no number; inplace needs the caller's
    frames as they are"""
    from projects.mmdet3d_plugin.core.visualizer import Visualizer
    vis = Visualizer(["a"], [-8.0, -8.0, -4.0, 8.0, 8.0, 4.0], bev_size=(64, 64), device=dev)
    img = vis.bev([], trails=[np.array([[-4, -4, 0], [4, 4, 0]], np.float32)]).cpu().numpy()
    assert _has_colour(img, [NR.TRAIL_RGB]) and (img.reshape(-1, 3).any(1)).sum() >= 30
    rows = torch.tensor([[0, 0, 0, 2, 2, 1, 0.0], [3, 3, 0, 0.0, 2, 1, 0.0], [-3, -3, 0, 2, 2, 1, float("nan")]], device=dev)
    ids = torch.tensor([5, 6, 7], dtype=torch.int32, device=dev)
    both = vis.bev([], boxes=rows, track_ids=ids, z_origin=0.5)
    assert torch.equal(both, vis.bev([], boxes=rows[:1], track_ids=ids[:1], z_origin=0.5))
    assert _has_colour(both.cpu().numpy(), [NR.DIGIT_RGB])
    frames = torch.zeros((1, 16, 16, 3), dtype=torch.uint8)
    view = [np.eye(4)]
    with pytest.raises(ValueError, match="inplace"):
        vis.cameras(frames, view, inplace=True)                       # on the host
    with pytest.raises(ValueError, match="inplace"):
        vis.cameras(frames.to(dev).expand(1, 16, 16, 3)[:, :, ::2], view, inplace=True)   # not contiguous
    assert tuple(vis.cameras(frames, view).shape) == (1, 16, 16, 3)  # without inplace a copy is made


# ---- the CLI -----------------------------------------------------------------------------------------------------
def _cli_module(name):
    import importlib.util
    spec = importlib.util.spec_from_file_location(name, os.path.join(PKG, "tools", "test.py"))
    cli = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(cli)
    return cli


def test_cli_show_dir_detector_cameras(NR, dev, tmp_path, capsys):
    """tools/test.py --detector --show-dir in this process on the coop fusion config: both agents' frames get their
    overlays through the uncropped lidar2img (the vehicle's moved into the infrastructure frame by --sweeps' pose), the
    pictures are numbered across the agents (1 vehicle camera, 3 infrastructure cameras), ground truth from --eval nds,
    boxes after --nms.  The frame and model sizes are those of test_cli_detector_ida_size."""
    from projects.mmdet3d_plugin.core.visualizer import read_png
    cli = _cli_module("cmt_test_cli_render_det")
    out = tmp_path / "pics"
    seen = []
    real = cli.detector_frame_inputs

    def spy(*a, **kw):
        res = real(*a, **kw)
        seen.append([(f.clone(), [np.asarray(m) for m in l2i]) for f, l2i in kw["show"]])
        return res
    cli.detector_frame_inputs = spy
    rc = cli.main(["cmtcoop_fusion_tumtraf", "--synthetic", "--detector", "--num-query", "32", "--num-layers", "1",
                   "--grid", "32", "32", "--frame-size", "150", "384", "--ida-size", "188", "320", "--points", "1000",
                   "--sweeps", "1", "--cfg-options", "bbox_coder.max_num=200", "--nms", "rotate", "--eval", "nds",
                   "--show-dir", str(out)])
    assert rc == 0
    assert f"wrote 5 pictures to {out}" in capsys.readouterr().out.splitlines()
    assert sorted(os.listdir(out)) == ["000000_bev.png"] + [f"000000_cam{v}.png" for v in range(4)]
    assert read_png(str(out / "000000_bev.png")).shape == (800, 800, 3)
    (veh, inf), = seen
    assert veh[0].shape == (1, 150, 384, 3) and inf[0].shape == (3, 150, 384, 3) and len(veh[1]) == 1 and len(inf[1]) == 3
    # the uncropped lidar2img: the intrinsics of the frame as loaded; the vehicle's differs from a camera at the origin
    # by the vehicle-to-infrastructure pose, the infrastructure's does not
    from projects.mmdet3d_plugin import synthetic as S
    K = np.eye(4)
    K[0, 0] = K[1, 1] = 1266.0 * 384 / 1600.0
    K[0, 2], K[1, 2] = 192.0, 75.0
    for m, y in zip(inf[1], S.INFRA_YAWS):
        assert np.allclose(m, K @ S.camera_lidar2img(y, f=1.0, cx=0.0, cy=0.0), atol=1e-9)
    assert not np.allclose(veh[1][0], K @ S.camera_lidar2img(S.VEHICLE_YAWS[0], f=1.0, cx=0.0, cy=0.0), atol=1e-3)
    frames = [veh[0][0]] + list(inf[0])
    for v, f in enumerate(frames):       # every picture is its frame with overlays: same size, most pixels untouched
        img = read_png(str(out / f"000000_cam{v}.png"))
        same = (img == f.cpu().numpy()).all(-1).mean()
        assert img.shape == (150, 384, 3) and 0.5 < same
    changed = sum(int((read_png(str(out / f"000000_cam{v}.png")) != f.cpu().numpy()).any()) for v, f in enumerate(frames))
    assert changed >= 1                  # 1000 points a cloud: some camera sees some


def test_cli_show_dir_coop_nms_eval(NR, dev, tmp_path, capsys):
    """the README's second command at a small model size, in this process: both agents' clouds, --nms, ground truth"""
    from projects.mmdet3d_plugin.core.visualizer import read_png
    cli = _cli_module("cmt_test_cli_render_coop")
    out = tmp_path / "pics"
    rc = cli.main(["cmtcoop_lidar_tumtraf", "--synthetic", "--frames", "2", "--nms", "rotate", "--eval", "nds",
                   "--num-query", "32", "--num-layers", "1", "--cfg-options", "bbox_coder.max_num=200", "--show-dir", str(out)])
    assert rc == 0 and f"wrote 2 pictures to {out}" in capsys.readouterr().out.splitlines()
    for f in ("000000_bev.png", "000001_bev.png"):
        img = read_png(str(out / f))
        assert _has_colour(img, [NR.GT_RGB]) and _has_colour(img, NR.class_palette(7))
        assert _has_colour(img, NR.height_lut(0)) and _has_colour(img, NR.height_lut(1))     # both agents' ramps

def _run_cli(args):
    cmd = ["timeout", "-k", "10", "120", sys.executable, os.path.join(PKG, "tools", "test.py")] + args
    return subprocess.run(cmd, capture_output=True, text=True)


def test_cli_show_dir(NR, tmp_path):
    from projects.mmdet3d_plugin.core.visualizer import read_png
    base = ["cmt_lidar_nus", "--synthetic", "--num-query", "32", "--num-layers", "1", "--frames", "2", "--track"]
    out, res = tmp_path / "pics", tmp_path / "r.json"
    # --show-dir alone is an operation (tests/test_render_host.py); here beside one of today's, so that the same
    # command without the flag can be compared: the flag adds its one line and changes nothing else
    with_flag = _run_cli(base + ["--out", str(res), "--show-dir", str(out)])
    assert with_flag.returncode == 0, with_flag.stderr[-2000:]
    first = res.read_text()
    assert sorted(os.listdir(out)) == ["000000_bev.png", "000001_bev.png"]
    for f in sorted(os.listdir(out)):
        img = read_png(str(out / f))
        assert img.shape == (800, 800, 3) and _has_colour(img, NR.class_palette(10))     # the prediction palette
        assert _has_colour(img, [NR.DIGIT_RGB])                                          # --track: ids are drawn
    without = _run_cli(base + ["--out", str(res)])
    assert without.returncode == 0, without.stderr[-2000:]
    assert without.stdout.splitlines() == [f"writing results to {res}"]
    assert with_flag.stdout.splitlines() == without.stdout.splitlines() + [f"wrote 2 pictures to {out}"]
    assert res.read_text() == first
    bad = _run_cli(base + ["--show"])                 # refused by the parser, before torch is imported
    assert bad.returncode == 2 and "--show-dir" in bad.stderr
