"""Result pictures on the device: cmt_render_points / _segments / _boxes / _digits / _resolve (include/cmt_hip.h).

A picture in progress is an int64 [V, H, W] key plane (``new_plane``; the library reads it as uint64) that every
drawing call only raises with atomic maxima, so the finished plane does not depend on the order of anything and is
bitwise repeatable.  ``resolve`` turns it into uint8 [V, H, W, 3] pictures.  Colours are 0xRRGGBB; colour arrays are
int32 tensors (the library reads the low 24 bits).  ``views`` is a HOST [V, 4, 4] array: ``bev_view`` gives the
orthographic matrix of the top view, ``camera_view`` the matrix of a camera from its ``lidar2img``.

Like native_iou.py: argument checks raise ValueError before the device check, tensors must live on a HIP device,
there is no CPU fallback.  No call here reads a result back.
"""
import ctypes
import math

import numpy as np
import torch

from ._argcheck import count_word as _count, same_device, strided_rows, tensor
from .native import _check, _flt, _i64, _int, _p, _stream, _vp, lib

__all__ = ["MAX_VIEWS", "MAX_SIZE", "MAX_ITEMS", "LAYER_POINTS", "LAYER_GT", "LAYER_PRED", "LAYER_TRAILS", "LAYER_DIGITS",
           "render_lib", "new_plane", "bev_view", "camera_view", "height_lut", "depth_lut", "class_palette",
           "render_points", "render_segments", "render_boxes", "render_digits", "render_resolve"]

MAX_VIEWS, MAX_SIZE, MAX_ITEMS = 8, 4096, 1 << 20   # cmt_hip.h CMT_RENDER_MAX_VIEWS, _MAX_SIZE, _MAX_ITEMS
LAYER_POINTS, LAYER_GT, LAYER_PRED, LAYER_TRAILS, LAYER_DIGITS = 0, 1, 2, 3, 4
_u32 = ctypes.c_uint32


class RenderTarget(ctypes.Structure):
    _fields_ = [("V", _int), ("H", _int), ("W", _int), ("layer", _int), ("near", _flt), ("reserved_f", _flt),
                ("view", (_flt * 16) * MAX_VIEWS), ("plane", _vp)]


class RenderPointsArgs(ctypes.Structure):
    _fields_ = [("t", RenderTarget), ("N", _int), ("ld", _int), ("radius", _int), ("near_wins", _int),
                ("color_col", _int), ("reserved", _int), ("lo", _flt), ("inv_span", _flt),
                ("points", _vp), ("n", _vp), ("lut", _vp)]


class RenderSegmentsArgs(ctypes.Structure):
    _fields_ = [("t", RenderTarget), ("S", _int), ("planar", _int), ("thickness", _int), ("reserved", _int),
                ("p0", _vp), ("p1", _vp), ("rgb", _vp), ("rank", _vp), ("n", _vp)]


class RenderBoxesArgs(ctypes.Structure):
    _fields_ = [("t", RenderTarget), ("M", _int), ("ld", _int), ("thickness", _int), ("ncls", _int),
                ("z_origin", _flt), ("score_thr", _flt), ("rgb_default", _u32), ("reserved", _u32),
                ("boxes", _vp), ("count", _vp), ("labels", _vp), ("scores", _vp), ("class_rgb", _vp)]


class RenderDigitsArgs(ctypes.Structure):
    _fields_ = [("t", RenderTarget), ("M", _int), ("planar", _int), ("scale", _int), ("reserved", _int),
                ("rgb_one", _u32), ("reserved_u", _u32), ("values", _vp), ("anchors", _vp), ("rgb", _vp), ("rank", _vp)]


class RenderResolveArgs(ctypes.Structure):
    _fields_ = [("V", _int), ("H", _int), ("W", _int), ("reserved", _int), ("background", _u32), ("reserved_u", _u32),
                ("plane", _vp), ("src", _vp), ("out", _vp)]


STRUCTS = {"points": RenderPointsArgs, "segments": RenderSegmentsArgs, "boxes": RenderBoxesArgs,
           "digits": RenderDigitsArgs, "resolve": RenderResolveArgs}
_READY = False


def render_lib():
    """libcmt_hip.so with the cmt_render_* signatures set and the struct mirrors checked (no device needed)"""
    global _READY
    L = lib()
    if not _READY:
        for name, st in STRUCTS.items():
            size = getattr(L, f"cmt_render_{name}_args_size")
            size.argtypes, size.restype = [], _i64
            fn = getattr(L, f"cmt_render_{name}")
            fn.argtypes, fn.restype = [ctypes.POINTER(st), _vp], _int
            if size() != ctypes.sizeof(st):
                raise RuntimeError(f"cmt_render_{name}_args: library struct is {size()} bytes, the ctypes mirror "
                                   f"{ctypes.sizeof(st)} (stale binding)")
        _READY = True
    return L


# ---- host helpers ----------------------------------------------------------------------------------------------

def bev_view(point_cloud_range, H, W):
    """The orthographic 4 x 4 matrix of the top view of ``point_cloud_range`` (x0 y0 z0 x1 y1 z1) at H x W pixels: +x
    to the right, +y up, the depth is z.  With a power-of-two number of metres per pixel every entry, and every
    product with a coordinate on that grid, is exact."""
    x0, y0, _, x1, y1, _ = [float(v) for v in point_cloud_range]
    H, W = int(H), int(W)
    if not (x1 > x0 and y1 > y0) or H < 1 or W < 1:
        raise ValueError(f"bev_view needs x1 > x0, y1 > y0 and a picture of at least 1 x 1, got {point_cloud_range}, {H} x {W}")
    sx, sy = W / (x1 - x0), H / (y1 - y0)
    return np.array([[sx, 0.0, 0.0, -x0 * sx], [0.0, -sy, 0.0, y1 * sy], [0.0, 0.0, 1.0, 0.0], [0.0, 0.0, 0.0, 1.0]],
                    dtype=np.float32)


def camera_view(lidar2img):
    """The view of a camera from its 4 x 4 ``lidar2img`` (rows: u * depth, v * depth, depth, 0 0 0 1): row 3 becomes a
    copy of the depth row, so that u = row 0 / row 3 and v = row 1 / row 3 as the contract divides -> float32 [4, 4]"""
    m = np.array(lidar2img.detach().cpu().numpy() if torch.is_tensor(lidar2img) else lidar2img, dtype=np.float64)
    if m.shape != (4, 4) or not np.isfinite(m).all():
        raise ValueError(f"lidar2img must be a finite 4 x 4 matrix, got shape {m.shape}")
    m[3] = m[2]
    return m.astype(np.float32)


def _ramp(stops):
    """256 colours, piecewise linear between (position 0..1, (r, g, b)) stops, as a host int32 array"""
    pos = np.array([s[0] for s in stops])
    t = np.arange(256) / 255.0
    ch = [np.rint(np.interp(t, pos, [s[1][c] for s in stops])).astype(np.int64) for c in range(3)]
    return ((ch[0] << 16) | (ch[1] << 8) | ch[2]).astype(np.int32)


def height_lut(kind=0):
    """the colour ramp of a cloud by height, host int32 [256]: 0 blue -> cyan -> yellow -> white (the vehicle's cloud),
    1 purple -> red -> orange -> light yellow (the infrastructure's), so two clouds in one picture stay apart"""
    if kind % 2 == 0:
        return _ramp([(0.0, (30, 60, 160)), (0.4, (40, 190, 210)), (0.75, (230, 230, 90)), (1.0, (255, 255, 255))])
    return _ramp([(0.0, (90, 30, 130)), (0.4, (220, 50, 60)), (0.75, (250, 160, 40)), (1.0, (255, 245, 190))])


def depth_lut():
    """the colour ramp of camera overlays by depth, host int32 [256]: near red -> yellow -> green -> far blue"""
    return _ramp([(0.0, (255, 40, 40)), (0.33, (250, 230, 50)), (0.66, (60, 220, 90)), (1.0, (50, 90, 255))])


_PALETTE = (0xFF9E00, 0xFF6347, 0xFFD700, 0xFF7F50, 0xE96C46, 0xDC143C, 0xFF3D63, 0x4FA5FF, 0xC88CFF, 0x70E000,
            0x00CFBF, 0xF032E6)


def class_palette(n):
    """n box colours (0xRRGGBB), a fixed list repeated: host int32 [n].  None of them is a grey, so a prediction's
    pixels can be told from the point ramps' white end and from the ground truth's colour."""
    return np.array([_PALETTE[i % len(_PALETTE)] for i in range(int(n))], dtype=np.int32)


GT_RGB = 0x00FF00
TRAIL_RGB = 0xFFFFFF
DIGIT_RGB = 0xFFFF00


def new_plane(V, H, W, device):
    """a cleared key plane: int64 [V, H, W] zeros"""
    V, H, W = _size(V, H, W)
    return torch.zeros((V, H, W), dtype=torch.int64, device=device)


# ---- argument checks -------------------------------------------------------------------------------------------

def _size(V, H, W):
    V, H, W = int(V), int(H), int(W)
    if not 1 <= V <= MAX_VIEWS or not 1 <= H <= MAX_SIZE or not 1 <= W <= MAX_SIZE:
        raise ValueError(f"a picture set has 1..{MAX_VIEWS} views of 1..{MAX_SIZE} pixels a side, got {V} x {H} x {W}")
    return V, H, W


def _target(t, plane, views, near, layer):
    """fill the cmt_render_target ``t``; ``views`` None: the call applies no view (planar)"""
    if not torch.is_tensor(plane) or plane.dtype != torch.int64 or plane.dim() != 3 or not plane.is_contiguous():
        raise ValueError("plane must be a contiguous int64 [V, H, W] tensor (new_plane)")
    V, H, W = _size(*plane.shape)
    layer, near = int(layer), float(near)
    if not 0 <= layer <= 255:
        raise ValueError(f"layer must be 0..255, got {layer}")
    if not math.isfinite(near):
        raise ValueError(f"near must be finite, got {near}")
    if views is not None:
        m = np.asarray(views.detach().cpu().numpy() if torch.is_tensor(views) else views, dtype=np.float32)
        if m.shape == (4, 4):
            m = m[None]
        if m.shape != (V, 4, 4) or not np.isfinite(m).all():
            raise ValueError(f"views must be a finite [{V}, 4, 4] host array (one matrix per picture of the plane), got "
                             f"shape {m.shape}")
        for v in range(V):
            for e, val in enumerate(m[v].reshape(-1)):
                t.view[v][e] = float(val)
    t.V, t.H, t.W, t.layer, t.near, t.plane = V, H, W, layer, near, _p(plane)
    return V, H, W


def _int_in(v, lo, hi, name):
    v = int(v)
    if not lo <= v <= hi:
        raise ValueError(f"{name} must be {lo}..{hi}, got {v}")
    return v


def _rgb(v, name):
    v = int(v)
    if not 0 <= v <= 0xFFFFFF:
        raise ValueError(f"{name} must be a colour 0xRRGGBB, got {v:#x}")
    return v


def _on_device(dev, **ts):
    same_device(dev, "the render calls need tensors", **ts)


# ---- the calls -------------------------------------------------------------------------------------------------

def render_points(plane, views, points, lut, *, n=None, layer=LAYER_POINTS, near=0.1, radius=0, near_wins=False,
                  color_col=-1, lo=0.0, span=1.0):
    """cmt_render_points.  ``points`` fp32 [N, >= 3] (rows may be views with a row stride; NaN rows are skipped),
    ``lut`` int32 [256] colours on the device, ``n`` None or a device int32.  The colour index of a point is
    ``floor((c - lo) / span * 255)`` clamped to 0..255 with c the column ``color_col`` (-1: the view's depth); the
    library multiplies with the float32 ``1 / span``.  ``near_wins``: the smaller depth covers (cameras); otherwise
    the larger (the top view: the highest point)."""
    g = RenderPointsArgs()
    N, ld = strided_rows(points, "points", 3)
    _target(g.t, plane, views, near, layer)
    lut = tensor(lut, "lut", torch.int32, (256,))
    _count(n, "n")
    radius = _int_in(radius, 0, 2, "radius")
    color_col = _int_in(color_col, -1, int(points.shape[1]) - 1, "color_col")
    lo, span = float(lo), float(span)
    if not math.isfinite(lo) or not math.isfinite(span) or span == 0.0:
        raise ValueError(f"lo must be finite and span finite and not 0, got {lo}, {span}")
    _on_device(plane.device, points=points, lut=lut, n=n)
    L = render_lib()
    if N == 0:
        return plane
    g.N, g.ld, g.radius, g.near_wins, g.color_col = N, ld, radius, int(bool(near_wins)), color_col
    g.lo, g.inv_span = lo, float(np.float32(1.0) / np.float32(span))
    g.points, g.n, g.lut = _p(points), _p(n), _p(lut)
    _check(L.cmt_render_points(ctypes.byref(g), _stream()), "cmt_render_points")
    return plane


def render_segments(plane, views, p0, p1, rgb, *, rank=None, n=None, layer=LAYER_TRAILS, near=0.1, thickness=1,
                    planar=False):
    """cmt_render_segments.  ``p0``, ``p1`` fp32 [S, 3] scene positions, or with ``planar`` [S, 2] pixel coordinates
    (``views`` is ignored, every picture of the plane gets the segment); ``rgb`` int32 [S]; ``rank`` None (the index)
    or int32 [S], the lower rank on top; ``n`` None or a device int32."""
    g = RenderSegmentsArgs()
    c = 2 if planar else 3
    p0 = tensor(p0, "p0", torch.float32, (None, c))
    S = int(p0.shape[0])
    p1 = tensor(p1, "p1", torch.float32, (S, c))
    rgb = tensor(rgb, "rgb", torch.int32, (S,))
    if rank is not None:
        rank = tensor(rank, "rank", torch.int32, (S,))
    if S >= MAX_ITEMS:
        raise ValueError(f"a call draws fewer than {MAX_ITEMS} segments, got {S}")
    _target(g.t, plane, None if planar else views, near, layer)
    _count(n, "n")
    thickness = _int_in(thickness, 1, 3, "thickness")
    _on_device(plane.device, p0=p0, p1=p1, rgb=rgb, rank=rank, n=n)
    L = render_lib()
    if S == 0:
        return plane
    g.S, g.planar, g.thickness = S, int(bool(planar)), thickness
    g.p0, g.p1, g.rgb, g.rank, g.n = _p(p0), _p(p1), _p(rgb), _p(rank), _p(n)
    _check(L.cmt_render_segments(ctypes.byref(g), _stream()), "cmt_render_segments")
    return plane


def render_boxes(plane, views, boxes, *, z_origin=0.5, count=None, labels=None, scores=None, score_thr=0.0,
                 class_rgb=None, rgb_default=0xFFFFFF, layer=LAYER_PRED, near=0.1, thickness=1):
    """cmt_render_boxes: the wire frame and heading mark of every valid row of ``boxes`` fp32 [M, >= 7] below
    ``count`` (None or a device int32) whose score (``scores`` fp32 [M], optional) is above ``score_thr``.  The colour
    is ``class_rgb[label]`` (``labels`` int32 [M], ``class_rgb`` int32 [ncls], both on the device) or ``rgb_default``.
    Row 0 lies on top."""
    g = RenderBoxesArgs()
    M, ld = strided_rows(boxes, "boxes", 7)
    if M >= MAX_ITEMS:
        raise ValueError(f"a call draws fewer than {MAX_ITEMS} boxes, got {M}")
    z_origin = float(z_origin)
    if z_origin not in (0.0, 0.5):
        raise ValueError(f"z_origin must be 0 (z is the bottom) or 0.5 (z is the gravity centre), got {z_origin}")
    _target(g.t, plane, views, near, layer)
    _count(count, "count")
    if labels is not None:
        labels = tensor(labels, "labels", torch.int32, (M,))
    if scores is not None:
        scores = tensor(scores, "scores", torch.float32, (M,))
    if class_rgb is not None:
        class_rgb = tensor(class_rgb, "class_rgb", torch.int32, (None,))
    score_thr = float(score_thr)
    if math.isnan(score_thr):
        raise ValueError("score_thr must not be NaN")
    thickness = _int_in(thickness, 1, 3, "thickness")
    rgb_default = _rgb(rgb_default, "rgb_default")
    _on_device(plane.device, boxes=boxes, count=count, labels=labels, scores=scores, class_rgb=class_rgb)
    L = render_lib()
    if M == 0:
        return plane
    g.M, g.ld, g.thickness, g.ncls = M, ld, thickness, 0 if class_rgb is None else int(class_rgb.shape[0])
    g.z_origin, g.score_thr, g.rgb_default = z_origin, score_thr, rgb_default
    g.boxes, g.count, g.labels, g.scores, g.class_rgb = _p(boxes), _p(count), _p(labels), _p(scores), _p(class_rgb)
    _check(L.cmt_render_boxes(ctypes.byref(g), _stream()), "cmt_render_boxes")
    return plane


def render_digits(plane, views, values, anchors, *, rgb=DIGIT_RGB, rank=None, scale=1, layer=LAYER_DIGITS, near=0.1,
                  planar=False):
    """cmt_render_digits: the decimal digits of ``values`` int32 [M] (negative: nothing) in the 5 x 7 font, the top
    left pixel of the first digit at the projected ``anchors`` fp32 [M, 3] (``planar``: [M, 2] pixel coordinates).
    ``rgb``: one colour or int32 [M]."""
    g = RenderDigitsArgs()
    values = tensor(values, "values", torch.int32, (None,))
    M = int(values.shape[0])
    anchors = tensor(anchors, "anchors", torch.float32, (M, 2 if planar else 3))
    if M >= MAX_ITEMS:
        raise ValueError(f"a call draws fewer than {MAX_ITEMS} numbers, got {M}")
    per_value = torch.is_tensor(rgb)
    if per_value:
        rgb = tensor(rgb, "rgb", torch.int32, (M,))
    else:
        g.rgb_one = _rgb(rgb, "rgb")
    if rank is not None:
        rank = tensor(rank, "rank", torch.int32, (M,))
    _target(g.t, plane, None if planar else views, near, layer)
    scale = _int_in(scale, 1, 4, "scale")
    _on_device(plane.device, values=values, anchors=anchors, rgb=rgb if per_value else None, rank=rank)
    L = render_lib()
    if M == 0:
        return plane
    g.M, g.planar, g.scale = M, int(bool(planar)), scale
    g.values, g.anchors, g.rgb, g.rank = _p(values), _p(anchors), _p(rgb) if per_value else None, _p(rank)
    _check(L.cmt_render_digits(ctypes.byref(g), _stream()), "cmt_render_digits")
    return plane


def render_resolve(plane, *, background=0x000000, src=None, out=None):
    """cmt_render_resolve -> uint8 [V, H, W, 3].  An empty pixel takes ``src``'s pixel (uint8 [V, H, W, 3]) when given,
    else ``background``.  ``out``: a tensor to write into; ``out is src`` resolves in place."""
    if not torch.is_tensor(plane) or plane.dtype != torch.int64 or plane.dim() != 3 or not plane.is_contiguous():
        raise ValueError("plane must be a contiguous int64 [V, H, W] tensor (new_plane)")
    V, H, W = _size(*plane.shape)
    background = _rgb(background, "background")
    if src is not None:
        src = tensor(src, "src", torch.uint8, (V, H, W, 3))
    if out is None:
        out = torch.empty((V, H, W, 3), dtype=torch.uint8, device=plane.device)
    else:
        out = tensor(out, "out", torch.uint8, (V, H, W, 3))
    _on_device(plane.device, src=src, out=out)
    g = RenderResolveArgs()
    g.V, g.H, g.W, g.background = V, H, W, background
    g.plane, g.src, g.out = _p(plane), _p(src), _p(out)
    _check(render_lib().cmt_render_resolve(ctypes.byref(g), _stream()), "cmt_render_resolve")
    return out
