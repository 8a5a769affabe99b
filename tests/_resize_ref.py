"""The contract of cmt_img_resize_prepare (include/cmt_hip.h) in numpy, shared by tests/test_resize_host.py and
tests/test_gpu_imgresize.py.  Not a test module.

``resize_u8`` is the 8-bit fixed-point bilinear resample in integers, ``resize_f64`` the float64 bilinear with
the same geometry (pixel centres, horizontal border taps zeroed, vertical indices clamped), ``reference`` the
whole call: resize, window (byte 0 outside the resized image), the two-step float32 normalisation of
tests/test_gpu_imgprep.py's ``_reference`` and the zero pad.
"""
import numpy as np

COEF = 2048   # coefficient scale, 11 bits


def axis_taps(S, R, horizontal):
    """(s0, s1, t) per resized index: clamped tap indices (int64) and the float32 fraction"""
    scale = np.float64(S) / np.float64(R)
    d = np.arange(R, dtype=np.float64)
    f = ((d + 0.5) * scale - 0.5).astype(np.float32)   # float64 multiply, float64 subtract, one rounding to float32
    s = np.floor(f)
    t = f - s
    assert s.dtype == np.float32 and t.dtype == np.float32
    s = s.astype(np.int64)
    if horizontal:
        lo, hi = s < 0, s >= S - 1
        s = np.where(lo, 0, np.where(hi, S - 1, s))
        t = np.where(lo | hi, np.float32(0), t).astype(np.float32)
    return np.clip(s, 0, S - 1), np.clip(s + 1, 0, S - 1), t


def axis_coefs(S, R, horizontal):
    """(s0, s1, c0, c1): tap indices and the integer coefficients of the two taps"""
    s0, s1, t = axis_taps(S, R, horizontal)
    c1 = np.rint(t * np.float32(COEF))
    c0 = np.rint((np.float32(1) - t) * np.float32(COEF))
    assert c0.dtype == np.float32 and c1.dtype == np.float32
    return s0, s1, c0.astype(np.int64), c1.astype(np.int64)


def resize_u8(src, Hr, Wr):
    """uint8 [..., Hs, Ws, C] -> uint8 [..., Hr, Wr, C]"""
    Hs, Ws = src.shape[-3:-1]
    x0, x1, a0, a1 = axis_coefs(Ws, Wr, True)
    y0, y1, b0, b1 = axis_coefs(Hs, Hr, False)
    s = src.astype(np.int64)
    rows = s[..., :, x0, :] * a0[:, None] + s[..., :, x1, :] * a1[:, None]     # [..., Hs, Wr, C]
    r0, r1 = rows[..., y0, :, :] >> 4, rows[..., y1, :, :] >> 4
    out = (((b0[:, None, None] * r0) >> 16) + ((b1[:, None, None] * r1) >> 16) + 2) >> 2
    assert out.min() >= 0 and out.max() <= 255
    return out.astype(np.uint8)


def resize_f64(src, Hr, Wr):
    """float64 bilinear with the same taps and the unrounded fractions"""
    Hs, Ws = src.shape[-3:-1]
    x0, x1, tx = axis_taps(Ws, Wr, True)
    y0, y1, ty = axis_taps(Hs, Hr, False)
    tx, ty = tx.astype(np.float64)[:, None], ty.astype(np.float64)[:, None, None]
    s = src.astype(np.float64)
    rows = s[..., :, x0, :] * (1.0 - tx) + s[..., :, x1, :] * tx
    return rows[..., y0, :, :] * (1.0 - ty) + rows[..., y1, :, :] * ty


def window_u8(img, win):
    """the (x0, y0, w, h) window of uint8 [n, H, W, 3], byte 0 outside the image"""
    x0, y0, w, h = win
    n, H, W, _ = img.shape
    crop = np.zeros((n, h, w, 3), np.uint8)
    ys, xs = np.arange(y0, y0 + h), np.arange(x0, x0 + w)
    yi, xi = (ys >= 0) & (ys < H), (xs >= 0) & (xs < W)
    if yi.any() and xi.any():
        crop[:, np.ix_(yi, xi)[0], np.ix_(yi, xi)[1]] = img[:, ys[yi]][:, :, xs[xi]]
    return crop


def normalise_pad(crop, Hp, Wp, mean, std, to_rgb):
    """uint8 [n, h, w, 3] -> float32 [n, 3, Hp, Wp]: (x.astype(f32) - mean32) * inv32, zeros in the pad"""
    n, h, w, _ = crop.shape
    if to_rgb:
        crop = crop[..., ::-1]
    mean32, std32 = np.asarray(mean, np.float32), np.asarray(std, np.float32)
    inv32 = (1.0 / std32.astype(np.float64)).astype(np.float32)
    f32 = (crop.astype(np.float32) - mean32) * inv32
    assert f32.dtype == np.float32
    out = np.zeros((n, 3, Hp, Wp), np.float32)
    out[:, :, :h, :w] = f32.transpose(0, 3, 1, 2)
    return out


def reference(src, resize_dims, win, Hp, Wp, mean, std, to_rgb):
    """the whole contract: ``resize_dims`` = (Wr, Hr), ``win`` = (x0, y0, w, h) in resized pixels"""
    Wr, Hr = resize_dims
    return normalise_pad(window_u8(resize_u8(src, Hr, Wr), win), Hp, Wp, mean, std, to_rgb)
