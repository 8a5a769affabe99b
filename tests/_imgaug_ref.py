"""The contracts of cmt_img_augment, cmt_grid_mask and cmt_img_paste (include/cmt_hip.h) in numpy, shared by
tests/test_imgaug_host.py and tests/test_gpu_imgaug.py.  Not a test module.

The resize bytes and the normalisation are tests/_resize_ref.py's.  ``flipped_crop`` is the tap array T,
``warp_sums`` the 1/32-pixel bilinear of the rotation as exact integers (1024 * val), ``grid_mask`` the GridMask
predicate, ``augment`` the whole of cmt_img_augment, ``paste`` the whole of cmt_img_paste.
"""
import numpy as np

import _resize_ref as R

IDENTITY = (1.0, 0.0, 0.0, 0.0, 1.0, 0.0)


def flipped_crop(img, Hr, Wr, x0, y0, w, h, flip=False, zero=False):
    """T of the contract for one uint8 [Hs, Ws, 3] frame: int64 [h, w, 3]"""
    crop = R.window_u8(R.resize_u8(img[None], Hr, Wr), (x0, y0, w, h))[0]
    if flip:
        crop = crop[:, ::-1]
    T = crop.astype(np.int64)
    return T * 0 if zero else T


def warp_coords(w, h, iM):
    """(ix, fx, iy, fy), each int64 [h, w]"""
    iM = [np.float64(v) for v in iM]
    x, y = np.arange(w, dtype=np.float64), np.arange(h, dtype=np.float64)
    AX = np.rint(iM[0] * x * 1024.0).astype(np.int64)
    AY = np.rint(iM[3] * x * 1024.0).astype(np.int64)
    BX = np.rint((iM[1] * y + iM[2]) * 1024.0).astype(np.int64) + 16
    BY = np.rint((iM[4] * y + iM[5]) * 1024.0).astype(np.int64) + 16
    X, Y = (BX[:, None] + AX[None, :]) >> 5, (BY[:, None] + AY[None, :]) >> 5
    return X >> 5, X & 31, Y >> 5, Y & 31


def warp_sums(T, iM):
    """1024 * val of the contract: int64 [h, w, 3] from the tap array T [h, w, 3]"""
    h, w = T.shape[:2]
    ix, fx, iy, fy = warp_coords(w, h, iM)

    def tap(ty, tx):
        ok = (ty >= 0) & (ty < h) & (tx >= 0) & (tx < w)
        return np.where(ok[..., None], T[np.clip(ty, 0, h - 1), np.clip(tx, 0, w - 1)], 0)

    fx, fy = fx[..., None], fy[..., None]
    return ((32 - fx) * (32 - fy) * tap(iy, ix) + fx * (32 - fy) * tap(iy, ix + 1) +
            (32 - fx) * fy * tap(iy + 1, ix) + fx * fy * tap(iy + 1, ix + 1))


def grid_mask(Hp, Wp, d, l, st_h, st_w, use_h, use_w, mode):
    """m(y, x) of the contract as float32 [Hp, Wp]"""
    hh, ww = int(1.5 * Hp), int(1.5 * Wp)
    Y = np.arange(Hp) + (hh - Hp) // 2
    X = np.arange(Wp) + (ww - Wp) // 2
    rowband = (Y >= st_h) & ((Y - st_h) // d < hh // d) & ((Y - st_h) % d < l)
    colband = (X >= st_w) & ((X - st_w) // d < ww // d) & ((X - st_w) % d < l)
    base = ~((bool(use_h) & rowband)[:, None] | (bool(use_w) & colband)[None, :])
    return (~base if mode == 1 else base).astype(np.float32)


def augment(src, images, w, h, Hp, Wp, mean, std, to_rgb, grid=None):
    """The whole of cmt_img_augment.  ``images``: one dict(Hr, Wr, x0, y0, flip, zero, iM) per frame of uint8 ``src``
    [N, Hs, Ws, 3]; ``grid``: None or grid_mask's keyword arguments -> float32 [N, 3, Hp, Wp]"""
    mean32, std32 = np.asarray(mean, np.float32), np.asarray(std, np.float32)
    inv32 = (1.0 / std32.astype(np.float64)).astype(np.float32)
    out = np.zeros((len(src), 3, Hp, Wp), np.float32)
    for n, im in enumerate(images):
        T = flipped_crop(src[n], im["Hr"], im["Wr"], im["x0"], im["y0"], w, h, im.get("flip", False), im.get("zero", False))
        sums = warp_sums(T, im.get("iM", IDENTITY))
        assert sums.min() >= 0 and sums.max() <= 255 * 1024
        val = sums.astype(np.float32) / np.float32(1024)   # exact
        if to_rgb:
            val = val[..., ::-1]
        f32 = (val - mean32) * inv32
        assert f32.dtype == np.float32
        out[n, :, :h, :w] = f32.transpose(2, 0, 1)
    if grid is not None:
        out = out * grid_mask(Hp, Wp, **grid)[None, None]
        assert out.dtype == np.float32
    return out


def paste(frames, plan, patches, m):
    """The whole of cmt_img_paste on a copy of uint8 ``frames`` [N, Hs, Ws, 3]: ``plan`` one [k, 5] integer array
    per camera, ``patches`` uint8 HWC arrays, ``m`` the mixup rate (< 0: plain paste)"""
    out = frames.copy()
    om = 1.0 - np.float64(m)
    for n, rects in enumerate(plan):
        for x0, y0, x1, y1, crop in np.asarray(rects).reshape(-1, 5).tolist():
            if x1 <= x0 or y1 <= y0:
                continue
            reg = out[n, y0:y1, x0:x1]
            v = reg.astype(np.float64)
            if crop < 0:
                if m >= 0:
                    reg[...] = np.trunc(v * om + v * np.float64(m)).astype(np.uint8)
                continue
            p = np.asarray(patches[crop])
            if p.size == 0:
                continue
            c = R.resize_u8(p[None], y1 - y0, x1 - x0)[0]
            reg[...] = c if m < 0 else np.trunc(v * om + c.astype(np.float64) * np.float64(m)).astype(np.uint8)
    return out
