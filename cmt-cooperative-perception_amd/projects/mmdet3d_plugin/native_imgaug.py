"""The training side of the image pipeline on the device: cmt_img_augment, cmt_grid_mask and cmt_img_paste
(include/cmt_hip.h) and the host helpers that restate the reference's choices around them.

``paste_images`` is the pixel part of ``unified_sample`` (``sample_2d=True``) in place on the uint8 frames, with
``paste_plan`` the rectangles it pastes into; ``augment_images`` is ResizeCropFlipImage[Coop](training=True),
NormalizeMultiviewImage and PadMultiViewImage in one launch, optionally with GridMask and ModalMask3D's zeroed
images, from the per-image draws of ``sample_images_plan``; ``grid_mask_`` applies the mask to a prepared batch.
``train_image_lidar2img`` and ``sample_bev_image_augmentation`` give the matrices and box parameters that belong
to the augmented frames.  The database sampler, its files and ``modify_points`` stay with the caller.

Like native_aug.py: argument checks raise ValueError before the device check, tensors must live on a HIP device,
there is no CPU fallback and no wrapper synchronises with the host.  Random draws come from the ``rng`` the
caller passes (a numpy RandomState, or the ``numpy.random`` module for the reference's global stream) in the
reference's order, so that with the reference's seed the numbers are the reference's.
"""
import ctypes
import math

import numpy as np
import torch

from . import native as N
from .native import _check, _p, _stream, lib
from .native_img import IMG_MEAN, IMG_STD, _f32, _pipeline_steps, norm_constants, resize_crop_plan

__all__ = ["MAX_IMAGES", "MAX_PASTE_RECTS", "sample_image_augmentation", "sample_images_plan", "warp_inverse",
           "train_image_lidar2img", "paste_plan", "paste_images", "augment_images", "sample_grid_mask", "grid_mask_",
           "sample_modal_mask", "sample_bev_image_augmentation", "image_train_plan_from_config"]

MAX_IMAGES = N.IMG_AUG_MAX
MAX_PASTE_RECTS = N.PASTE_MAX_RECTS
# GridMask as the reference's detectors build it (cmt.py: GridMask(True, True, rotate=1, offset=False, ratio=0.5,
# mode=1, prob=0.7))
DETECTOR_GRID_MASK = dict(use_h=True, use_w=True, rotate=1, offset=False, ratio=0.5, mode=1, prob=0.7)


# ---- ResizeCropFlipImage[Coop] -----------------------------------------------------------------------------------
def sample_image_augmentation(conf, rng, training=True):
    """ResizeCropFlipImage[Coop]._sample_augmentation for ``conf`` (the config's ida_aug_conf) ->
    dict(resize, resize_dims=(newW, newH), crop=(x0, y0, x1, y1), flip, rotate) with rotate in degrees.  Training
    draws, in this order, ``uniform(*resize_lim)``, ``uniform(*bot_pct_lim)``, ``uniform(0, max(0, newW - fW))``,
    ``choice([0, 1])`` only if ``rand_flip``, ``uniform(*rot_lim)``; the int() truncations are the reference's.
    Test mode draws nothing and returns resize_crop_plan's values."""
    H, W = int(conf["H"]), int(conf["W"])
    fH, fW = (int(v) for v in conf["final_dim"])
    if min(H, W, fH, fW) <= 0:
        raise ValueError(f"positive sizes required, got H, W {(H, W)}, final_dim {(fH, fW)}")
    if not training:
        resize, dims, crop = resize_crop_plan((H, W), (fH, fW), conf.get("bot_pct_lim", (0.0, 0.0)))
        return dict(resize=resize, resize_dims=dims, crop=crop, flip=False, rotate=0)
    resize = float(rng.uniform(*conf["resize_lim"]))
    new_w, new_h = int(W * resize), int(H * resize)
    crop_h = int((1 - float(rng.uniform(*conf["bot_pct_lim"]))) * new_h) - fH
    crop_w = int(rng.uniform(0, max(0, new_w - fW)))
    flip = False
    if conf["rand_flip"] and rng.choice([0, 1]):
        flip = True
    rotate = float(rng.uniform(*conf["rot_lim"]))
    return dict(resize=resize, resize_dims=(new_w, new_h), crop=(crop_w, crop_h, crop_w + fW, crop_h + fH), flip=flip,
                rotate=rotate)


def sample_images_plan(conf, rng, n_images, pic_wise=False, training=True):
    """The loop of ResizeCropFlipImage[Coop].__call__ over one agent's ``n_images`` frames -> a list of
    sample_image_augmentation dicts: one draw in front of the loop and, with ``pic_wise``, a fresh one per image
    (the first draw is then consumed and dropped, as in the reference).  The coop sample calls this for the
    infrastructure images first, then for the vehicle's."""
    n = int(n_images)
    if n < 0:
        raise ValueError(f"n_images must not be negative, got {n_images}")
    aug = sample_image_augmentation(conf, rng, training)
    plans = []
    for _ in range(n):
        if pic_wise:
            aug = sample_image_augmentation(conf, rng, training)
        plans.append(dict(aug))
    return plans


def warp_inverse(w, h, rotate_deg):
    """The six float64 entries iM of cmt_img_augment for a rotation by ``rotate_deg`` degrees about (w / 2, h / 2):
    cv2.getRotationMatrix2D((w / 2, h / 2), angle, 1) followed by cv2.warpAffine's inversion (include/cmt_hip.h
    writes the sequence down; restated from memory, not verified against a real OpenCV).  ``rotate_deg == 0``
    returns the exact identity, which makes the rotation an exact pass-through."""
    ang = float(rotate_deg)
    if not math.isfinite(ang):
        raise ValueError(f"rotate must be finite, got {rotate_deg!r}")
    if ang == 0.0:
        return [1.0, 0.0, 0.0, 0.0, 1.0, 0.0]
    cx, cy = float(w) / 2, float(h) / 2
    rad = ang * (math.pi / 180.0)
    al, be = math.cos(rad), math.sin(rad)
    M = [al, be, (1 - al) * cx - be * cy, -be, al, be * cx + (1 - al) * cy]
    D = M[0] * M[4] - M[1] * M[3]
    D = 1.0 / D if D != 0 else 0.0
    A11, A22 = M[4] * D, M[0] * D
    M[0] = A11
    M[1] *= -D
    M[3] *= -D
    M[4] = A22
    b1 = -M[0] * M[2] - M[1] * M[5]
    b2 = -M[3] * M[2] - M[4] * M[5]
    M[2], M[5] = b1, b2
    return M


def train_image_lidar2img(cam_intrinsic, lidar2cam, resize, crop, flip, rotate):
    """lidar2img of a frame after ResizeCropFlipImage[Coop](training=True): ``post_rot`` / ``post_tran`` of
    ``_img_transform`` (scale by ``resize``, shift by the crop origin, mirror about the crop's width, rotate by
    ``rotate`` degrees about the crop's centre), then rows 0-1 of the intrinsic become post_rot @ K[:2, :3] and its
    principal point moves by post_tran, then intrinsic @ lidar2cam.  Host float64 throughout; stated deviation: the
    reference builds post_rot and post_tran in float32 torch.  ``cam_intrinsic`` is 3 x 3 or 4 x 4, ``lidar2cam``
    4 x 4; the inputs are not modified."""
    K = np.array(cam_intrinsic, dtype=np.float64)
    E = np.array(lidar2cam, dtype=np.float64)
    if K.shape == (3, 3):
        K4 = np.eye(4)
        K4[:3, :3] = K
        K = K4
    if K.shape != (4, 4) or E.shape != (4, 4):
        raise ValueError(f"cam_intrinsic must be 3 x 3 or 4 x 4 and lidar2cam 4 x 4, got {K.shape} and {E.shape}")
    x0, y0, x1, y1 = (float(v) for v in crop)
    post_rot = np.eye(2) * float(resize)
    post_tran = -np.array([x0, y0])
    if flip:
        A = np.array([[-1.0, 0.0], [0.0, 1.0]])
        post_rot = A @ post_rot
        post_tran = A @ post_tran + np.array([x1 - x0, 0.0])
    h = float(rotate) / 180 * np.pi
    A = np.array([[np.cos(h), np.sin(h)], [-np.sin(h), np.cos(h)]])
    b = np.array([x1 - x0, y1 - y0]) / 2
    b = A @ (-b) + b
    post_rot = A @ post_rot
    post_tran = A @ post_tran + b
    K[:2, :3] = post_rot @ K[:2, :3]
    K[:2, 2] = post_tran + K[:2, 2]
    return K @ E


# ---- unified_sample's image pasting ------------------------------------------------------------------------------
def paste_plan(corners, lidar2img, frame_hw, n_sampled, by_depth=True):
    """The rectangles ``unified_sample`` pastes into, per camera, in float64 numpy.  ``corners`` is [n, 8, 3] (the
    ground truth's corners followed by the ``n_sampled`` sampled boxes'), ``lidar2img`` a stack of 4 x 4 matrices,
    ``frame_hw = (H, W)`` -> a list, per camera, of int32 arrays [k, 5] with rows (x0, y0, x1, y1, crop) in paste
    order; crop is -1 for a ground-truth box and the sampled box's index otherwise.

    As the reference: a box counts where all eight corners have depth > 0; min / max of the projected corners are
    truncated by ``astype(int)``, x clipped to [0, W - 1] and y to [0, H - 1]; a box stays if both sides are > 1;
    ``by_depth`` orders by the mean corner depth, far first.  Stated deviations: the order is a STABLE ascending
    sort reversed (numpy's default argsort is not stable, so the reference's order among equal depths is not
    defined); ``n_sampled == 0`` means no sampled box (the reference's ``is_raw[-0:] = 0`` would clear every
    flag).  Non-finite projections raise ValueError."""
    c = np.asarray(corners, dtype=np.float64)
    L = np.asarray(lidar2img, dtype=np.float64)
    if c.ndim != 3 or c.shape[1:] != (8, 3):
        raise ValueError(f"corners must be [n, 8, 3], got {c.shape}")
    if L.ndim != 3 or L.shape[1:] != (4, 4):
        raise ValueError(f"lidar2img must be [cams, 4, 4], got {L.shape}")
    H, W = (int(v) for v in frame_hw)
    ns = int(n_sampled)
    if H <= 0 or W <= 0 or ns < 0 or ns > len(c):
        raise ValueError(f"frame_hw must be positive and 0 <= n_sampled <= {len(c)}, got {frame_hw}, {n_sampled}")
    raw_num = len(c) - ns
    c4 = np.concatenate([c, np.ones_like(c[..., :1])], -1)
    out = []
    for mat in L:
        rects = np.zeros((0, 5), np.int32)
        with np.errstate(invalid="ignore"):
            coord = c4 @ mat.T
        if not np.isfinite(coord).all():
            raise ValueError("non-finite projection of a box corner")
        depth = coord[..., 2]
        mask = (depth > 0).all(axis=-1)
        idx = mask.nonzero()[0]
        if len(idx):
            xy = coord[mask][..., :2] / coord[mask][..., 2, None]
            if not np.isfinite(xy).all():
                raise ValueError("non-finite projection of a box corner")
            mean_depth = depth.mean(1)[mask]
            box = np.concatenate([xy.min(axis=-2), xy.max(axis=-2)], axis=-1)
            box = np.clip(box, -2.0 ** 31, 2.0 ** 31).astype(np.int64)   # truncation; the frame clip follows
            box[:, 0::2] = np.clip(box[:, 0::2], 0, W - 1)
            box[:, 1::2] = np.clip(box[:, 1::2], 0, H - 1)
            keep = ((box[:, 2:] - box[:, :2]) > 1).all(axis=-1)
            idx, box, mean_depth = idx[keep], box[keep], mean_depth[keep]
            order = np.argsort(mean_depth, kind="stable")[::-1] if by_depth else np.arange(len(idx))
            idx, box = idx[order], box[order]
            crop = np.where(idx < raw_num, -1, idx - raw_num)
            rects = np.concatenate([box, crop[:, None]], axis=1).astype(np.int32)
        out.append(rects)
    return out


def paste_images(frames, plan, patches, mixup_rate=-1, modify_points=False):
    """cmt_img_paste: the pixel part of ``unified_sample`` in place on uint8 ``frames`` [N, Hs, Ws, 3] (contiguous,
    on the device).  ``plan`` is paste_plan's list (one [k, 5] array per camera, k <= MAX_PASTE_RECTS),
    ``patches`` the sampled objects' image crops, uint8 HWC arrays (an empty one is skipped, as in the reference);
    they are packed into one buffer and uploaded with the tables.  ``mixup_rate < 0`` pastes, otherwise the pixel
    becomes trunc(old * (1 - rate) + new * rate) in float64.  Returns ``frames``."""
    if modify_points:
        raise NotImplementedError("modify_points=True is not built (no reference config sets it)")
    if not torch.is_tensor(frames) or frames.dtype != torch.uint8:
        raise ValueError(f"frames must be a uint8 tensor, got {frames.dtype if torch.is_tensor(frames) else type(frames)}")
    if frames.dim() != 4 or frames.shape[3] != 3 or min(frames.shape) <= 0:
        raise ValueError(f"frames must be a non-empty [N, H, W, 3] tensor, got {tuple(frames.shape)}")
    if not frames.is_contiguous():
        raise ValueError("frames must be contiguous (interleaved HWC rows)")
    n, Hs, Ws = (int(s) for s in frames.shape[:3])
    if n > MAX_IMAGES or max(Hs, Ws) >= 2 ** 30:
        raise ValueError(f"at most {MAX_IMAGES} frames below 2^30 pixels a side, got {tuple(frames.shape)}")
    m = float(mixup_rate)
    if math.isnan(m) or m > 1:
        raise ValueError(f"mixup_rate must be at most 1 (negative: plain paste), got {mixup_rate!r}")
    if len(plan) != n:
        raise ValueError(f"plan has {len(plan)} cameras, frames {n}")
    metas, chunks, off = [], [], 0
    for i, pt in enumerate(patches):
        pt = pt.cpu().numpy() if torch.is_tensor(pt) else np.asarray(pt)
        if pt.size == 0:
            metas.append((off, 0, 0))
            continue
        if pt.dtype != np.uint8 or pt.ndim != 3 or pt.shape[2] != 3 or max(pt.shape) >= 2 ** 15:
            raise ValueError(f"patch {i} must be uint8 [h, w, 3] below 2^15 a side, got {pt.dtype} {pt.shape}")
        metas.append((off, pt.shape[0], pt.shape[1]))
        chunks.append(np.ascontiguousarray(pt).reshape(-1))
        off += pt.size
    rects = np.zeros((n, MAX_PASTE_RECTS, 5), np.int32)
    counts = []
    for i, r in enumerate(plan):
        r = np.asarray(r)
        if r.size == 0:
            counts.append(0)
            continue
        if r.ndim != 2 or r.shape[1] != 5 or not np.issubdtype(r.dtype, np.integer):
            raise ValueError(f"plan[{i}] must be an integer [k, 5] array, got {r.dtype} {r.shape}")
        if len(r) > MAX_PASTE_RECTS:
            raise ValueError(f"plan[{i}] has {len(r)} rectangles, at most {MAX_PASTE_RECTS}")
        r = r.astype(np.int64)
        if ((r[:, 0] < 0) | (r[:, 1] < 0) | (r[:, 0] > r[:, 2]) | (r[:, 1] > r[:, 3]) | (r[:, 2] > Ws) | (r[:, 3] > Hs)).any():
            raise ValueError(f"plan[{i}]: rectangles must satisfy 0 <= x0 <= x1 <= {Ws} and 0 <= y0 <= y1 <= {Hs}")
        if ((r[:, 4] < -1) | (r[:, 4] >= len(metas))).any():
            raise ValueError(f"plan[{i}]: crop must be -1 or an index into the {len(metas)} patches")
        rects[i, :len(r)] = r
        counts.append(len(r))
    if not frames.is_cuda:
        raise ValueError("frames must live on a HIP device (no CPU path)")
    if sum(counts) == 0:
        return frames
    table = np.zeros(max(len(metas), 1), dtype=np.dtype([("offset", np.int64), ("hc", np.int32), ("wc", np.int32)]))
    for i, (o, hc, wc) in enumerate(metas):
        table[i] = (o, hc, wc)
    packed = np.concatenate(chunks) if chunks else np.zeros(1, np.uint8)
    dev = frames.device
    rects_dev = torch.from_numpy(rects.reshape(-1)).to(dev)
    table_dev = torch.from_numpy(table.view(np.uint8)).to(dev)
    bytes_dev = torch.from_numpy(packed).to(dev)
    a = N.ImgPasteArgs()
    a.N, a.Hs, a.Ws, a.n_patches = n, Hs, Ws, len(metas)
    for i, k in enumerate(counts):
        a.count[i] = k
    a.mixup = m
    a.rects, a.patches = ctypes.c_void_p(rects.ctypes.data), ctypes.c_void_p(table.ctypes.data)
    a.rects_dev, a.patches_dev, a.patch_bytes = _p(rects_dev), _p(table_dev), _p(bytes_dev)
    a.patch_bytes_size = off
    a.frames = _p(frames)
    _check(lib().cmt_img_paste(ctypes.byref(a), _stream()), "cmt_img_paste")
    return frames


# ---- GridMask ----------------------------------------------------------------------------------------------------
def _grid_fields(g, grid_mask):
    keys = {"d", "l", "st_h", "st_w", "use_h", "use_w", "mode"}
    if not isinstance(grid_mask, dict) or set(grid_mask) != keys:
        raise ValueError(f"grid_mask must be a dict with the keys {sorted(keys)}")
    d, l, st_h, st_w = (int(grid_mask[k]) for k in ("d", "l", "st_h", "st_w"))
    if not (2 <= d < 2 ** 30 and 1 <= l < d and 0 <= st_h < d and 0 <= st_w < d):
        raise ValueError(f"grid_mask needs 2 <= d < 2^30, 1 <= l < d and 0 <= st_h, st_w < d, got {grid_mask}")
    if int(grid_mask["mode"]) not in (0, 1):
        raise ValueError(f"grid_mask mode must be 0 or 1, got {grid_mask['mode']!r}")
    g.d, g.l, g.st_h, g.st_w = d, l, st_h, st_w
    g.use_h, g.use_w, g.mode = int(bool(grid_mask["use_h"])), int(bool(grid_mask["use_w"])), int(grid_mask["mode"])


def sample_grid_mask(conf, h, rng, training=True):
    """GridMask.forward's draws for a batch of height ``h`` -> the ``grid_mask`` dict of augment_images and
    grid_mask_, or None where the reference returns its input: ``rand() > prob`` is drawn first (also outside
    training, as there), then ``d = randint(2, h)``, ``st_h = randint(d)``, ``st_w = randint(d)`` and
    ``randint(rotate)``; ``l = min(max(int(d * ratio + 0.5), 1), d - 1)``.  ``conf`` holds the constructor's
    arguments (use_h, use_w, rotate, offset, ratio, mode, prob); ``rotate != 1`` and ``offset`` are not built."""
    if int(conf.get("rotate", 1)) != 1:
        raise NotImplementedError("GridMask with rotate != 1 (a rotated mask) is not built")
    if conf.get("offset", False):
        raise NotImplementedError("GridMask(offset=True) is not built")
    if rng.rand() > conf.get("prob", 1.0) or not training:
        return None
    d = int(rng.randint(2, int(h)))
    l = min(max(int(d * conf.get("ratio", 0.5) + 0.5), 1), d - 1)
    st_h = int(rng.randint(d))
    st_w = int(rng.randint(d))
    rng.randint(1)   # r = randint(rotate): always 0, the draw is still made
    return dict(d=d, l=l, st_h=st_h, st_w=st_w, use_h=bool(conf["use_h"]), use_w=bool(conf["use_w"]),
                mode=int(conf.get("mode", 0)))


def grid_mask_(x, grid_mask):
    """cmt_grid_mask: the mask of ``grid_mask`` (sample_grid_mask's dict) applied in place to fp32 ``x``
    [n, c, h, w] (contiguous, on the device); every element is multiplied by 0.f or 1.f.  Returns ``x``."""
    if not torch.is_tensor(x) or x.dtype != torch.float32 or x.dim() != 4 or min(x.shape) <= 0:
        raise ValueError("x must be a non-empty fp32 [n, c, h, w] tensor")
    if not x.is_contiguous():
        raise ValueError("x must be contiguous")
    n, c, h, w = (int(s) for s in x.shape)
    if max(h, w) >= 2 ** 30 or n * c * h * ((w + 3) // 4) >= 2 ** 31:
        raise ValueError("x beyond the kernel's index range")
    a = N.GridMaskArgs()
    _grid_fields(a.grid, grid_mask)
    if not x.is_cuda:
        raise ValueError("x must live on a HIP device (no CPU path)")
    a.planes, a.h, a.w, a.x = n * c, h, w, _p(x)
    _check(lib().cmt_grid_mask(ctypes.byref(a), _stream()), "cmt_grid_mask")
    return x


# ---- ResizeCropFlipImage + Normalize + Pad (+ GridMask, ModalMask3D) ----------------------------------------------
def augment_images(frames, plans, mean=IMG_MEAN, std=IMG_STD, to_rgb=False, size_divisor=32, size=None, grid_mask=None,
                   zero=False, out=None):
    """cmt_img_augment: uint8 ``frames`` [N, Hs, Ws, 3] -> fp32 [N, 3, Hp, Wp] in one launch.  ``plans`` has one
    dict per frame with ``resize_dims = (Wr, Hr)``, ``crop = (x0, y0, x1, y1)`` in resized pixels, ``flip`` and
    ``rotate`` (degrees), as sample_images_plan returns them; the crops share one size.  (Hp, Wp) is that size
    rounded up to ``size_divisor``, or the explicit ``size``.  ``grid_mask`` (sample_grid_mask's dict, or None)
    masks every element, the pad included; ``zero`` (a bool, or one per frame) is ModalMask3D's ``0. * img``."""
    if not torch.is_tensor(frames) or frames.dtype != torch.uint8:
        raise ValueError(f"frames must be a uint8 tensor, got {frames.dtype if torch.is_tensor(frames) else type(frames)}")
    if frames.dim() != 4 or frames.shape[3] != 3 or min(frames.shape) <= 0:
        raise ValueError(f"frames must be a non-empty [N, H, W, 3] tensor, got {tuple(frames.shape)}")
    if not frames.is_contiguous():
        raise ValueError("frames must be contiguous (interleaved HWC rows)")
    n, Hs, Ws = (int(s) for s in frames.shape[:3])
    if n > MAX_IMAGES:
        raise ValueError(f"at most {MAX_IMAGES} frames per call, got {n}")
    if max(Hs, Ws) >= 2 ** 30:
        raise ValueError("frames beyond 2^30 pixels a side")
    if len(plans) != n:
        raise ValueError(f"{len(plans)} plans for {n} frames")
    zeros = [bool(zero)] * n if isinstance(zero, (bool, int)) else [bool(z) for z in zero]
    if len(zeros) != n:
        raise ValueError(f"zero must be a bool or one per frame, got {len(zeros)} for {n} frames")
    a = N.ImgAugmentArgs()
    w = h = None
    for i, pl in enumerate(plans):
        Wr, Hr = (int(v) for v in pl["resize_dims"])
        x0, y0, x1, y1 = (int(v) for v in pl["crop"])
        if Wr <= 0 or Hr <= 0 or max(Wr, Hr) >= 2 ** 30:
            raise ValueError(f"plans[{i}]: resize_dims must be positive and below 2^30, got {(Wr, Hr)}")
        if x1 - x0 <= 0 or y1 - y0 <= 0:
            raise ValueError(f"plans[{i}]: empty crop {(x0, y0, x1, y1)}")
        if w is None:
            w, h = x1 - x0, y1 - y0
        elif (w, h) != (x1 - x0, y1 - y0):
            raise ValueError(f"plans[{i}]: the crop size {(x1 - x0, y1 - y0)} differs from the first frame's {(w, h)}")
        if max(abs(x0), abs(y0), w, h) >= 2 ** 30:
            raise ValueError(f"plans[{i}]: crop beyond the kernel's index range")
        iM = warp_inverse(w, h, pl.get("rotate", 0))
        if not all(math.isfinite(v) and abs(v) < 2 ** 20 for v in iM):
            raise ValueError(f"plans[{i}]: the inverse map {iM} is not finite and below 2^20")
        im = a.img[i]
        im.Hr, im.Wr, im.x0, im.y0, im.flip, im.zero = Hr, Wr, x0, y0, int(bool(pl.get("flip", False))), int(zeros[i])
        im.iM[:] = iM
    if size is not None:
        Hp, Wp = (int(v) for v in size)
        if Hp < h or Wp < w:
            raise ValueError(f"size {(Hp, Wp)} below the crop's {(h, w)}")
    else:
        d = int(size_divisor)
        if d <= 0:
            raise ValueError(f"size_divisor must be positive, got {size_divisor}")
        Hp, Wp = (h + d - 1) // d * d, (w + d - 1) // d * d
    if max(Hp, Wp) >= 2 ** 30 or Hp * ((Wp + 3) // 4) >= 2 ** 31:
        raise ValueError("output size beyond the kernel's index range")
    mean32, inv32 = norm_constants(mean, std)
    if grid_mask is not None:
        _grid_fields(a.grid, grid_mask)
    if not frames.is_cuda:
        raise ValueError("frames must live on a HIP device (no CPU path)")
    if out is not None:
        _f32("out", out, (n, 3, Hp, Wp))
        if out.device != frames.device:
            raise ValueError("out must live on the frames' device")
    Y = out if out is not None else torch.empty((n, 3, Hp, Wp), dtype=torch.float32, device=frames.device)
    a.N, a.Hs, a.Ws, a.to_rgb = n, Hs, Ws, int(bool(to_rgb))
    a.w, a.h, a.Hp, a.Wp = w, h, Hp, Wp
    for c in range(3):
        a.mean[c], a.inv_std[c] = float(mean32[c]), float(inv32[c])
    a.src, a.dst = _p(frames), _p(Y)
    _check(lib().cmt_img_augment(ctypes.byref(a), _stream()), "cmt_img_augment")
    return Y


# ---- ModalMask3D, GlobalRotScaleTransImage[Coop] ------------------------------------------------------------------
def sample_modal_mask(rng):
    """ModalMask3D(mode='train'): one ``rand()``; > 0.75 zeroes the images ('image'), else > 0.5 the points
    ('points'), else nothing (None)"""
    seed = rng.rand()
    if seed > 0.75:
        return "image"
    if seed > 0.5:
        return "points"
    return None


def sample_bev_image_augmentation(step, rng):
    """GlobalRotScaleTransImage[Coop]'s draws for ``step`` (image_train_plan_from_config's ``bev_image_step``), in
    its order: ``uniform(*rot_range)``, ``uniform(*scale_ratio_range)``, ``rand() < flip_dx_ratio``,
    ``rand() < flip_dy_ratio`` -> (params, box_params), two dicts of the form native_aug.augment_lidar2img and
    native_aug.augment_boxes take: ``params`` for the lidar2img / lidar2cam matrices, ``box_params`` for the
    annotations.  They differ only under ``reverse_angle``, which negates the boxes' angle.  A flip of x
    (``dx``) is ``flip_v``, a flip of y (``dy``) ``flip_h``; there is no translation."""
    angle = float(rng.uniform(*step["rot_range"]))
    scale = float(rng.uniform(*step["scale_ratio_range"]))
    flip_v = bool(rng.rand() < step.get("flip_dx_ratio", 0.0))
    flip_h = bool(rng.rand() < step.get("flip_dy_ratio", 0.0))
    params = dict(angle=angle, scale=scale, trans=None, flip_h=flip_h, flip_v=flip_v)
    box_params = dict(params, angle=-angle) if step.get("reverse_angle", False) else dict(params)
    return params, box_params


_SAMPLERS = ("UnifiedObjectSample", "UnifiedObjectSampleCoop")
_BEV_IMAGE = ("GlobalRotScaleTransImage", "GlobalRotScaleTransImageCoop")


def image_train_plan_from_config(cfg):
    """The training-side image pipeline of a config dict (config.load_config): ``data.train`` (through
    CBGSDataset's ``dataset``), its ResizeCropFlipImage[Coop], NormalizeMultiviewImage[Coop], PadMultiViewImage[Coop],
    UnifiedObjectSample[Coop], ModalMask3D and GlobalRotScaleTransImage[Coop] steps, and ``model.use_grid_mask`` (for the
    coop detector, its ``vehicle_model`` / ``infrastructure_model``) ->
    dict(data_aug_conf, pic_wise, mean, std, to_rgb, size_divisor, image_paste, mixup_rate, paste_by_depth,
    modal_mask, bev_image_step, grid_mask); None for a pipeline without the resize step (LiDAR only).

    ``modal_mask`` is 'train' (draw with sample_modal_mask), 'image' / 'points' (ModalMask3D in test mode) or None;
    ``bev_image_step`` the step's dict(rot_range, scale_ratio_range, reverse_angle, flip_dx_ratio, flip_dy_ratio) or
    None; ``grid_mask`` the constructor arguments the reference's detectors use, or None."""
    train = cfg["data"]["train"]
    while isinstance(train, dict) and "pipeline" not in train and "dataset" in train:
        train = train["dataset"]   # CBGSDataset and other wrappers
    steps = list(_pipeline_steps(train["pipeline"]))

    def find(kinds):
        hits = [st for st in steps if st.get("type") in kinds]
        return hits[0] if hits else None

    rcf = find(("ResizeCropFlipImage", "ResizeCropFlipImageCoop"))
    if rcf is None:
        return None
    if not rcf.get("training", True):
        raise ValueError("the train pipeline's ResizeCropFlipImage step has training=False")
    norm = find(("NormalizeMultiviewImage", "NormalizeMultiviewImageCoop"))
    pad = find(("PadMultiViewImage", "PadMultiViewImageCoop"))
    if norm is None or pad is None:
        raise ValueError("the train pipeline resizes images but has no NormalizeMultiviewImage / PadMultiViewImage step")
    if pad.get("size_divisor") is None:
        raise ValueError("PadMultiViewImage with a fixed size is not supported, only size_divisor")
    plan = dict(data_aug_conf=dict(rcf["data_aug_conf"]), pic_wise=bool(rcf.get("pic_wise", False)),
                mean=tuple(norm["mean"]), std=tuple(norm["std"]),
                to_rgb=bool(norm.get("to_rgb", True)), size_divisor=int(pad["size_divisor"]), image_paste=False,
                mixup_rate=-1.0, paste_by_depth=True, modal_mask=None, bev_image_step=None, grid_mask=None)
    smp = find(_SAMPLERS)
    if smp is not None and smp.get("sample_2d", False):
        if smp.get("modify_points", False):
            raise NotImplementedError("UnifiedObjectSample(modify_points=True) is not built")
        plan.update(image_paste=True, mixup_rate=float(smp.get("mixup_rate", -1)),
                    paste_by_depth="depth" in smp.get("sample_method", "depth"))
    mm = find(("ModalMask3D",))
    if mm is not None:
        plan["modal_mask"] = "train" if mm.get("mode", "test") != "test" else mm.get("mask_modal", "image")
    bev = find(_BEV_IMAGE)
    if bev is not None:
        plan["bev_image_step"] = dict(rot_range=[float(v) for v in bev.get("rot_range", [-0.3925, 0.3925])],
                                      scale_ratio_range=[float(v) for v in bev.get("scale_ratio_range", [0.95, 1.05])],
                                      reverse_angle=bool(bev.get("reverse_angle", False)),
                                      flip_dx_ratio=float(bev.get("flip_dx_ratio", 0.0)),
                                      flip_dy_ratio=float(bev.get("flip_dy_ratio", 0.0)))
    model = cfg.get("model") or {}
    agents = [model] + [model.get(k) for k in ("vehicle_model", "infrastructure_model")]   # the coop detector's extractors
    if any(isinstance(m, dict) and m.get("use_grid_mask", False) for m in agents):
        plan["grid_mask"] = dict(DETECTOR_GRID_MASK)
    return plan
