"""Wrappers of the image backbone's entry points (include/cmt_hip.h, cmt_img_*) and the weight packing of
the stem and of the OSA aggregation.  Like native_bev.py: argument checks raise ValueError before the
device check, tensors must live on a HIP device, there is no CPU fallback, no wrapper synchronises with the
host.  The packing reuses native_bev's float64 BN fold and f16 hi / lo split.
"""
import ctypes
import functools
import os

import numpy as np
import torch

from . import native as N
from .native import _check, _dev, _p, _stream, lib
from .native_bev import _flag, _shift, fold_bn, out_hw, split_pair

__all__ = ["STEM_K", "CONCAT_TM", "MAX_SRC", "pack_stem", "pack_concat", "pool_hw", "concat_tiles", "stem", "conv3x3",
           "conv3x3_gemm", "concat1x1", "ese_gate", "ese_apply", "maxpool", "IMG_MEAN", "IMG_STD", "norm_constants",
           "test_crop", "crop_lidar2img", "prepare_images", "resize_crop_plan", "resize_crop_lidar2img",
           "image_plan_from_config", "set_img_precision", "img_precision", "round_f16",
           "pack_stem_f16", "pack_conv3x3_f16", "pack_concat_f16", "stem_f16", "conv3x3_f16", "concat1x1_f16",
           "ese_apply_f16", "maxpool_f16"]

STEM_K = 32        # the stem's K = 9 Cin <= 27, zero-padded (cmt_hip.h)
CONCAT_TM = 128    # pixels per tile of cmt_img_concat1x1 (cmt_img_concat_tile_rows())
MAX_SRC = N.IMG_MAX_SRC


# img_norm_cfg of the reference's VoVNet configs (BGR order as cv2 loads, to_rgb=False)
IMG_MEAN = (103.530, 116.280, 123.675)
IMG_STD = (57.375, 57.120, 58.395)


def norm_constants(mean, std):
    """(mean32, inv32) as the pipeline holds them: mean32 = float32(mean), inv32 = float32(1 / float64(float32(std)))
    (mmcv's imnormalize_ subtracts the float32 mean and multiplies by the reciprocal of the float32 std)"""
    mean32 = np.asarray(mean, dtype=np.float32).reshape(-1)
    std32 = np.asarray(std, dtype=np.float32).reshape(-1)
    if mean32.shape != (3,) or std32.shape != (3,):
        raise ValueError("mean and std must have 3 entries")
    if not (np.all(np.isfinite(mean32)) and np.all(np.isfinite(std32)) and np.all(std32 != 0)):
        raise ValueError("mean must be finite and std finite and non-zero")
    return mean32, (1.0 / std32.astype(np.float64)).astype(np.float32)


def resize_crop_plan(aug_hw, final_dim, bot_pct_lim=(0.0, 0.0)):
    """The whole test branch of ResizeCropFlipImage[Coop]._sample_augmentation (transform_3d.py:449-455) for
    ``aug_hw = (H, W)`` of the config's ida_aug_conf and ``final_dim = (fH, fW)`` -> (resize, (newW, newH), crop):
    the frame is resized to (newW, newH), whatever its own size, and ``crop = (x0, y0, x1, y1)`` is in pixels of the
    resized frame.  int() truncates as there.  H and W are the config's, not the frame's: a 1200 x 1920 TUMTraf
    frame under H = 900, W = 1600 gets resize 1.0 and is still resampled to 1600 x 900."""
    H, W = (int(v) for v in aug_hw)
    fH, fW = (int(v) for v in final_dim)
    if min(H, W, fH, fW) <= 0:
        raise ValueError(f"positive sizes required, got aug_hw {tuple(aug_hw)}, final_dim {tuple(final_dim)}")
    resize = max(fH / H, fW / W)
    new_w, new_h = int(W * resize), int(H * resize)
    crop_h = int((1 - float(np.mean(bot_pct_lim))) * new_h) - fH
    crop_w = int(max(0, new_w - fW) / 2)
    return resize, (new_w, new_h), (crop_w, crop_h, crop_w + fW, crop_h + fH)


def resize_crop_lidar2img(cam_intrinsic, lidar2cam, resize, crop):
    """lidar2img of the resized and cropped image, in float64: rows 0-1 of the intrinsic are multiplied by
    ``resize``, the principal point then moves by (-x0, -y0) (transform_3d.py:373-378 and 420-431, no flip, no
    rotation), then intrinsic @ lidar2cam.  ``cam_intrinsic`` is 3 x 3 or 4 x 4, ``lidar2cam`` 4 x 4; the inputs are
    not modified.  ``resize`` is the scalar of resize_crop_plan, as in the reference, also where the pixels were
    scaled by other, anisotropic factors because the frame is not the config's H x W (TUMTraf: pixels x (0.8333,
    0.75), intrinsics x 1.0).  That is the reference's behaviour, kept so that its checkpoints see the projection
    they were trained with."""
    K = np.array(cam_intrinsic, dtype=np.float64)
    E = np.array(lidar2cam, dtype=np.float64)
    if K.shape == (3, 3):
        K4 = np.eye(4)
        K4[:3, :3] = K
        K = K4
    if K.shape != (4, 4) or E.shape != (4, 4):
        raise ValueError(f"cam_intrinsic must be 3 x 3 or 4 x 4 and lidar2cam 4 x 4, got {K.shape} and {E.shape}")
    K[:2] *= float(resize)
    K[0, 2] -= float(crop[0])
    K[1, 2] -= float(crop[1])
    return K @ E


def test_crop(src_hw, final_dim, bot_pct_lim=(0.0, 0.0)):
    """resize_crop_plan for a frame that already has the config's size ``src_hw = (H, W)`` -> (resize, crop) with
    crop = (x0, y0, x1, y1) in source pixels.  Only resize == 1 (a pure integer crop) is accepted here;
    resize_crop_plan and prepare_images(resize_dims=...) cover every other case."""
    resize, _, crop = resize_crop_plan(src_hw, final_dim, bot_pct_lim)
    if resize != 1.0:
        raise NotImplementedError(f"test_crop: {tuple(src_hw)} -> {tuple(final_dim)} needs a resize by {resize:.6g}: use "
                                  "resize_crop_plan and prepare_images(resize_dims=...)")
    return resize, crop


test_crop.__test__ = False   # a host helper, not a test, whatever collects names starting with test_


def crop_lidar2img(cam_intrinsic, lidar2cam, crop):
    """resize_crop_lidar2img at resize 1: the principal point moves by (-x0, -y0), then intrinsic @ lidar2cam"""
    return resize_crop_lidar2img(cam_intrinsic, lidar2cam, 1.0, crop)


def _pipeline_steps(steps):
    for st in steps or []:
        if isinstance(st, dict):
            yield st
            yield from _pipeline_steps(st.get("transforms"))


def image_plan_from_config(cfg):
    """The image preparation of a config dict (config.load_config): the ResizeCropFlipImage[Coop]
    (training=False), NormalizeMultiviewImage[Coop] and PadMultiViewImage[Coop] steps of ``data.test.pipeline``,
    looked for inside MultiScaleFlipAug3D's ``transforms`` too -> dict(resize, resize_dims, crop, mean, std, to_rgb,
    size_divisor), the first three from resize_crop_plan; None for a pipeline without the resize step (LiDAR only)."""
    steps = list(_pipeline_steps(cfg["data"]["test"]["pipeline"]))

    def find(kind):
        hits = [st for st in steps if st.get("type") in (kind, kind + "Coop")]
        return hits[0] if hits else None

    rcf = find("ResizeCropFlipImage")
    if rcf is None:
        return None
    if rcf.get("training", True):
        raise ValueError("the test pipeline's ResizeCropFlipImage step has training=True")
    aug = rcf["data_aug_conf"]
    resize, dims, crop = resize_crop_plan((aug["H"], aug["W"]), aug["final_dim"], aug.get("bot_pct_lim", (0.0, 0.0)))
    norm, pad = find("NormalizeMultiviewImage"), find("PadMultiViewImage")
    if norm is None or pad is None:
        raise ValueError("the test pipeline resizes images but has no NormalizeMultiviewImage / PadMultiViewImage step")
    if pad.get("size_divisor") is None:
        raise ValueError("PadMultiViewImage with a fixed size is not supported, only size_divisor")
    return dict(resize=resize, resize_dims=dims, crop=crop, mean=tuple(norm["mean"]), std=tuple(norm["std"]),
                to_rgb=bool(norm.get("to_rgb", True)), size_divisor=int(pad["size_divisor"]))


def prepare_images(frames, crop=None, mean=IMG_MEAN, std=IMG_STD, to_rgb=False, size_divisor=32, out=None, size=None,
                   resize_dims=None):
    """cmt_img_prepare: uint8 frames [N, Hs, Ws, 3] (interleaved, as cv2 loads them) -> the backbone's input fp32
    [N, 3, Hp, Wp]: crop, normalise, zero-pad, HWC -> CHW in one kernel.  ``crop`` = (x0, y0, x1, y1) in source
    pixels as test_crop returns it (None: the whole frame); crop pixels outside the source count as byte 0
    before normalisation.  (Hp, Wp) is the crop size rounded up to ``size_divisor``, or the explicit
    ``size = (Hp, Wp)``; the pad is 0 after normalisation.  ``mean`` / ``std`` are indexed by output channel,
    which reads source channel 2 - c when ``to_rgb``.

    ``resize_dims = (Wr, Hr)`` (as resize_crop_plan returns it) selects cmt_img_resize_prepare: the frame is first
    resampled to Hr x Wr with the 8-bit fixed-point bilinear of include/cmt_hip.h, in the same kernel; ``crop`` is
    then in pixels of the resized frame and defaults to all of it."""
    if not torch.is_tensor(frames) or frames.dtype != torch.uint8:
        raise ValueError(f"frames must be a uint8 tensor, got {frames.dtype if torch.is_tensor(frames) else type(frames)}")
    if frames.dim() != 4 or frames.shape[3] != 3 or min(frames.shape) <= 0:
        raise ValueError(f"frames must be a non-empty [N, H, W, 3] tensor, got {tuple(frames.shape)}")
    if not frames.is_contiguous():
        raise ValueError("frames must be contiguous (interleaved HWC rows)")
    n, Hs, Ws = (int(s) for s in frames.shape[:3])
    Wr, Hr = Ws, Hs
    if resize_dims is not None:
        if len(tuple(resize_dims)) != 2:
            raise ValueError(f"resize_dims must be (Wr, Hr), got {resize_dims!r}")
        Wr, Hr = (int(v) for v in resize_dims)
        if Wr <= 0 or Hr <= 0 or max(Wr, Hr) >= 2 ** 30:
            raise ValueError(f"resize_dims must be positive and below 2^30, got {(Wr, Hr)}")
    elif not frames.is_cuda:
        raise ValueError("frames must live on a HIP device (no CPU path)")
    x0, y0, x1, y1 = (0, 0, Wr, Hr) if crop is None else (int(v) for v in crop)
    w, h = x1 - x0, y1 - y0
    if w <= 0 or h <= 0:
        raise ValueError(f"empty crop {(x0, y0, x1, y1)}")
    if size is not None:
        Hp, Wp = (int(v) for v in size)
        if Hp < h or Wp < w:
            raise ValueError(f"size {(Hp, Wp)} below the crop's {(h, w)}")
    else:
        d = int(size_divisor)
        if d <= 0:
            raise ValueError(f"size_divisor must be positive, got {size_divisor}")
        Hp, Wp = (h + d - 1) // d * d, (w + d - 1) // d * d
    if max(abs(x0), abs(y0), Hp, Wp) >= 2 ** 30 or n * Hp * ((Wp + 3) // 4) >= 2 ** 31:
        raise ValueError("crop or output size beyond the kernel's index range")
    mean32, inv32 = norm_constants(mean, std)
    if not frames.is_cuda:
        raise ValueError("frames must live on a HIP device (no CPU path)")
    if out is not None:
        _f32("out", out, (n, 3, Hp, Wp))
        if out.device != frames.device:
            raise ValueError("out must live on the frames' device")
    Y = out if out is not None else torch.empty((n, 3, Hp, Wp), dtype=torch.float32, device=frames.device)
    a = N.ImgPrepareArgs() if resize_dims is None else N.ImgResizeArgs()
    a.N, a.Hs, a.Ws, a.to_rgb = n, Hs, Ws, int(bool(to_rgb))
    a.x0, a.y0, a.w, a.h, a.Hp, a.Wp = x0, y0, w, h, Hp, Wp
    for c in range(3):
        a.mean[c], a.inv_std[c] = float(mean32[c]), float(inv32[c])
    a.src, a.dst = _p(frames), _p(Y)
    if resize_dims is None:
        _check(lib().cmt_img_prepare(ctypes.byref(a), _stream()), "cmt_img_prepare")
    else:
        a.Hr, a.Wr = Hr, Wr
        _check(lib().cmt_img_resize_prepare(ctypes.byref(a), _stream()), "cmt_img_resize_prepare")
    return Y


class RowFormat:
    """What the wrappers below need to know of a row buffer of the backbone kernels.  Two instances: PAIR, the
    split-f16 pair rows uint16 [rows, 2, C] of cmt_img_*, and FP16, the plain fp16 rows [rows, C] of cmt_img_*_f16
    (the one-pass policy).  ``words``: 16-bit words per element; ``suffix``: of the entry names; ``quantize``:
    float64 weight rows -> the format's W image.  What a wrapper takes beyond contiguous buffers differs between
    the two and is data here: ``strided_stem`` (the stem takes a strided batch axis), ``sliced_conv`` (conv3x3
    takes column slices of wider row buffers for X and out; the concat's sources may be slices in both)."""

    def __init__(self, what, dtype, words, suffix, quantize, strided_stem, sliced_conv):
        self.what, self.dtype, self.words, self.suffix, self.quantize = what, dtype, words, suffix, quantize
        self.strided_stem, self.sliced_conv = strided_stem, sliced_conv

    def shape(self, rows, C):
        return (rows, 2, C) if self.words == 2 else (rows, C)

    def empty(self, rows, C, device):
        return torch.empty(self.shape(rows, C), dtype=self.dtype, device=device)

    def width(self, t):
        """C of a row buffer, 0 for anything of another rank"""
        return int(t.shape[-1]) if torch.is_tensor(t) and t.dim() == len(self.shape(0, 0)) else 0

    def check(self, name, t, rows, C, sliced=False):
        """``t`` holds at least ``rows`` rows of width C: contiguous, or with ``sliced`` a column slice of a wider
        row buffer (a row's words contiguous at a leading dimension % 8) -> the leading dimension in words"""
        shape = self.shape(rows, C)
        if t.dtype != self.dtype or t.dim() != len(shape) or tuple(t.shape[1:]) != shape[1:] or t.shape[0] < rows or \
                not (sliced or t.is_contiguous()):
            raise ValueError(f"{name} must be {'' if sliced else 'contiguous '}{self.what} [>= {rows}, "
                             f"{', '.join(str(s) for s in shape[1:])}], got {t.dtype} {tuple(t.shape)}")
        n = self.words * C
        if not sliced:
            return n
        ld = int(t.stride(0)) if t.shape[0] > 1 else max(int(t.stride(0)), n)
        if tuple(t.stride()[1:]) != ((C, 1) if self.words == 2 else (1,)) or ld < n or ld % 8:
            raise ValueError(f"{name}: a row must be {n} contiguous words at a leading dimension >= {n}, % 8; got "
                             f"strides {tuple(t.stride())}")
        return ld

    def call(self, kind, args):
        name = f"cmt_img_{kind}{self.suffix}"
        _check(getattr(lib(), name)(ctypes.byref(args), _stream()), name)


PAIR = RowFormat("split-f16 pair rows uint16", torch.uint16, 2, "", split_pair, strided_stem=False, sliced_conv=False)
FP16 = RowFormat("fp16 rows", torch.float16, 1, "_f16", lambda w64: round_f16(w64), strided_stem=True, sliced_conv=True)


def _bind(fn, fmt):
    """the public wrapper of one format: ``fn`` with its first argument bound"""
    f = functools.partial(fn, fmt)
    f.__doc__, f.__name__ = fn.__doc__, fn.__name__.lstrip("_") + fmt.suffix
    return f


def _pack_stem(fmt, w, bn):
    """Conv2d weight (Cout, Cin <= 3, 3, 3) and its BN (weight, bias, running_mean, running_var, eps) ->
    (W rows of K = 32 with k = (ky*3 + kx) * Cin + c and zeros from 9 Cin on, fp32 shift [Cout]); the rows are
    pair rows [Cout, 2, 32] (pack_stem) or fp16 [Cout, 32] (pack_stem_f16)."""
    if w.dim() != 4 or tuple(w.shape[2:]) != (3, 3) or not 1 <= w.shape[1] <= 3:
        raise ValueError(f"expected a (Cout, Cin <= 3, 3, 3) conv weight, got {tuple(w.shape)}")
    scale, shift = fold_bn(*bn)
    w64 = (w.detach().double() * scale[:, None, None, None]).permute(0, 2, 3, 1).reshape(w.shape[0], -1)
    rows = torch.zeros((w.shape[0], STEM_K), dtype=torch.float64, device=w.device)
    rows[:, :w64.shape[1]] = w64
    return fmt.quantize(rows), shift.float().contiguous()


def _pack_concat(fmt, w, bn):
    """The OSA aggregation's Conv2d weight (Cout, sum C_s, 1, 1) and its BN -> (W rows in the concatenation's
    channel order, fp32 shift [Cout]); pair rows [Cout, 2, K] (pack_concat) or fp16 [Cout, K] (pack_concat_f16)."""
    if not isinstance(bn, (list, tuple)) or len(bn) != 5:
        raise ValueError("bn must be (weight, bias, running_mean, running_var, eps)")
    if w.dim() != 4 or tuple(w.shape[2:]) != (1, 1):
        raise ValueError(f"expected a (Cout, Cin, 1, 1) conv weight, got {tuple(w.shape)}")
    scale, shift = fold_bn(*bn)
    w64 = w.detach().double().reshape(w.shape[0], w.shape[1]) * scale[:, None]
    return fmt.quantize(w64), shift.float().contiguous()


def pack_conv3x3_f16(w, bn):
    """native_bev.pack_conv3x3 for cmt_img_conv3x3_f16 -> (fp16 [Cout, 9 Cin] with k = (ky*3 + kx) * Cin + c,
    fp32 shift [Cout])"""
    if w.dim() != 4 or tuple(w.shape[2:]) != (3, 3):
        raise ValueError(f"expected a (Cout, Cin, 3, 3) conv weight, got {tuple(w.shape)}")
    scale, shift = fold_bn(*bn)
    w64 = w.detach().double() * scale[:, None, None, None]
    return round_f16(w64.permute(0, 2, 3, 1).reshape(w.shape[0], -1)), shift.float().contiguous()


pack_stem, pack_stem_f16 = _bind(_pack_stem, PAIR), _bind(_pack_stem, FP16)
pack_concat, pack_concat_f16 = _bind(_pack_concat, PAIR), _bind(_pack_concat, FP16)


def pool_hw(H, W):
    """Output size of MaxPool2d(kernel 3, stride 2, ceil_mode=True), no padding: ceil((n - 3) / 2) + 1"""
    H, W = int(H), int(W)
    if H < 2 or W < 2:
        raise ValueError(f"the 3 x 3 / stride 2 ceil-mode pool needs H, W >= 2, got {(H, W)}")
    return (H - 2) // 2 + 1, (W - 2) // 2 + 1


def concat_tiles(HW):
    return (int(HW) + CONCAT_TM - 1) // CONCAT_TM


def _f32(name, t, shape):
    if t.dtype != torch.float32 or tuple(t.shape) != tuple(shape) or not t.is_contiguous():
        raise ValueError(f"{name} must be contiguous fp32 {tuple(shape)}, got {t.dtype} {tuple(t.shape)}")


def _positive(**kw):
    for k, v in kw.items():
        if int(v) <= 0:
            raise ValueError(f"{k} must be positive, got {v}")


def _w_rows(fmt, Wt, Cout, K):
    fmt.check("W", Wt, Cout, K)
    if Wt.shape[0] != Cout:
        raise ValueError(f"W must hold {Cout} rows, got {Wt.shape[0]}")


def _stem(fmt, x, Wt, shift, *, Cout, relu=True, out=None, range_flag=None):
    """cmt_img_stem[_f16]: the 3 x 3 / stride 2 / pad 1 conv of the fp32 NCHW image [B, Cin <= 3, H, W] -> rows
    of width Cout for the B*Ho*Wo outputs (rows beyond stay untouched).  ``stem``: a contiguous image to pair rows
    [B*Ho*Wo, 2, Cout]; ``stem_f16``: a strided batch axis is taken as it is, to fp16 rows [B*Ho*Wo, Cout]."""
    if x.dim() != 4 or x.dtype != torch.float32 or not (fmt.strided_stem or x.is_contiguous()):
        raise ValueError(f"x must be {'an' if fmt.strided_stem else 'a contiguous'} fp32 [B, C, H, W] image")
    B, Cin, H, W = (int(s) for s in x.shape)
    if min(B, H, W) <= 0 or not 1 <= Cin <= 3 or Cout <= 0 or Cout % 32:
        raise ValueError(f"a non-empty image with 1 <= Cin <= 3 and Cout % 32 == 0 required, got {tuple(x.shape)} "
                         f"and Cout {Cout}")
    bstride = int(x.stride(0)) if fmt.strided_stem and B > 1 else Cin * H * W
    if fmt.strided_stem and (tuple(x.stride()[1:]) != (H * W, W, 1) or bstride < Cin * H * W):
        raise ValueError("every image of x must be contiguous [C, H, W] at a batch stride >= C*H*W")
    if B * H * W >= 2 ** 31:
        raise ValueError("B*H*W must be below 2^31")
    Ho, Wo = out_hw(H, W, 2)
    _w_rows(fmt, Wt, Cout, STEM_K)
    _shift(shift, Cout)
    _flag(range_flag)
    if out is not None:
        fmt.check("out", out, B * Ho * Wo, Cout)
    _dev(x, Wt, shift, out, range_flag)
    Y = out if out is not None else fmt.empty(B * Ho * Wo, Cout, x.device)
    a = N.ImgStemArgs()
    a.B, a.H, a.W, a.Cin, a.Cout, a.relu = B, H, W, Cin, Cout, int(bool(relu))
    a.X, a.x_bstride, a.Wt, a.shift = _p(x), bstride, _p(Wt), _p(shift)
    a.Y, a.ldy, a.range_flag = _p(Y), fmt.words * Cout, _p(range_flag)
    fmt.call("stem", a)
    return Y


def _conv_checks(fmt, X, Wt, shift, B, H, W, Cin, Cout, stride, out, range_flag, mult, sliced):
    """-> (Ho, Wo, ldx, ldy)"""
    if min(B, H, W) <= 0:
        raise ValueError(f"B, H and W must be positive, got {(B, H, W)}")
    if stride not in (1, 2):
        raise ValueError(f"stride must be 1 or 2, got {stride}")
    if Cin <= 0 or Cin % mult or Cout <= 0 or Cout % mult or Cout > 256:
        raise ValueError(f"Cin and Cout must be multiples of {mult}, Cout at most 256, got {Cin} and {Cout}")
    if B * H * W >= 2 ** 31:
        raise ValueError("B*H*W must be below 2^31")
    Ho, Wo = out_hw(H, W, stride)
    ldx = fmt.check("X", X, B * H * W, Cin, sliced)
    _w_rows(fmt, Wt, Cout, 9 * Cin)
    _shift(shift, Cout)
    _flag(range_flag)
    ldy = fmt.words * Cout if out is None else fmt.check("out", out, B * Ho * Wo, Cout, sliced)
    return Ho, Wo, ldx, ldy


def conv3x3_gemm(X, Wp, shift, *, B, H, W, Cin, Cout, relu=True, out=None, range_flag=None):
    """The stride-1 conv of conv3x3's contract on cmt_gemm's CMT_A_CONV3X3 pair-row path (batch in M, any
    width): Cin % 64 == 0 and Cout % 64 == 0.  Same K order, so the rows are bit-equal to conv3x3's."""
    _conv_checks(PAIR, X, Wp, shift, B, H, W, Cin, Cout, 1, out, range_flag, 64, False)
    _dev(X, Wp, shift, out, range_flag)
    M = B * H * W
    Y = out if out is not None else PAIR.empty(M, Cout, X.device)
    N.gemm(X, Wp, Y, M=M, N=Cout, K=9 * Cin, lda=Cin, ldw=9 * Cin, ldc=Cout, bias=shift, relu=relu,
           a_mode=N.A_CONV3X3, conv=(H, W, Cin), range_flag=range_flag)
    return Y


def _conv3x3(fmt, X, Wt, shift, *, B, H, W, Cin, Cout, stride, relu=True, out=None, range_flag=None, nb=0):
    """cmt_img_conv3x3[_f16]: rows of width Cin for B*H*W pixels -> rows of width Cout for B*Ho*Wo (rows beyond
    stay untouched); Cin % 32 == 0, Cout % 32 == 0, Cout <= 256, any map width.  ``conv3x3``: contiguous pair rows
    [.., 2, C]; ``conv3x3_f16``: fp16 rows [.., C], where X and out may be column slices of wider row buffers
    (leading dimension % 8).  ``nb``: 32-column blocks per workgroup, a divisor of Cout / 32 (0: the library
    chooses from the row count; the result is the same)"""
    if nb < 0 or (nb and Cout > 0 and (Cout // 32) % nb):
        raise ValueError(f"nb must be 0 or a divisor of Cout / 32 = {Cout // 32}, got {nb}")
    Ho, Wo, ldx, ldy = _conv_checks(fmt, X, Wt, shift, B, H, W, Cin, Cout, stride, out, range_flag, 32, fmt.sliced_conv)
    _dev(X, Wt, shift, out, range_flag)
    Y = out if out is not None else fmt.empty(B * Ho * Wo, Cout, X.device)
    a = N.ImgConvArgs()
    a.B, a.H, a.W, a.Cin, a.Cout, a.stride, a.relu, a.nb = B, H, W, Cin, Cout, stride, int(bool(relu)), nb
    a.X, a.ldx, a.Wt, a.ldw, a.shift = _p(X), ldx, _p(Wt), 9 * fmt.words * Cin, _p(shift)
    a.Y, a.ldy, a.range_flag = _p(Y), ldy, _p(range_flag)
    fmt.call("conv3x3", a)
    return Y


def _concat1x1(fmt, sources, Wt, shift, *, B, HW, Cout, relu=True, out=None, part=None, range_flag=None):
    """cmt_img_concat1x1[_f16]: the 1 x 1 conv of the channel concatenation of up to 8 ``sources`` (rows of
    width C_s % 32 == 0 for B*HW pixels each, possibly a column slice of a wider row buffer) -> rows of width Cout;
    pair rows (``concat1x1``) or fp16 rows (``concat1x1_f16``).  ``part``: True allocates, a tensor is used, None
    writes none: fp32 [B, concat_tiles(HW), Cout], the per-tile column sums of the values as stored.  Returns
    (rows, part)."""
    sources = list(sources)
    if not 1 <= len(sources) <= MAX_SRC:
        raise ValueError(f"1 to {MAX_SRC} sources required, got {len(sources)}")
    _positive(B=B, HW=HW)
    if Cout <= 0 or Cout % 128:
        raise ValueError(f"Cout must be a positive multiple of 128, got {Cout}")
    if B * HW >= 2 ** 31 or B > 65535:
        raise ValueError("B*HW must be below 2^31 and B at most 65535")
    dims = []
    for i, t in enumerate(sources):
        C = fmt.width(t)
        if C <= 0 or C % 32:
            raise ValueError(f"source {i} must be {fmt.what} [>= {B * HW}, ..., C] with C a positive multiple of 32, got "
                             f"{tuple(t.shape) if torch.is_tensor(t) else type(t)}")
        dims.append((C, fmt.check(f"source {i}", t, B * HW, C, sliced=True)))
    K = sum(c for c, _ in dims)
    _w_rows(fmt, Wt, Cout, K)
    _shift(shift, Cout)
    _flag(range_flag)
    if out is not None:
        fmt.check("out", out, B * HW, Cout)
    tiles = concat_tiles(HW)
    if part is not None and part is not True:
        _f32("part", part, (B, tiles, Cout))
    _dev(*sources, Wt, shift, out, None if part is True else part, range_flag)
    dev = sources[0].device
    Y = out if out is not None else fmt.empty(B * HW, Cout, dev)
    if part is True:
        part = torch.empty((B, tiles, Cout), dtype=torch.float32, device=dev)
    a = N.ImgConcatArgs()
    a.B, a.HW, a.Cout, a.nsrc, a.relu = B, HW, Cout, len(sources), int(bool(relu))
    for i, (t, (c, ld)) in enumerate(zip(sources, dims)):
        a.C[i], a.X[i], a.ldx[i] = c, t.data_ptr(), ld
    a.Wt, a.ldw, a.shift = _p(Wt), fmt.words * K, _p(shift)
    a.Y, a.ldy, a.part, a.range_flag = _p(Y), fmt.words * Cout, _p(part), _p(range_flag)
    fmt.call("concat1x1", a)
    return Y, part


def ese_gate(part, w, bias, *, HW, out=None):
    """cmt_img_ese_gate: fp32 per-tile sums [B, tiles, C], fc weight [C, C] (or (C, C, 1, 1)) and bias [C] ->
    the gate fp32 [B, C] = hsigmoid(fc(mean))"""
    if part.dim() != 3 or part.dtype != torch.float32 or not part.is_contiguous() or min(part.shape) <= 0:
        raise ValueError(f"part must be contiguous non-empty fp32 [B, tiles, C], got {part.dtype} {tuple(part.shape)}")
    B, tiles, C = (int(s) for s in part.shape)
    _positive(HW=HW)
    if C % 4 or C > 8192 or B > 65535:
        raise ValueError(f"C must be a multiple of 4, at most 8192, and B at most 65535, got C {C}, B {B}")
    if w.dim() == 4 and tuple(w.shape[2:]) == (1, 1):
        w = w.view(w.shape[0], w.shape[1])
    _f32("w", w, (C, C))
    _f32("bias", bias, (C,))
    if out is not None:
        _f32("out", out, (B, C))
    _dev(part, w, bias, out)
    G = out if out is not None else torch.empty((B, C), dtype=torch.float32, device=part.device)
    a = N.ImgGateArgs()
    a.B, a.C, a.tiles, a.HW = B, C, tiles, int(HW)
    a.part, a.Wfc, a.bias, a.gate = _p(part), _p(w), _p(bias), _p(G)
    _check(lib().cmt_img_ese_gate(ctypes.byref(a), _stream()), "cmt_img_ese_gate")
    return G


def _ese_apply(fmt, X, gate, *, B, HW, C, identity=None, out=None, range_flag=None):
    """cmt_img_ese_apply[_f16]: rows x of width C for B*HW pixels times gate [B, C] (plus the rows ``identity``),
    in fp32, converted once -> rows; ``out`` may be X (in place).  Pair rows (``ese_apply``) or fp16 rows
    (``ese_apply_f16``)."""
    _positive(B=B, HW=HW)
    if C <= 0 or C % 8:
        raise ValueError(f"C must be a positive multiple of 8, got {C}")
    if B * HW >= 2 ** 31:
        raise ValueError("B*HW must be below 2^31")
    fmt.check("X", X, B * HW, C)
    _f32("gate", gate, (B, C))
    if identity is not None:
        fmt.check("identity", identity, B * HW, C)
    if out is not None:
        fmt.check("out", out, B * HW, C)
    _flag(range_flag)
    _dev(X, gate, identity, out, range_flag)
    Y = out if out is not None else fmt.empty(B * HW, C, X.device)
    a = N.ImgApplyArgs()
    a.B, a.HW, a.C = B, HW, C
    a.X, a.ldx, a.gate, a.R, a.ldr = _p(X), fmt.words * C, _p(gate), _p(identity), fmt.words * C
    a.Y, a.ldy, a.range_flag = _p(Y), fmt.words * C, _p(range_flag)
    fmt.call("ese_apply", a)
    return Y


def _maxpool(fmt, X, *, B, H, W, C, out=None):
    """cmt_img_maxpool[_f16]: 3 x 3 / stride 2 / ceil-mode / no-pad max, rows of width C for B*H*W pixels -> rows
    for B*Ho*Wo with (Ho, Wo) = pool_hw(H, W).  Pair rows (``maxpool``) or fp16 rows (``maxpool_f16``)."""
    _positive(B=B)
    Ho, Wo = pool_hw(H, W)
    if C <= 0 or C % 8:
        raise ValueError(f"C must be a positive multiple of 8, got {C}")
    if B * H * W >= 2 ** 31:
        raise ValueError("B*H*W must be below 2^31")
    fmt.check("X", X, B * H * W, C)
    if out is not None:
        fmt.check("out", out, B * Ho * Wo, C)
    _dev(X, out)
    Y = out if out is not None else fmt.empty(B * Ho * Wo, C, X.device)
    a = N.ImgPoolArgs()
    a.B, a.H, a.W, a.C = B, H, W, C
    a.X, a.ldx, a.Y, a.ldy = _p(X), fmt.words * C, _p(Y), fmt.words * C
    fmt.call("maxpool", a)
    return Y


stem, stem_f16 = _bind(_stem, PAIR), _bind(_stem, FP16)
conv3x3, conv3x3_f16 = _bind(_conv3x3, PAIR), _bind(_conv3x3, FP16)
concat1x1, concat1x1_f16 = _bind(_concat1x1, PAIR), _bind(_concat1x1, FP16)
ese_apply, ese_apply_f16 = _bind(_ese_apply, PAIR), _bind(_ese_apply, FP16)
maxpool, maxpool_f16 = _bind(_maxpool, PAIR), _bind(_maxpool, FP16)


# ---- the one-pass fp16 policy -------------------------------------------------------------------------------------
# Arithmetic of VoVNet (models/backbones/vovnet.py): "ref" (the three-pass split-f16 kernels above on pair rows,
# fp32-accurate) or "fp16" (cmt_img_*_f16: plain fp16 rows [B*H*W, C] between launches, weights folded in float64
# and rounded once to fp16, one MFMA per 16-k step with fp32 accumulation).  Independent of runtime.set_precision
# (the head's policy).  The initial mode is the environment variable CMT_IMG_PRECISION, read once here.
_IMG_PRECISIONS = ("ref", "fp16")


def _img_precision_name(mode, what):
    if mode not in _IMG_PRECISIONS:
        raise ValueError(f"{what} must be one of {list(_IMG_PRECISIONS)}, got {mode!r}")
    return mode


_img_precision = _img_precision_name(os.environ.get("CMT_IMG_PRECISION") or "ref", "CMT_IMG_PRECISION")


def set_img_precision(mode):
    """Select the arithmetic of the image backbone ("ref" or "fp16"); returns the previous mode."""
    global _img_precision
    old, _img_precision = _img_precision, _img_precision_name(mode, "img precision")
    return old


def img_precision():
    """the current mode of set_img_precision"""
    return _img_precision


def round_f16(w64):
    """float64 rows [N, K] -> contiguous fp16 [N, K], rounded once (RNE); a value that is non-finite or beyond
    fp16's largest finite 65504 raises"""
    if w64.numel() and not bool(torch.isfinite(w64).all()):
        raise ValueError("non-finite folded weights cannot take the fp16 format")
    if w64.numel() and w64.abs().max().item() > 65504.0:
        raise ValueError("folded weights beyond the f16 range (65504) cannot take the fp16 format")
    return w64.half().contiguous()
