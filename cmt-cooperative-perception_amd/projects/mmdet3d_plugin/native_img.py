"""Wrappers of the image backbone's entry points (include/cmt_hip.h, cmt_img_*) and the weight packing of
the stem and of the OSA aggregation.  Like native_bev.py: argument checks raise ValueError before the
device check, tensors must live on a HIP device, there is no CPU fallback, no wrapper synchronises with the
host.  The packing reuses native_bev's float64 BN fold and f16 hi / lo split.
"""
import ctypes

import torch

from . import native as N
from .native import _check, _dev, _p, _stream, lib
from .native_bev import _flag, _pair_rows, _shift, fold_bn, out_hw, split_pair
from .native_fpn import pack_conv1x1

__all__ = ["STEM_K", "CONCAT_TM", "MAX_SRC", "pack_stem", "pack_concat", "pool_hw", "concat_tiles", "stem", "conv3x3",
           "conv3x3_gemm", "concat1x1", "ese_gate", "ese_apply", "maxpool"]

STEM_K = 32        # the stem's K = 9 Cin <= 27, zero-padded (cmt_hip.h)
CONCAT_TM = 128    # pixels per tile of cmt_img_concat1x1 (cmt_img_concat_tile_rows())
MAX_SRC = N.IMG_MAX_SRC


def pack_stem(w, bn):
    """Conv2d weight (Cout, Cin <= 3, 3, 3) and its BN (weight, bias, running_mean, running_var, eps) ->
    (pair rows [Cout, 2, 32] with k = (ky*3 + kx) * Cin + c and zeros from 9 Cin on, fp32 shift [Cout])."""
    if w.dim() != 4 or tuple(w.shape[2:]) != (3, 3) or not 1 <= w.shape[1] <= 3:
        raise ValueError(f"expected a (Cout, Cin <= 3, 3, 3) conv weight, got {tuple(w.shape)}")
    scale, shift = fold_bn(*bn)
    w64 = (w.detach().double() * scale[:, None, None, None]).permute(0, 2, 3, 1).reshape(w.shape[0], -1)
    rows = torch.zeros((w.shape[0], STEM_K), dtype=torch.float64, device=w.device)
    rows[:, :w64.shape[1]] = w64
    return split_pair(rows), shift.float().contiguous()


def pack_concat(w, bn):
    """The OSA aggregation's Conv2d weight (Cout, sum C_s, 1, 1) and its BN -> (pair rows [Cout, 2, K] in the
    concatenation's channel order, fp32 shift [Cout])"""
    if not isinstance(bn, (list, tuple)) or len(bn) != 5:
        raise ValueError("bn must be (weight, bias, running_mean, running_var, eps)")
    return pack_conv1x1(w, list(bn))


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


def stem(x, Wp, shift, *, Cout, relu=True, out=None, range_flag=None):
    """cmt_img_stem: the 3 x 3 / stride 2 / pad 1 conv of the fp32 NCHW image [B, Cin <= 3, H, W] -> pair rows
    [B*Ho*Wo, 2, Cout] (rows beyond stay untouched)"""
    if x.dim() != 4 or x.dtype != torch.float32 or not x.is_contiguous():
        raise ValueError("x must be a contiguous fp32 [B, C, H, W] image")
    B, Cin, H, W = (int(s) for s in x.shape)
    if min(B, H, W) <= 0 or not 1 <= Cin <= 3 or Cout <= 0 or Cout % 32:
        raise ValueError(f"a non-empty image with 1 <= Cin <= 3 and Cout % 32 == 0 required, got {tuple(x.shape)} "
                         f"and Cout {Cout}")
    if B * H * W >= 2 ** 31:
        raise ValueError("B*H*W must be below 2^31")
    Ho, Wo = out_hw(H, W, 2)
    _pair_rows("Wp", Wp, Cout, STEM_K)
    if Wp.shape[0] != Cout:
        raise ValueError(f"Wp must hold {Cout} rows, got {Wp.shape[0]}")
    _shift(shift, Cout)
    _flag(range_flag)
    if out is not None:
        _pair_rows("out", out, B * Ho * Wo, Cout)
    _dev(x, Wp, shift, out, range_flag)
    Y = out if out is not None else torch.empty((B * Ho * Wo, 2, Cout), dtype=torch.uint16, device=x.device)
    a = N.ImgStemArgs()
    a.B, a.H, a.W, a.Cin, a.Cout, a.relu = B, H, W, Cin, Cout, int(bool(relu))
    a.X, a.x_bstride, a.Wt, a.shift = _p(x), Cin * H * W, _p(Wp), _p(shift)
    a.Y, a.ldy, a.range_flag = _p(Y), 2 * Cout, _p(range_flag)
    _check(lib().cmt_img_stem(ctypes.byref(a), _stream()), "cmt_img_stem")
    return Y


def _conv_checks(X, Wp, shift, B, H, W, Cin, Cout, stride, out, range_flag, mult):
    if min(B, H, W) <= 0:
        raise ValueError(f"B, H and W must be positive, got {(B, H, W)}")
    if stride not in (1, 2):
        raise ValueError(f"stride must be 1 or 2, got {stride}")
    if Cin <= 0 or Cin % mult or Cout <= 0 or Cout % mult or Cout > 256:
        raise ValueError(f"Cin and Cout must be multiples of {mult}, Cout at most 256, got {Cin} and {Cout}")
    if B * H * W >= 2 ** 31:
        raise ValueError("B*H*W must be below 2^31")
    Ho, Wo = out_hw(H, W, stride)
    _pair_rows("X", X, B * H * W, Cin)
    _pair_rows("Wp", Wp, Cout, 9 * Cin)
    if Wp.shape[0] != Cout:
        raise ValueError(f"Wp must hold {Cout} rows, got {Wp.shape[0]}")
    _shift(shift, Cout)
    _flag(range_flag)
    if out is not None:
        _pair_rows("out", out, B * Ho * Wo, Cout)
    return Ho, Wo


def conv3x3_gemm(X, Wp, shift, *, B, H, W, Cin, Cout, relu=True, out=None, range_flag=None):
    """The stride-1 conv of conv3x3's contract on cmt_gemm's CMT_A_CONV3X3 pair-row path (batch in M, any
    width): Cin % 64 == 0 and Cout % 64 == 0.  Same K order, so the rows are bit-equal to conv3x3's."""
    _conv_checks(X, Wp, shift, B, H, W, Cin, Cout, 1, out, range_flag, 64)
    _dev(X, Wp, shift, out, range_flag)
    M = B * H * W
    Y = out if out is not None else torch.empty((M, 2, Cout), dtype=torch.uint16, device=X.device)
    N.gemm(X, Wp, Y, M=M, N=Cout, K=9 * Cin, lda=Cin, ldw=9 * Cin, ldc=Cout, bias=shift, relu=relu,
           a_mode=N.A_CONV3X3, conv=(H, W, Cin), range_flag=range_flag)
    return Y


def conv3x3(X, Wp, shift, *, B, H, W, Cin, Cout, stride, relu=True, out=None, range_flag=None, nb=0):
    """cmt_img_conv3x3: pair rows [B*H*W, 2, Cin] -> pair rows [B*Ho*Wo, 2, Cout] (rows beyond stay untouched);
    Cin % 32 == 0, Cout % 32 == 0, Cout <= 256, any width.  ``nb``: 32-column blocks per workgroup, a divisor
    of Cout / 32 (0: the library chooses from the row count; the result is the same)"""
    if nb < 0 or (nb and Cout > 0 and (Cout // 32) % nb):
        raise ValueError(f"nb must be 0 or a divisor of Cout / 32 = {Cout // 32}, got {nb}")
    Ho, Wo = _conv_checks(X, Wp, shift, B, H, W, Cin, Cout, stride, out, range_flag, 32)
    _dev(X, Wp, shift, out, range_flag)
    Y = out if out is not None else torch.empty((B * Ho * Wo, 2, Cout), dtype=torch.uint16, device=X.device)
    a = N.ImgConvArgs()
    a.B, a.H, a.W, a.Cin, a.Cout, a.stride, a.relu, a.nb = B, H, W, Cin, Cout, stride, int(bool(relu)), nb
    a.X, a.ldx, a.Wt, a.ldw, a.shift = _p(X), 2 * Cin, _p(Wp), 18 * Cin, _p(shift)
    a.Y, a.ldy, a.range_flag = _p(Y), 2 * Cout, _p(range_flag)
    _check(lib().cmt_img_conv3x3(ctypes.byref(a), _stream()), "cmt_img_conv3x3")
    return Y


def _source(i, t, rows):
    """a source of the concat: uint16 [>= rows, 2, C], C % 32 == 0, rows of 2 C contiguous words at a leading
    dimension (stride(0)) >= 2 C that is a multiple of 8 -> (C, ld)"""
    if t.dtype != torch.uint16 or t.dim() != 3 or t.shape[1] != 2 or t.shape[0] < rows:
        raise ValueError(f"source {i} must be split-f16 pair rows uint16 [>= {rows}, 2, C], got {t.dtype} "
                         f"{tuple(t.shape)}")
    C = int(t.shape[2])
    if C <= 0 or C % 32:
        raise ValueError(f"source {i}: width {C} is no positive multiple of 32")
    ld = int(t.stride(0)) if t.shape[0] > 1 else max(int(t.stride(0)), 2 * C)
    if t.stride(2) != 1 or t.stride(1) != C or ld < 2 * C or ld % 8:
        raise ValueError(f"source {i}: a row must be 2 C contiguous words at a leading dimension >= 2 C, % 8; got "
                         f"strides {tuple(t.stride())}")
    return C, ld


def concat1x1(sources, Wp, shift, *, B, HW, Cout, relu=True, out=None, part=None, range_flag=None):
    """cmt_img_concat1x1: the 1 x 1 conv of the channel concatenation of up to 8 pair-row ``sources``
    ([B*HW, 2, C_s] each, possibly a column slice of a wider row buffer) -> pair rows [B*HW, 2, Cout].
    ``part``: True allocates, a tensor is used, None writes none: fp32 [B, concat_tiles(HW), Cout], the
    per-tile column sums of the stored values.  Returns (rows, part)."""
    sources = list(sources)
    if not 1 <= len(sources) <= MAX_SRC:
        raise ValueError(f"1 to {MAX_SRC} sources required, got {len(sources)}")
    _positive(B=B, HW=HW)
    if Cout <= 0 or Cout % 128:
        raise ValueError(f"Cout must be a positive multiple of 128, got {Cout}")
    if B * HW >= 2 ** 31 or B > 65535:
        raise ValueError("B*HW must be below 2^31 and B at most 65535")
    dims = [_source(i, t, B * HW) for i, t in enumerate(sources)]
    K = sum(c for c, _ in dims)
    _pair_rows("Wp", Wp, Cout, K)
    if Wp.shape[0] != Cout:
        raise ValueError(f"Wp must hold {Cout} rows, got {Wp.shape[0]}")
    _shift(shift, Cout)
    _flag(range_flag)
    if out is not None:
        _pair_rows("out", out, B * HW, Cout)
    tiles = concat_tiles(HW)
    if part is not None and part is not True:
        _f32("part", part, (B, tiles, Cout))
    _dev(*sources, Wp, shift, out, None if part is True else part, range_flag)
    dev = sources[0].device
    Y = out if out is not None else torch.empty((B * HW, 2, Cout), dtype=torch.uint16, device=dev)
    if part is True:
        part = torch.empty((B, tiles, Cout), dtype=torch.float32, device=dev)
    a = N.ImgConcatArgs()
    a.B, a.HW, a.Cout, a.nsrc, a.relu = B, HW, Cout, len(sources), int(bool(relu))
    for i, (t, (c, ld)) in enumerate(zip(sources, dims)):
        a.C[i], a.X[i], a.ldx[i] = c, t.data_ptr(), ld
    a.Wt, a.ldw, a.shift = _p(Wp), 2 * K, _p(shift)
    a.Y, a.ldy, a.part, a.range_flag = _p(Y), 2 * Cout, _p(part), _p(range_flag)
    _check(lib().cmt_img_concat1x1(ctypes.byref(a), _stream()), "cmt_img_concat1x1")
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


def ese_apply(X, gate, *, B, HW, C, identity=None, out=None, range_flag=None):
    """cmt_img_ese_apply: pair rows x [B*HW, 2, C] times gate [B, C] (plus the pair rows ``identity``) -> pair
    rows; ``out`` may be X (in place)"""
    _positive(B=B, HW=HW)
    if C <= 0 or C % 8:
        raise ValueError(f"C must be a positive multiple of 8, got {C}")
    if B * HW >= 2 ** 31:
        raise ValueError("B*HW must be below 2^31")
    _pair_rows("X", X, B * HW, C)
    _f32("gate", gate, (B, C))
    if identity is not None:
        _pair_rows("identity", identity, B * HW, C)
    if out is not None:
        _pair_rows("out", out, B * HW, C)
    _flag(range_flag)
    _dev(X, gate, identity, out, range_flag)
    Y = out if out is not None else torch.empty((B * HW, 2, C), dtype=torch.uint16, device=X.device)
    a = N.ImgApplyArgs()
    a.B, a.HW, a.C = B, HW, C
    a.X, a.ldx, a.gate, a.R, a.ldr = _p(X), 2 * C, _p(gate), _p(identity), 2 * C
    a.Y, a.ldy, a.range_flag = _p(Y), 2 * C, _p(range_flag)
    _check(lib().cmt_img_ese_apply(ctypes.byref(a), _stream()), "cmt_img_ese_apply")
    return Y


def maxpool(X, *, B, H, W, C, out=None):
    """cmt_img_maxpool: 3 x 3 / stride 2 / ceil-mode / no-pad max, pair rows [B*H*W, 2, C] -> [B*Ho*Wo, 2, C]
    with (Ho, Wo) = pool_hw(H, W)"""
    _positive(B=B)
    Ho, Wo = pool_hw(H, W)
    if C <= 0 or C % 8:
        raise ValueError(f"C must be a positive multiple of 8, got {C}")
    if B * H * W >= 2 ** 31:
        raise ValueError("B*H*W must be below 2^31")
    _pair_rows("X", X, B * H * W, C)
    if out is not None:
        _pair_rows("out", out, B * Ho * Wo, C)
    _dev(X, out)
    Y = out if out is not None else torch.empty((B * Ho * Wo, 2, C), dtype=torch.uint16, device=X.device)
    a = N.ImgPoolArgs()
    a.B, a.H, a.W, a.C = B, H, W, C
    a.X, a.ldx, a.Y, a.ldy = _p(X), 2 * C, _p(Y), 2 * C
    _check(lib().cmt_img_maxpool(ctypes.byref(a), _stream()), "cmt_img_maxpool")
    return Y
