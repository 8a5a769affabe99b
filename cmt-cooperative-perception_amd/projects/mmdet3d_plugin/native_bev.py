"""Wrappers of the dense BEV backbone / neck entry points (include/cmt_hip.h, cmt_bev_*) and of the
two cmt_gemm conv paths the stride-1 layers run on, plus the weight packing (BN folded in float64,
split to f16 hi / lo).  Like native_sparse.py: argument checks raise ValueError before the device
check, tensors must live on a HIP device, there is no CPU fallback, no wrapper synchronises with
the host.  The packing helpers are pure torch and run wherever the weights live.
"""
import ctypes

import torch

from . import native as N
from .native import _check, _dev, _p, _stream, lib

__all__ = ["RowMap", "fold_bn", "split_pair", "unpack_pair", "pack_conv3x3", "pack_deblock", "out_hw", "conv3x3",
           "conv3x3_gemm", "conv3x3_nchw_gemm", "deblock", "to_rows", "WMAX"]

WMAX = 180   # the widest map the conv kernels take (cmt_hip.h)


class RowMap:
    """A feature map as NHWC split-f16 pair rows: ``rows`` uint16 [B*H*W, 2, C] (cmt_hip.h CMT_F16P)
    with ``shape`` (B, C, H, W), what SECOND hands to SECONDFPN."""

    def __init__(self, rows, shape):
        self.rows, self.shape = rows, tuple(int(s) for s in shape)

    def nchw(self):
        """The fp32 NCHW tensor (torch ops, off the hot path)."""
        B, C, H, W = self.shape
        v = self.rows[:B * H * W].view(torch.float16).float()
        return (v[:, 0] + v[:, 1]).view(B, H, W, C).permute(0, 3, 1, 2).contiguous()


def fold_bn(weight, bias, running_mean, running_var, eps):
    """BN2d in eval mode as float64 (scale, shift): y = scale * x + shift"""
    scale = weight.detach().double() / torch.sqrt(running_var.detach().double() + eps)
    return scale, bias.detach().double() - running_mean.detach().double() * scale


def split_pair(w64):
    """float64 rows [N, K] -> the split pair image uint16 [N, 2, K]: hi = f16(w), lo = f16(w - hi), the
    residual taken in float64 (packing.to_dtype splits the fp32-rounded weight)"""
    if w64.numel() and w64.abs().max().item() >= 65504.0:
        raise ValueError("weights beyond the f16 range cannot take the split f16 pair format")
    hi = w64.half()
    lo = (w64 - hi.double()).half()
    return torch.stack([hi, lo], dim=1).contiguous().view(torch.uint16)


def unpack_pair(wp):
    """uint16 [N, 2, K] -> float64 [N, K] (hi + lo)"""
    v = wp.view(torch.float16).double()
    return v[:, 0] + v[:, 1]


def pack_conv3x3(w, bn):
    """Conv2d weight (Cout, Cin, 3, 3) and its BN (weight, bias, running_mean, running_var, eps) ->
    (pair rows [Cout, 2, 9 Cin] with K = (ky*3 + kx) * Cin + c, fp32 shift [Cout])."""
    if w.dim() != 4 or tuple(w.shape[2:]) != (3, 3):
        raise ValueError(f"expected a (Cout, Cin, 3, 3) conv weight, got {tuple(w.shape)}")
    scale, shift = fold_bn(*bn)
    w64 = w.detach().double() * scale[:, None, None, None]
    return split_pair(w64.permute(0, 2, 3, 1).reshape(w.shape[0], -1)), shift.float().contiguous()


def pack_deblock(w, bn, k, transposed=True):
    """Upsampling weight -> (pair rows [k*k*Cout, 2, Cin], row (dy*k + dx) * Cout + n, fp32 shift [Cout]).
    ``transposed``: a ConvTranspose2d weight (Cin, Cout, k, k); else the 1 x 1 Conv2d weight (Cout, Cin, 1, 1)."""
    k = int(k)
    if w.dim() != 4 or tuple(w.shape[2:]) != (k, k) or (not transposed and k != 1):
        raise ValueError(f"expected a {'(Cin, Cout' if transposed else '(Cout, Cin'}, {k}, {k}) weight, got "
                         f"{tuple(w.shape)}")
    scale, shift = fold_bn(*bn)
    w64 = w.detach().double()
    if transposed:
        rows = (w64 * scale[None, :, None, None]).permute(2, 3, 1, 0).reshape(k * k * w.shape[1], w.shape[0])
    else:
        rows = (w64 * scale[:, None, None, None]).reshape(w.shape[0], w.shape[1])
    return split_pair(rows), shift.float().contiguous()


def out_hw(H, W, stride):
    """3 x 3 / pad 1: (n - 1) // s + 1 per axis"""
    return (int(H) - 1) // stride + 1, (int(W) - 1) // stride + 1


def _pair_rows(name, t, rows, C):
    if t.dtype != torch.uint16 or t.dim() != 3 or t.shape[1] != 2 or t.shape[2] != C or t.shape[0] < rows or \
            not t.is_contiguous():
        raise ValueError(f"{name} must be contiguous split-f16 pair rows uint16 [>= {rows}, 2, {C}], got {t.dtype} "
                         f"{tuple(t.shape)}")


def _shift(shift, Cout):
    if shift.dtype != torch.float32 or shift.dim() != 1 or shift.numel() != Cout or not shift.is_contiguous():
        raise ValueError(f"shift must be contiguous fp32 [{Cout}]")


def _flag(range_flag):
    if range_flag is not None and (range_flag.dtype != torch.int32 or range_flag.numel() != 1):
        raise ValueError("range_flag must be one int32 on the device")


def _conv_checks(X, Wp, shift, B, H, W, Cin, Cout, stride, out, range_flag, cin_mult):
    if min(B, H, W) <= 0:
        raise ValueError(f"B, H and W must be positive, got {(B, H, W)}")
    if stride not in (1, 2):
        raise ValueError(f"stride must be 1 or 2, got {stride}")
    if Cin <= 0 or Cin % cin_mult or Cout <= 0 or Cout % 128:
        raise ValueError(f"Cin must be a multiple of {cin_mult} and Cout of 128, got {Cin} and {Cout}")
    if W > WMAX:
        raise ValueError(f"map width {W} above {WMAX}")
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


def conv3x3(X, Wp, shift, *, B, H, W, Cin, Cout, stride, relu=True, out=None, range_flag=None):
    """cmt_bev_conv3x3: pair rows [B*H*W, 2, Cin] -> pair rows [B*Ho*Wo, 2, Cout] (rows beyond stay untouched)."""
    Ho, Wo = _conv_checks(X, Wp, shift, B, H, W, Cin, Cout, stride, out, range_flag, 32)
    _dev(X, Wp, shift, out, range_flag)
    Y = out if out is not None else torch.empty((B * Ho * Wo, 2, Cout), dtype=torch.uint16, device=X.device)
    a = N.BevConvArgs()
    a.B, a.H, a.W, a.Cin, a.Cout, a.stride, a.relu = B, H, W, Cin, Cout, stride, int(bool(relu))
    a.X, a.ldx, a.Wt, a.ldw, a.shift = _p(X), 2 * Cin, _p(Wp), 18 * Cin, _p(shift)
    a.Y, a.ldy, a.range_flag = _p(Y), 2 * Cout, _p(range_flag)
    _check(lib().cmt_bev_conv3x3(ctypes.byref(a), _stream()), "cmt_bev_conv3x3")
    return Y


def conv3x3_gemm(X, Wp, shift, *, B, H, W, Cin, Cout, relu=True, out=None, range_flag=None):
    """The stride-1 conv of the same contract on cmt_gemm's CMT_A_CONV3X3 pair-row path (batch in M).  Its
    64 x 64 tiles (small maps) need Cin % 64 == 0."""
    _conv_checks(X, Wp, shift, B, H, W, Cin, Cout, 1, out, range_flag, 32)
    _dev(X, Wp, shift, out, range_flag)
    M = B * H * W
    Y = out if out is not None else torch.empty((M, 2, Cout), dtype=torch.uint16, device=X.device)
    N.gemm(X, Wp, Y, M=M, N=Cout, K=9 * Cin, lda=Cin, ldw=9 * Cin, ldc=Cout, bias=shift, relu=relu,
           a_mode=N.A_CONV3X3, conv=(H, W, Cin), range_flag=range_flag)
    return Y


def conv3x3_nchw_gemm(x, Wp, shift, *, Cout, relu=True, out=None, range_flag=None):
    """The stride-1 conv straight from the fp32 NCHW map (cmt_gemm CMT_A_CONV3X3_NCHW) to pair rows."""
    if x.dim() != 4 or x.dtype != torch.float32 or not x.is_contiguous():
        raise ValueError("x must be a contiguous fp32 [B, C, H, W] map")
    B, Cin, H, W = (int(s) for s in x.shape)
    if min(B, H, W) <= 0 or Cin <= 0 or Cin % 16 or Cout <= 0 or Cout % 128:
        raise ValueError(f"a non-empty map with Cin % 16 == 0 and Cout % 128 == 0 required, got {tuple(x.shape)} "
                         f"and Cout {Cout}")
    if W > WMAX:
        raise ValueError(f"map width {W} above {WMAX}")
    _pair_rows("Wp", Wp, Cout, 9 * Cin)
    _shift(shift, Cout)
    _flag(range_flag)
    if out is not None:
        _pair_rows("out", out, B * H * W, Cout)
    _dev(x, Wp, shift, out, range_flag)
    Y = out if out is not None else torch.empty((B * H * W, 2, Cout), dtype=torch.uint16, device=x.device)
    N.gemm(x, Wp, Y, M=H * W, N=Cout, K=9 * Cin, lda=H * W, ldw=9 * Cin, ldc=Cout, bias=shift, relu=relu,
           a_mode=N.A_CONV3X3_NCHW, conv=(H, W, Cin), batch=B, a_bstride=Cin * H * W, c_bstride=H * W * Cout,
           range_flag=range_flag)
    return Y


def to_rows(x, range_flag=None):
    """fp32 NCHW -> RowMap (cmt_nchw_to_rows_ex)"""
    if x.dim() != 4 or x.dtype != torch.float32 or not x.is_contiguous():
        raise ValueError("x must be a contiguous fp32 [B, C, H, W] map")
    _flag(range_flag)
    _dev(x, range_flag)
    B, C, H, W = (int(s) for s in x.shape)
    rows = torch.empty((B * H * W, 2, C), dtype=torch.uint16, device=x.device)
    N.nchw_to_rows(x, rows, nb=B, nv=1, C=C, HW=H * W, ldy=C, rows_per_batch=H * W, range_flag=range_flag)
    return RowMap(rows, (B, C, H, W))


def deblock(X, Wp, shift, out, *, B, H, W, Cin, Cout, k, c0, relu=True, range_flag=None):
    """cmt_bev_deblock: pair rows [B*H*W, 2, Cin] -> channels [c0, c0 + Cout) of the fp32 NCHW ``out``
    [B, Ctot, k H, k W]; the other channels are not touched."""
    if min(B, H, W) <= 0:
        raise ValueError(f"B, H and W must be positive, got {(B, H, W)}")
    if k not in (1, 2, 4):
        raise ValueError(f"k must be 1, 2 or 4, got {k}")
    if Cin <= 0 or Cin % 32 or Cout <= 0 or Cout % 128:
        raise ValueError(f"Cin must be a multiple of 32 and Cout of 128, got {Cin} and {Cout}")
    _pair_rows("X", X, B * H * W, Cin)
    _pair_rows("Wp", Wp, k * k * Cout, Cin)
    if Wp.shape[0] != k * k * Cout:
        raise ValueError(f"Wp must hold k*k*Cout = {k * k * Cout} rows, got {Wp.shape[0]}")
    _shift(shift, Cout)
    _flag(range_flag)
    if out.dtype != torch.float32 or out.dim() != 4 or not out.is_contiguous() or out.shape[0] != B or \
            out.shape[2] != k * H or out.shape[3] != k * W:
        raise ValueError(f"out must be contiguous fp32 [{B}, Ctot, {k * H}, {k * W}], got {out.dtype} "
                         f"{tuple(out.shape)}")
    Ctot = int(out.shape[1])
    if c0 < 0 or c0 + Cout > Ctot:
        raise ValueError(f"channel slice [{c0}, {c0 + Cout}) outside the {Ctot} channels of out")
    _dev(X, Wp, shift, out, range_flag)
    a = N.BevDeblockArgs()
    a.B, a.H, a.W, a.Cin, a.Cout, a.k, a.c0, a.Ctot, a.relu = B, H, W, Cin, Cout, k, c0, Ctot, int(bool(relu))
    a.X, a.ldx, a.Wt, a.ldw, a.shift = _p(X), 2 * Cin, _p(Wp), 2 * Cin, _p(shift)
    a.Y, a.range_flag = _p(out), _p(range_flag)
    _check(lib().cmt_bev_deblock(ctypes.byref(a), _stream()), "cmt_bev_deblock")
    return out
