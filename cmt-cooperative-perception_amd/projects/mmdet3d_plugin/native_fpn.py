"""Wrappers of the camera neck's entry points (include/cmt_hip.h, cmt_fpn_lateral and cmt_rows_to_nchw)
and the 1 x 1 weight packing.  Like native_bev.py: argument checks raise ValueError before the device
check, tensors must live on a HIP device, there is no CPU fallback, no wrapper synchronises with the
host.  The packing reuses native_bev's float64 BN fold and f16 hi / lo split.
"""
import ctypes

import torch

from . import native as N
from .native import _check, _dev, _p, _stream, lib
from .native_bev import RowMap, _flag, _pair_rows, _shift, fold_bn, pack_conv3x3, split_pair
from .native_img import FP16, PAIR, _bind

__all__ = ["lateral", "rows_to_nchw", "rows_to_nchw_f16", "pack_conv1x1", "pack_conv3x3_bias", "nearest_index"]


def _is_bn(bias_or_bn):
    return isinstance(bias_or_bn, (list, tuple))


def pack_conv1x1(w, bias_or_bn):
    """Conv2d weight (Cout, Cin, 1, 1) -> (pair rows [Cout, 2, Cin], fp32 shift [Cout]).  ``bias_or_bn``: the
    conv's bias [Cout] (a conv without a norm; None: zero), or the BN that follows a bias-free conv as
    (weight, bias, running_mean, running_var, eps), folded in float64 (W' = scale * W, shift)."""
    if w.dim() != 4 or tuple(w.shape[2:]) != (1, 1):
        raise ValueError(f"expected a (Cout, Cin, 1, 1) conv weight, got {tuple(w.shape)}")
    w64 = w.detach().double().reshape(w.shape[0], w.shape[1])
    if _is_bn(bias_or_bn):
        scale, shift = fold_bn(*bias_or_bn)
        w64 = w64 * scale[:, None]
    elif bias_or_bn is None:
        shift = torch.zeros(w.shape[0], dtype=torch.float64, device=w.device)
    else:
        if tuple(bias_or_bn.shape) != (w.shape[0],):
            raise ValueError(f"expected a bias of {w.shape[0]} values, got {tuple(bias_or_bn.shape)}")
        shift = bias_or_bn.detach().double()
    return split_pair(w64), shift.float().contiguous()


def pack_conv3x3_bias(w, bias_or_bn):
    """pack_conv3x3 with the same second argument as pack_conv1x1: a bias is the shift of an identity BN"""
    if _is_bn(bias_or_bn):
        return pack_conv3x3(w, bias_or_bn)
    one = torch.ones(w.shape[0], dtype=torch.float64, device=w.device)
    bias = torch.zeros_like(one) if bias_or_bn is None else bias_or_bn
    if tuple(bias.shape) != (w.shape[0],):
        raise ValueError(f"expected a bias of {w.shape[0]} values, got {tuple(bias.shape)}")
    return pack_conv3x3(w, [one, bias, torch.zeros_like(one), one, 0.0])


def nearest_index(out_size, in_size):
    """The source index of every output index of F.interpolate(mode='nearest', size=out_size) along one axis,
    as the kernel computes it: min(floor(fp32(dst) * fp32(in / out)), in - 1) with one fp32 multiply."""
    scale = torch.tensor(float(in_size), dtype=torch.float32) / torch.tensor(float(out_size), dtype=torch.float32)
    dst = torch.arange(int(out_size), dtype=torch.float32)
    return torch.clamp(torch.floor(dst * scale).to(torch.int64), max=int(in_size) - 1)


def lateral(x, Wp, shift, *, Cout, top=None, top_hw=None, relu=False, out=None, range_flag=None):
    """cmt_fpn_lateral: the 1 x 1 conv of the fp32 NCHW map ``x`` [B, Cin, H, W] plus the nearest-upsampled
    coarser level ``top`` (pair rows [B*Ht*Wt, 2, Cout] with ``top_hw`` = (Ht, Wt); None: no top-down term)
    -> pair rows [B*H*W, 2, Cout] (rows beyond stay untouched).  ``relu`` acts before the add."""
    if x.dim() != 4 or x.dtype != torch.float32 or not x.is_contiguous():
        raise ValueError("x must be a contiguous fp32 [B, C, H, W] map")
    B, Cin, H, W = (int(s) for s in x.shape)
    if min(B, H, W) <= 0 or Cin <= 0 or Cin % 16 or Cout <= 0 or Cout % 128:
        raise ValueError(f"a non-empty map with Cin % 16 == 0 and Cout % 128 == 0 required, got {tuple(x.shape)} "
                         f"and Cout {Cout}")
    _pair_rows("Wp", Wp, Cout, Cin)
    if Wp.shape[0] != Cout:
        raise ValueError(f"Wp must hold {Cout} rows, got {Wp.shape[0]}")
    _shift(shift, Cout)
    _flag(range_flag)
    Ht = Wt = 0
    if (top is None) != (top_hw is None):
        raise ValueError("top and top_hw go together")
    if top is not None:
        Ht, Wt = (int(s) for s in top_hw)
        if not (1 <= Ht <= H and 1 <= Wt <= W):
            raise ValueError(f"the coarser map {(Ht, Wt)} must be non-empty and no larger than {(H, W)}")
        _pair_rows("top", top, B * Ht * Wt, Cout)
    if out is not None:
        _pair_rows("out", out, B * H * W, Cout)
    _dev(x, Wp, shift, top, out, range_flag)
    L = out if out is not None else torch.empty((B * H * W, 2, Cout), dtype=torch.uint16, device=x.device)
    a = N.FpnLateralArgs()
    a.B, a.H, a.W, a.Cin, a.Cout, a.Htop, a.Wtop, a.relu = B, H, W, Cin, Cout, Ht, Wt, int(bool(relu))
    a.X, a.x_bstride, a.Wt, a.ldw, a.shift = _p(x), Cin * H * W, _p(Wp), 2 * Cin, _p(shift)
    a.T, a.ldt, a.L, a.ldl, a.range_flag = _p(top), 2 * Cout, _p(L), 2 * Cout, _p(range_flag)
    _check(lib().cmt_fpn_lateral(ctypes.byref(a), _stream()), "cmt_fpn_lateral")
    return L


def _rows_to_nchw(fmt, rows, shape, out=None):
    """cmt_rows_to_nchw[_f16]: rows of width C of the map ``shape`` = (B, C, H, W) -> contiguous fp32 NCHW.
    ``rows_to_nchw``: pair rows [B*H*W, 2, C], bit-equal to RowMap.nchw(); ``rows_to_nchw_f16``: fp16 rows
    [B*H*W, C] (the image backbone's one-pass policy), every value widened exactly"""
    if isinstance(rows, RowMap):
        raise ValueError("pass RowMap.rows and RowMap.shape")
    B, C, H, W = (int(s) for s in shape)
    if min(B, H, W) <= 0 or C <= 0 or C % 8:
        raise ValueError(f"a non-empty map with C % 8 == 0 required, got {(B, C, H, W)}")
    if not torch.is_tensor(rows):
        raise ValueError(f"rows must be {fmt.what}, got {type(rows)}")
    fmt.check("rows", rows, B * H * W, C)
    if out is not None and (out.dtype != torch.float32 or tuple(out.shape) != (B, C, H, W) or not out.is_contiguous()):
        raise ValueError(f"out must be contiguous fp32 {(B, C, H, W)}, got {out.dtype} {tuple(out.shape)}")
    _dev(rows, out)
    Y = out if out is not None else torch.empty((B, C, H, W), dtype=torch.float32, device=rows.device)
    a = N.RowsToNchwArgs()
    a.B, a.C, a.HW, a.reserved = B, C, H * W, 0
    a.X, a.ldx, a.Y = _p(rows), fmt.words * C, _p(Y)
    name = "cmt_rows_to_nchw" + fmt.suffix
    _check(getattr(lib(), name)(ctypes.byref(a), _stream()), name)
    return Y


rows_to_nchw, rows_to_nchw_f16 = _bind(_rows_to_nchw, PAIR), _bind(_rows_to_nchw, FP16)
