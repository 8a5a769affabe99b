"""Wrappers of the sparse 3-D convolution entry points (include/cmt_hip.h,
cmt_sparse_*): site index, rulebooks, convolution, densify.  Like native.py:
tensors must live on a HIP device, there is no CPU fallback, and no wrapper
synchronises with the host (row counts are int32 tensors on the device).
"""
import ctypes

import torch

from . import native as N
from .native import _check, _dev, _p, _stream, lib

__all__ = ["out_shape", "index_bytes", "build_index", "rulebook_subm", "rulebook_down", "pack_weight", "conv",
           "to_dense", "triple"]


def triple(v):
    """3 -> (3, 3, 3); [0, 1, 1] -> (0, 1, 1)"""
    if isinstance(v, (list, tuple)):
        if len(v) != 3:
            raise ValueError(f"expected 3 values, got {v!r}")
        return tuple(int(x) for x in v)
    return (int(v),) * 3


def out_shape(shape3, kernel, stride, padding):
    """(n + 2p - k) // s + 1 per axis"""
    k, s, p = triple(kernel), triple(stride), triple(padding)
    return tuple((int(n) + 2 * p[i] - k[i]) // s[i] + 1 for i, n in enumerate(shape3))


def index_bytes(grid, cap):
    b = int(lib().cmt_sparse_index_bytes(*[int(g) for g in grid], int(cap)))
    if b <= 0:
        raise ValueError(f"no sparse index for grid {tuple(grid)} with capacity {cap}: extents must be positive and "
                         "B*D*H*W below 2^31")
    return b


def _coors(coors):
    if coors.dtype != torch.int32 or coors.dim() != 2 or coors.shape[1] != 4 or not coors.is_contiguous():
        raise ValueError("coors must be a contiguous int32 [n, 4] tensor (b, z, y, x)")
    _dev(coors)
    return coors


def _rows(name, t, rows, cols):
    """an fp32 operand the kernels index as t[row * stride(0) + col], row < rows, col < cols"""
    if t.dtype != torch.float32 or t.dim() != 2 or t.shape[0] < rows or t.shape[1] < cols or \
            (t.shape[1] > 1 and t.stride(1) != 1) or (t.shape[0] > 1 and t.stride(0) < cols):
        raise ValueError(f"{name} must be fp32 rows [>= {rows}, >= {cols}] with unit column stride, got "
                         f"{t.dtype} {tuple(t.shape)} strides {tuple(t.stride())}")


def _per_channel(name, t, n):
    if t.dtype != torch.float32 or not t.is_contiguous() or t.numel() < n:
        raise ValueError(f"{name} must be contiguous fp32 of at least {n} elements")


def _count(count, dev):
    _dev(count)
    if count.dtype != torch.int32 or count.numel() != 1:
        raise ValueError("count must be one int32 on the device")
    return count


def build_index(coors, count, grid):
    """The site index of ``coors[:count]`` on ``grid`` (B, D, H, W): a uint8 buffer."""
    coors = _coors(coors)
    _count(count, coors.device)
    cap = max(int(coors.shape[0]), 1)
    index = torch.empty((index_bytes(grid, cap),), dtype=torch.uint8, device=coors.device)
    a = N.SparseIndexArgs()
    a.B, a.D, a.H, a.W = [int(g) for g in grid]
    a.n_cap = cap
    a.coors, a.count, a.index, a.index_bytes = _p(coors), _p(count), _p(index), index.numel()
    _check(lib().cmt_sparse_index(ctypes.byref(a), _stream()), "cmt_sparse_index")
    return index


def _rulebook_args(coors, count, index, grid, kernel, stride, padding):
    a = N.SparseRulebookArgs()
    a.B, a.D, a.H, a.W = [int(g) for g in grid]
    k, s, p = triple(kernel), triple(stride), triple(padding)
    for i in range(3):
        a.kernel3[i], a.stride3[i], a.padding3[i] = k[i], s[i], p[i]
    a.K = k[0] * k[1] * k[2]
    a.n_cap = max(int(coors.shape[0]), 1)
    a.coors, a.count, a.index, a.index_bytes = _p(coors), _p(count), _p(index), index.numel()
    return a


def rulebook_subm(coors, count, index, grid, kernel=3):
    """nbr [n, K] int32 of a submanifold convolution (padding kernel // 2)."""
    coors = _coors(coors)
    _dev(index)
    _count(count, coors.device)
    k = triple(kernel)
    a = _rulebook_args(coors, count, index, grid, k, 1, tuple(x // 2 for x in k))
    nbr = torch.empty((a.n_cap, a.K), dtype=torch.int32, device=coors.device)
    a.nbr = _p(nbr)
    _check(lib().cmt_sparse_rulebook_subm(ctypes.byref(a), _stream()), "cmt_sparse_rulebook_subm")
    return nbr[:coors.shape[0]]


def rulebook_down(coors, count, index, grid, kernel, stride, padding, cap):
    """Strided convolution: (out_coors [cap, 4] ascending, out_count [1] (-1: more than cap), nbr [cap, K],
    out_index, out_grid)."""
    coors = _coors(coors)
    _dev(index)
    _count(count, coors.device)
    cap = int(cap)
    a = _rulebook_args(coors, count, index, grid, kernel, stride, padding)
    a.cap = cap
    og = (int(grid[0]),) + out_shape(grid[1:], kernel, stride, padding)
    dev = coors.device
    out_index = torch.empty((index_bytes(og, cap),), dtype=torch.uint8, device=dev)
    out_coors = torch.empty((cap, 4), dtype=torch.int32, device=dev)
    out_count = torch.empty((1,), dtype=torch.int32, device=dev)
    nbr = torch.empty((cap, a.K), dtype=torch.int32, device=dev)
    a.out_index, a.out_index_bytes = _p(out_index), out_index.numel()
    a.out_coors, a.out_count, a.nbr = _p(out_coors), _p(out_count), _p(nbr)
    _check(lib().cmt_sparse_rulebook_down(ctypes.byref(a), _stream()), "cmt_sparse_rulebook_down")
    return out_coors, out_count, nbr, out_index, og


def pack_weight(w):
    """Conv weight (Cout, kD, kH, kW, Cin) fp32 -> the bf16 hi/lo fragment image cmt_sparse_conv reads
    (cmt_hip.h): [K][KC][NB][2][64][8], Cin zero-padded to 16 KC and Cout to 32 NB.  Pure layout + rounding,
    done once per weight version; runs wherever ``w`` lives."""
    Cout, Cin = int(w.shape[0]), int(w.shape[-1])
    K = int(w.shape[1] * w.shape[2] * w.shape[3])
    KC, NB = (Cin + 15) // 16, (Cout + 31) // 32
    wk = w.detach().float().reshape(Cout, K, Cin).permute(1, 2, 0)          # [K][Cin][Cout]
    full = torch.zeros((K, KC * 16, NB * 32), dtype=torch.float32, device=w.device)
    full[:, :Cin, :Cout] = wk
    hi = full.to(torch.bfloat16)
    lo = (full - hi.float()).to(torch.bfloat16)
    img = torch.stack([hi, lo], dim=0)                                       # [2][K][16 KC][32 NB]
    img = img.reshape(2, K, KC, 2, 8, NB, 32)                                # p k kc h j nb r
    img = img.permute(1, 2, 5, 0, 3, 6, 4).contiguous()                      # k kc nb p h r j
    return img.reshape(K, KC, NB, 2, 64, 8)


def conv(X, nbr, count, Wp, scale, shift, *, Cin, Cout, relu=True, R=None, out=None):
    """Y[m] = act(scale * sum_k X[nbr[m][k]] W[k] + shift (+ R[m])) for m < count: fp32 rows [cap, Cout]."""
    if nbr.dim() != 2 or nbr.dtype != torch.int32 or not nbr.is_contiguous():
        raise ValueError("nbr must be a contiguous int32 [rows, K] tensor")
    cap, K = int(nbr.shape[0]), int(nbr.shape[1])
    if X.dtype != torch.float32 or X.dim() != 2 or X.stride(1) != 1 or X.shape[1] < Cin:
        raise ValueError("X must be fp32 rows [n, >= Cin] with unit column stride")
    if X.shape[0] == 0 and nbr.numel() > 0:
        raise ValueError("X has no rows but nbr is not empty")
    if Wp.dtype != torch.bfloat16 or not Wp.is_contiguous():
        raise ValueError("Wp must be the contiguous bf16 image of pack_weight")
    _per_channel("scale", scale, Cout)
    _per_channel("shift", shift, Cout)
    if R is not None:
        _rows("R", R, cap, Cout)
    if out is not None:
        _rows("out", out, cap, Cout)
    _dev(X, nbr, count, Wp, scale, shift, R, out)
    Y = out if out is not None else torch.empty((max(cap, 1), Cout), dtype=torch.float32, device=X.device)
    if cap == 0:
        return Y[:0]
    a = N.SparseConvArgs()
    a.cap, a.n_in_cap, a.Cin, a.Cout, a.K, a.relu = cap, max(int(X.shape[0]), 1), int(Cin), int(Cout), K, int(bool(relu))
    a.X, a.ldx, a.nbr, a.count = _p(X), X.stride(0), _p(nbr), _p(count)
    a.Wp, a.wp_bytes = _p(Wp), Wp.numel() * 2
    a.scale, a.shift = _p(scale), _p(shift)
    if R is not None:
        a.R, a.ldr = _p(R), R.stride(0)
    a.Y, a.ldy = _p(Y), Y.stride(0)
    _check(lib().cmt_sparse_conv(ctypes.byref(a), _stream()), "cmt_sparse_conv")
    return Y[:cap]


def to_dense(X, coors, count, grid, C):
    """Rows -> [B, C * D, H, W] fp32 (zero elsewhere), channel-major then depth as the reference's view."""
    if coors.dim() != 2:
        raise ValueError("coors must be a contiguous int32 [n, 4] tensor (b, z, y, x)")
    _rows("X", X, int(coors.shape[0]), int(C))
    coors = _coors(coors)
    _dev(X, count)
    B, D, H, W = [int(g) for g in grid]
    out = torch.empty((B, C * D, H, W), dtype=torch.float32, device=X.device)
    a = N.SparseDenseArgs()
    a.B, a.D, a.H, a.W, a.C, a.n_cap = B, D, H, W, int(C), max(int(coors.shape[0]), 1)
    a.X, a.ldx, a.coors, a.count, a.out = _p(X), X.stride(0), _p(coors), _p(count), _p(out)
    _check(lib().cmt_sparse_to_dense(ctypes.byref(a), _stream()), "cmt_sparse_to_dense")
    return out
