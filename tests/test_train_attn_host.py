"""The bf16x3 mode of the training attention core without a device: the mode switch
(native_train.set_train_attn, CMT_TRAIN_ATTN), the three additive C symbols on the unchanged
ABI 25 / cmt_attn_train_args, their argument checks (which run before any HIP call), and the
"HIP device" error of train_ops.attention on host tensors."""
import ctypes
import os

import pytest
import torch


def _N():
    from projects.mmdet3d_plugin import native as N
    return N


def _T():
    from projects.mmdet3d_plugin import native_train as T
    return T


SYMBOLS = ("cmt_attn_train_bf16x3_workspace_bytes", "cmt_attn_train_fwd_bf16x3", "cmt_attn_train_bwd_bf16x3")


def test_set_train_attn_round_trip():
    T = _T()
    assert "set_train_attn" in T.__all__
    # the initial mode is the environment's (read once at import), f32 when unset
    assert T.train_attn() == (os.environ.get("CMT_TRAIN_ATTN") or "f32")
    first = T.set_train_attn("bf16x3")
    try:
        assert T.train_attn() == "bf16x3"
        assert T.set_train_attn("f32") == "bf16x3"
        assert T.set_train_attn("f32") == "f32"
        with pytest.raises(ValueError, match="bf16x3.*f32"):
            T.set_train_attn("fp8")
        assert T.train_attn() == "f32"          # a refused mode changes nothing
    finally:
        T.set_train_attn(first)


def test_symbols_on_unchanged_abi():
    N = _N()
    L = N.lib()
    for s in SYMBOLS:
        assert hasattr(L, s), s
    assert L.cmt_abi_version() == 25
    assert L.cmt_attn_train_args_size() == ctypes.sizeof(N.AttnTrainArgs)


def _filled(N, keep):
    """a well-formed struct; the pointers only have to be non-null (every check runs before any HIP call)"""
    B, H, n = 1, 2, 8
    buf = (ctypes.c_float * (B * H * n * 32))()
    keep.append(buf)
    p = ctypes.addressof(buf)
    a = N.AttnTrainArgs()
    a.B, a.H, a.Nq, a.Nk = B, H, n, n
    for x in "qkvo":
        setattr(a, f"{x}_bs", n * H * 32)
        setattr(a, f"{x}_hs", 32)
        setattr(a, f"{x}_rs", H * 32)
    a.Q = a.K = a.V = a.O = a.LSE = p
    a.dO = a.dQ = a.dK = a.dV = a.delta = p
    a.scale = 32 ** -0.5
    return a


@pytest.mark.parametrize("entry", SYMBOLS[1:])
def test_argument_errors_without_device(entry):
    N = _N()
    fn = getattr(N.lib(), entry)
    assert fn(None, None) == 1001
    assert entry in N.lib().cmt_last_error().decode()
    keep = []
    a = _filled(N, keep)
    a.fp16_inputs = 1
    assert fn(ctypes.byref(a), None) == 1001
    msg = N.lib().cmt_last_error().decode()
    assert entry in msg and "fp16_inputs" in msg
    a = _filled(N, keep)
    a.dn_pad, a.dn_group = 4, 0
    assert fn(ctypes.byref(a), None) == 1001
    assert entry in N.lib().cmt_last_error().decode()
    assert N.lib().cmt_attn_train_bf16x3_workspace_bytes(None) == 0


def test_attention_refuses_host_tensors():
    from projects.mmdet3d_plugin.models.utils import train_ops as O
    q = torch.randn(1, 8, 64)
    with pytest.raises(RuntimeError, match="HIP device"):
        O.attention(q, q, q, 2, mode="bf16x3")
