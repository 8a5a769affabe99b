"""The bf16x3 mode of the training attention core (cmt_attn_train_fwd_bf16x3 / _bwd_bf16x3,
native_train.set_train_attn("bf16x3")) against two float64 CPU computations per case:

(a) the float64 reference: the ref_fn / autograd of test_attention_train_fwd_bwd with its keep_mask
    and dn_mask restatements;
(b) a float64 emulation of the three-pass arithmetic: every product a_lo b_hi + a_hi b_lo + a_hi b_hi
    on bf16 splits (x = hi + lo, hi = bf16(x) RNE, lo = bf16(x - hi)) of the fp32 operands,
    accumulated in float64; P rounded to fp32 before it is split; dS = P (dP - delta) rounded to fp32
    before it is split; the backward written out: dV = P^T dO, dP = dO V^T, delta = rowsum(dO o O),
    dQ = dS K scale, dK = dS^T Q scale.

E is (b)'s error against (a) in the norm of the existing test (outputs: max abs; each gradient: max
abs difference over the float64 gradient's max abs).  The kernels' error against (a) must stay below
2 E + 2e-5 per output and gradient: 2e-5 is the bound the exact-f32 kernels are held to (the fp32
softmax and accumulation), the factor 2 because kernel and emulation round P and dS from slightly
different fp32 values (two draws of one truncation-error distribution).  A single hi*hi pass is at
2e-3 .. 9e-3 on these shapes, E at 3e-6 .. 1.7e-5."""
import contextlib
import ctypes
import functools
import math

import pytest
import torch

from test_gpu_train_edges import Buf, Heads, NAN, _outside_bits
from test_gpu_train_kernels import dn_mask, keep_mask

pytestmark = pytest.mark.gpu

H, C = 8, 256
SEED = 1234
CMT_EWORKSPACE = 1003


def _T():
    from projects.mmdet3d_plugin import native_train as T
    return T


def _N():
    from projects.mmdet3d_plugin import native as N
    return N


def _ops():
    from projects.mmdet3d_plugin.models.utils import train_ops as O
    return O


# ---------------------------------------------------------------------------------------------
# the yardstick, on [B, H, N, 32]
# ---------------------------------------------------------------------------------------------
def _reference(q, k, v, do, pad, grp, p, seed=SEED):
    """(a): float64 autograd; returns o, dq, dk, dv"""
    B, Hh, Nq, _ = q.shape
    Nk = k.shape[2]
    qd, kd, vd = (t.double().requires_grad_() for t in (q, k, v))
    s = qd @ kd.transpose(-1, -2) / math.sqrt(32)
    if pad:
        s = s.masked_fill(dn_mask(Nq, Nk, pad, grp), float("-inf"))
    pr = torch.softmax(s, -1)
    if p > 0:
        pr = pr * keep_mask(seed, B, Hh, Nq, Nk, p).double() / (1 - p)
    out = pr @ vd
    out.backward(do.double())
    return out.detach(), qd.grad, kd.grad, vd.grad


def _split(x):
    x32 = x.float()
    hi = x32.bfloat16().float()
    lo = (x32 - hi).bfloat16().float()       # x32 - hi is exact in fp32
    return hi.double(), lo.double()


def _prod3(a, b):
    ah, al = _split(a)
    bh, bl = _split(b)
    return al @ bh + ah @ bl + ah @ bh


def _emulation(q, k, v, do, pad, grp, p, seed=SEED, passes=3):
    """(b): the three-pass arithmetic in float64 (passes=1: hi*hi alone, for the orientation figures)"""
    B, Hh, Nq, _ = q.shape
    Nk = k.shape[2]
    prod = _prod3 if passes == 3 else (lambda a, b: _split(a)[0] @ _split(b)[0])
    scale = 1 / math.sqrt(32)
    s = prod(q, k.transpose(-1, -2)) * scale
    if pad:
        s = s.masked_fill(dn_mask(Nq, Nk, pad, grp), float("-inf"))
    p32 = torch.softmax(s, -1).float().double()                  # P, rounded to fp32
    keep = keep_mask(seed, B, Hh, Nq, Nk, p).double() if p > 0 else 1.0
    ks = 1 / (1 - p)
    pd = p32 * keep                                              # the kept P (exact), scaled once after
    o = prod(pd, v) * ks
    dv = prod(pd.transpose(-1, -2), do) * ks
    dp = prod(do, v.transpose(-1, -2)) * keep * ks
    delta = (do.double() * o).sum(-1, keepdim=True)
    ds = (p32 * (dp - delta)).float().double()                   # dS, rounded to fp32
    dq = prod(ds, k) * scale
    dk = prod(ds.transpose(-1, -2), q) * scale
    return o, dq, dk, dv


def _errs(got, want):
    """the existing test's norm: output max abs; gradients max abs difference over the float64 maximum"""
    e = [(got[0].double() - want[0]).abs().max().item()]
    e += [(g.double() - w).abs().max().item() / max(w.abs().max().item(), 1e-6) for g, w in zip(got[1:], want[1:])]
    return e


def _heads(t, B, N):
    return t.view(B, N, H, 32).transpose(1, 2)


@functools.lru_cache(maxsize=None)
def _case(B, Nq, Nk, pad, grp, p):
    """inputs [B, N, C] (the generator of test_attention_train_fwd_bwd), the reference and E; computed
    once per shape and shared (read-only) by the tests below"""
    g = torch.Generator().manual_seed(Nq * 7 + Nk)
    q = torch.randn(B, Nq, C, generator=g)
    k = torch.randn(B, Nk, C, generator=g)
    v = torch.randn(B, Nk, C, generator=g)
    do = torch.randn(B, Nq, C, generator=g)
    hq, hk, hv, hd = _heads(q, B, Nq), _heads(k, B, Nk), _heads(v, B, Nk), _heads(do, B, Nq)
    ref = _reference(hq, hk, hv, hd, pad, grp, p)
    E = _errs(_emulation(hq, hk, hv, hd, pad, grp, p), ref)
    return dict(q=q, k=k, v=v, do=do, ref=ref, E=E)


def _run_attention(dev, c, B, Nq, Nk, pad, grp, p, *, mode="bf16x3", do_scale=1.0, seed=SEED, seed_dev=None):
    """train_ops.attention forward + backward; returns (o, dq, dk, dv) on the CPU as [B, H, N, 32]"""
    qg, kg, vg = (c[n].to(dev).requires_grad_() for n in ("q", "k", "v"))
    out = _ops().attention(qg, kg, vg, H, dn_pad=pad, dn_group=grp, dropout_p=p, seed=seed, seed_dev=seed_dev,
                           mode=mode)
    out.backward((c["do"] * do_scale).to(dev))
    torch.cuda.synchronize()
    return (_heads(out.detach().cpu(), B, Nq), _heads(qg.grad.cpu(), B, Nq), _heads(kg.grad.cpu(), B, Nk),
            _heads(vg.grad.cpu(), B, Nk))


NAMES = ("o", "dq", "dk", "dv")

# Split rules: forward key splits double while the grid is below 512 workgroups and a split keeps >= 4
# tiles (the exact-f32 rule); dQ key splits min(tiles / 2, 432 / workgroups); dK / dV query splits
# min(query tiles / 2, 288 / workgroups), workgroups = ceil(N / 128) B H.  With H = 8:
CASES = [
    (1, 100, 1000, 0, 0, 0.0),      # ragged query block and last key tile (40 keys); forward 4 splits + combine, dQ 8 splits
    (2, 70, 70, 30, 10, 0.0),       # two batch elements, DN mask, one full + one 6-row tile; no split
    (1, 140, 140, 40, 8, 0.25),     # mask + dropout, dn_pad no tile multiple, groups straddling the 4-row runs
    (1, 33, 65, 0, 0, 0.0),         # one query past a 32-row wave, one key past a tile
    (1, 300, 300, 60, 20, 0.1),     # the smallest shape with dQ key splits (2) and dK / dV query splits (2) above 1
    (2, 1100, 1100, 200, 20, 0.1),  # the coop self-attention: forward 4 splits, dQ 3, dK / dV 2 (18 tiles each way)
]


@pytest.mark.parametrize("B,Nq,Nk,pad,grp,p", CASES)
def test_attention_x3_fwd_bwd(dev, parity_log, B, Nq, Nk, pad, grp, p):
    c = _case(B, Nq, Nk, pad, grp, p)
    got = _run_attention(dev, c, B, Nq, Nk, pad, grp, p)
    errs = _errs(got, c["ref"])
    parity_log.append(f"attn_train bf16x3 B={B} {Nq}x{Nk} dn {pad}/{grp} p={p}: kernel o/dq/dk/dv "
                      + "/".join(f"{e:.2e}" for e in errs) + "; three-pass emulation E "
                      + "/".join(f"{e:.2e}" for e in c["E"]) + " (bound 2 E + 2e-5)")
    for n, e, E in zip(NAMES, errs, c["E"]):
        assert e < 2 * E + 2e-5, (n, e, E)


def test_attention_x3_exponent_range(dev, parity_log):
    """dO scaled by 2^-40: bf16 keeps the fp32 exponent, so every gradient keeps its relative error
    (an f16 pair loses operands below ~6e-5) and equals 2^-40 times the unscaled run's up to the fp32
    re-association of the split sums (1e-5, the figure of test_attention_train_bwd_reuses_forward_copies)."""
    case = CASES[2]
    c = _case(*case)
    sc = 2.0 ** -40
    base = _run_attention(dev, c, *case)
    got = _run_attention(dev, c, *case, do_scale=sc)
    # the reference's gradients are linear in dO: each scaled gradient against its own scaled float64
    # gradient is the gradient times 2^40 (exact) against the unscaled one
    errs = _errs((got[0],) + tuple(g.double() / sc for g in got[1:]), c["ref"])
    rel = [((g.double() - b.double() * sc).abs().max() / (b.double() * sc).abs().max()).item()
           for g, b in zip(got[1:], base[1:])]
    parity_log.append("attn_train bf16x3 dO x 2^-40 (case 3): dq/dk/dv vs float64 "
                      + "/".join(f"{e:.2e}" for e in errs[1:]) + ", vs 2^-40 x the unscaled run "
                      + "/".join(f"{e:.2e}" for e in rel) + " (1e-5)")
    for n, e, E in zip(NAMES, errs, c["E"]):
        assert e < 2 * E + 2e-5, (n, e, E)
    for n, e in zip(NAMES[1:], rel):
        assert e < 1e-5, (n, e)


def _raw_args(dev, q, k, v, do, *, pad, grp, p, kv_splits, seed=SEED):
    """Q / K / V: column slices of ONE NaN-filled [B, N, 3C] parent; O, dQ, dK, dV (and dO): slices of
    NaN-filled [B, N, 3C] parents of their own (a gap between rows, a guard tail)"""
    N = _N()
    B, Hh, Nq, _ = q.shape
    Nk = k.shape[2]
    assert Nq == Nk
    qkv = Heads(dev, B, Hh, Nq, 0).flat
    Q, K, V = (Heads(dev, B, Hh, Nq, i, src=t, arena=qkv) for i, t in enumerate((q, k, v)))
    dO, O = Heads(dev, B, Hh, Nq, 1, src=do), Heads(dev, B, Hh, Nq, 2)
    dQ, dK, dV = Heads(dev, B, Hh, Nq, 0), Heads(dev, B, Hh, Nk, 1), Heads(dev, B, Hh, Nk, 2)
    lse, delta = Buf(dev, 1, B * Hh * Nq), Buf(dev, 1, B * Hh * Nq)
    groups = [(qkv, [Q.view, K.view, V.view])] + [(t.flat, [t.view]) for t in (dO, O, dQ, dK, dV)]
    a = N.AttnTrainArgs()
    a.B, a.H, a.Nq, a.Nk = B, Hh, Nq, Nk
    a.Q, (a.q_bs, a.q_hs, a.q_rs) = Q.ptr, Q.strides
    a.K, (a.k_bs, a.k_hs, a.k_rs) = K.ptr, K.strides
    a.V, (a.v_bs, a.v_hs, a.v_rs) = V.ptr, V.strides
    a.O, (a.o_bs, a.o_hs, a.o_rs) = O.ptr, O.strides
    assert dO.strides == O.strides and dQ.strides == Q.strides and dK.strides == K.strides and dV.strides == V.strides
    a.LSE = lse.ptr
    a.scale, a.dn_pad, a.dn_group = 1 / math.sqrt(32), pad, grp
    a.fp16_inputs, a.dropout_p, a.seed, a.kv_splits = 0, p, seed, kv_splits
    a.dO, a.dQ, a.dK, a.dV, a.delta = dO.ptr, dQ.ptr, dK.ptr, dV.ptr, delta.ptr
    return a, dict(O=O, dQ=dQ, dK=dK, dV=dV, lse=lse, delta=delta, groups=groups)


def _raw_inputs(B, Hh, n):
    g = torch.Generator().manual_seed(n * 7 + n + Hh)
    return tuple(torch.randn(B, Hh, n, 32, generator=g) for _ in range(4))


def test_attention_x3_strides_and_guards(dev, parity_log):
    """raw struct, explicit kv_splits = 3 at Nk = 300 (tiles per split 2, 2, 1; the last tile 44 keys)"""
    N = _N()
    B, Hh, n, pad, grp, p = 2, 3, 300, 60, 20, 0.1
    q, k, v, do = _raw_inputs(B, Hh, n)
    ref = _reference(q, k, v, do, pad, grp, p)
    E = _errs(_emulation(q, k, v, do, pad, grp, p), ref)
    a, t = _raw_args(dev, q, k, v, do, pad=pad, grp=grp, p=p, kv_splits=3)
    before = [_outside_bits(f, vs) for f, vs in t["groups"]]
    need = N.lib().cmt_attn_train_bf16x3_workspace_bytes(ctypes.byref(a))
    assert need == 3 * B * Hh * n * 34 * 4
    ws = torch.full((need // 4 + Buf.TAIL,), NAN, dtype=torch.float32, device=dev)
    a.workspace, a.workspace_bytes = ws.data_ptr(), need
    for entry in ("cmt_attn_train_fwd_bf16x3", "cmt_attn_train_bwd_bf16x3"):
        N._check(getattr(N.lib(), entry)(ctypes.byref(a), N._stream()), entry)
    torch.cuda.synchronize()
    for (f, vs), b4 in zip(t["groups"], before):
        assert torch.equal(_outside_bits(f, vs), b4), "attention: gap or guard tail written"
    t["lse"].check_gaps("LSE")
    t["delta"].check_gaps("delta")
    assert torch.isnan(ws[need // 4:]).all(), "workspace overrun"
    assert torch.isfinite(t["lse"].cpu()).all()
    errs = _errs([t[x].cpu() for x in ("O", "dQ", "dK", "dV")], ref)
    parity_log.append(f"attn_train bf16x3 raw struct, arena slices, kv_splits=3 B={B} H={Hh} {n}x{n}: kernel "
                      + "/".join(f"{e:.2e}" for e in errs) + "; E " + "/".join(f"{e:.2e}" for e in E))
    for nm, e, Eo in zip(NAMES, errs, E):
        assert e < 2 * Eo + 2e-5, (nm, e, Eo)


def test_attention_x3_workspace_too_small(dev):
    N = _N()
    q, k, v, do = _raw_inputs(1, 2, 300)
    a, t = _raw_args(dev, q, k, v, do, pad=0, grp=0, p=0.0, kv_splits=3)
    need = N.lib().cmt_attn_train_bf16x3_workspace_bytes(ctypes.byref(a))
    ws = torch.empty(need, dtype=torch.uint8, device=dev)
    a.workspace, a.workspace_bytes = ws.data_ptr(), need - 4
    assert N.lib().cmt_attn_train_fwd_bf16x3(ctypes.byref(a), N._stream()) == CMT_EWORKSPACE
    assert "cmt_attn_train_fwd_bf16x3" in N.lib().cmt_last_error().decode()
    a.workspace = None
    assert N.lib().cmt_attn_train_fwd_bf16x3(ctypes.byref(a), N._stream()) == CMT_EWORKSPACE
    torch.cuda.synchronize()
    assert torch.isnan(t["O"].view).all(), "the refused forward launched"


def test_attention_x3_seed_dev_and_split_determinism(dev):
    """seed + *seed_dev is the seed (a shape without forward splits: bitwise the same O); the split
    forward's combine has no atomics: two runs are bitwise equal"""
    case = CASES[2]
    c = _case(*case)
    word = torch.tensor([234], dtype=torch.int32, device=dev)
    o0 = _run_attention(dev, c, *case, seed=1234)[0]
    o1 = _run_attention(dev, c, *case, seed=1000, seed_dev=word)[0]
    assert torch.equal(o0, o1)
    assert not torch.equal(o0, _run_attention(dev, c, *case, seed=1000)[0])
    B, Nq, Nk = 1, 100, 1000                                           # 4 forward key splits
    g = torch.Generator().manual_seed(11)
    q, k, v = (torch.randn(B, n, C, generator=g).to(dev) for n in (Nq, Nk, Nk))
    with torch.no_grad():
        r0 = _ops().attention(q, k, v, H, dropout_p=0.1, seed=7, mode="bf16x3")
        r1 = _ops().attention(q, k, v, H, dropout_p=0.1, seed=7, mode="bf16x3")
    torch.cuda.synchronize()
    assert torch.equal(r0, r1) and torch.isfinite(r0).all()


def test_attention_default_mode_untouched(dev):
    """With the mode at "f32", output and gradients are bitwise those of a run made before the bf16x3
    mode ran: the switch leaves no state behind.  (The first f32 run here may follow bf16x3 runs of
    other tests; both orders are compared.)"""
    T = _T()
    case = CASES[1]
    c = _case(*case)
    assert T.train_attn() == "f32"
    before = _run_attention(dev, c, *case, mode=None)
    old = T.set_train_attn("bf16x3")
    try:
        x3 = _run_attention(dev, c, *case, mode=None)
    finally:
        T.set_train_attn(old)
    after = _run_attention(dev, c, *case, mode=None)
    explicit = _run_attention(dev, c, *case, mode="f32")
    for b, a, e in zip(before, after, explicit):
        assert torch.equal(b, a) and torch.equal(b, e)
    # the global mode did select the other arithmetic in between
    assert torch.equal(x3[0], _run_attention(dev, c, *case, mode="bf16x3")[0])
    assert not torch.equal(x3[0], before[0])


@pytest.mark.parametrize("name,variant,coop", [("cmt_lidar_nus", "lidar", False), ("cmt_fusion_nus", "fusion", False),
                                               ("cmtcoop_fusion_tumtraf", "fusion", True)])
def test_training_step_x3_attention(dev, parity_log, monkeypatch, name, variant, coop):
    """The head's training step with the bf16x3 GEMMs AND the bf16x3 attention core (fp32 cross core, so
    the mode governs the cross-attention too) against the float64 oracle at the bf16x3 step's own
    bounds; the binding's call sites are counted: L self-attention and L x agents cross-attention
    calls each way on the bf16x3 entry points, none on the exact-f32 ones -- and none at all on the
    bf16x3 ones with the mode at "f32"."""
    from test_gpu_train_head import GRAD_BOUND, _run
    T = _T()
    L, agents = 2, 2 if coop else 1
    calls = []
    real = T._attn_call

    def counting(entry, a):
        calls.append((entry, a.Nq == a.Nk, a.fp16_inputs))
        return real(entry, a)
    monkeypatch.setattr(T, "_attn_call", counting)

    @contextlib.contextmanager
    def x3_attn():
        old = T.set_train_attn("bf16x3")
        try:
            yield
        finally:
            T.set_train_attn(old)

    def count(entry, self_attn):
        return sum(1 for e, s, _ in calls if e == entry and s == self_attn)

    # the backward runs after native_ctx has restored "f32": it takes the mode its forward recorded
    lerr, gerr, worst, _ = _run(name, variant, dev, parity_log, fp16=False, L=L, coop=coop, gemm="bf16x3",
                                native_ctx=x3_attn, label=" [bf16x3 attention core]")
    assert T.train_attn() == "f32"
    assert all(f == 0 for _, _, f in calls)
    for entry in ("cmt_attn_train_fwd_bf16x3", "cmt_attn_train_bwd_bf16x3"):
        assert count(entry, True) == L, (entry, calls)
        assert count(entry, False) == L * agents, (entry, calls)
    assert not [e for e, _, _ in calls if e in ("cmt_attn_train_fwd", "cmt_attn_train_bwd")]
    assert lerr < 2e-4
    assert gerr < GRAD_BOUND["bf16x3"], worst
    del calls[:]
    _run(name, variant, dev, [], fp16=False, L=L, coop=coop, gemm="bf16x3")
    assert len(calls) == 2 * (L + L * agents)
    assert not [e for e, _, _ in calls if e.endswith("bf16x3")]
