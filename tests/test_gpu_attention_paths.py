"""Every attention-forward kernel family at the smallest shape that reaches its
edge cases, pinning the pieces the families share in csrc/attention.hip (the
workgroup prologue, the ragged-tile mask, the V^T fragment, the write of a
finished row, the KW merge): against float64, every output form against the
fp32 output, and NaN guard rows after row Nq of each batch.

  attn_kw_kernel       Nq 33, Nk 65, kv_splits 0: two key tiles, the second of one key, six
                       waves without tiles, a second query block with one live row
  attn_fwd_kernel      Nq 129, Nk 65, kv_splits 1 / 2: a second workgroup with one live query,
                       direct write and partials + combine
  attn_pb2_kernel      Nq 129, Nk 4097, kv_splits 1 / 3: 64 full tiles and a ragged one of one key,
                       the last query block has one live wave; with and without kmax2
  attn_fwd_f32_kernel  Nq 33, Nk 65, kv_splits 1 / 2
  attn_kw_pair_kernel  Nq 33, Nk 33: 32-key tiles, a ragged one of one key
Every call goes through the C ABI."""
import functools
import math

import pytest
import torch

from test_gpu_split import SPLIT, _kmax2, _pair, _pair_heads, _same

pytestmark = pytest.mark.gpu

B, H, G = 2, 2, 3            # G guard rows after the Nq rows of each batch
C = H * 32
SCALE = 1 / math.sqrt(32)
NAN = float("nan")
TOL = {torch.float32: 2e-5, torch.float16: 3e-3, torch.bfloat16: 2e-2}
LOWP = [torch.float16, torch.bfloat16]


@pytest.fixture(scope="module")
def N():
    from projects.mmdet3d_plugin import native
    native.lib()
    return native


def _ref64(q, k, v):
    """[B, H, n, 32] -> float64 softmax(q k^T / sqrt(32)) v as [B, Nq, C]."""
    s = (q.double() @ k.double().transpose(-1, -2)) * SCALE
    o = torch.softmax(s, -1) @ v.double()
    return o.permute(0, 2, 1, 3).reshape(q.shape[0], q.shape[2], C)


@functools.lru_cache(maxsize=None)
def _case(dt, Nq, Nk):
    """Seeded operands in dt and their float64 result, computed once per (dt, shape)."""
    g = torch.Generator().manual_seed(1000 * Nq + Nk)
    q = (torch.randn(B, H, Nq, 32, generator=g) * 1.5).to(dt)
    k = (torch.randn(B, H, Nk, 32, generator=g) * 1.5).to(dt)
    v = torch.randn(B, H, Nk, 32, generator=g).to(dt)
    return q, k, v, _ref64(q, k, v)


def _launch(N, dev, q, k, v, Nq, Nk, odt, **kw):
    """One launch into a NaN-filled [B, Nq + G, ...] buffer: the Nq written rows of each batch
    (CPU), after checking that they are finite and that the guard rows are still NaN."""
    if odt == SPLIT:
        O = torch.full((B, Nq + G, 2, C), NAN, dtype=torch.float16, device=dev).view(SPLIT)
    else:
        O = torch.full((B, Nq + G, C), NAN, dtype=odt, device=dev)
    es = 64 if q.dtype == SPLIT else 32            # 16-bit elements of a pair row: 32 hi, 32 lo
    N.attention(q, k, v, O, B=B, H=H, Nq=Nq, Nk=Nk, q_strides=(H * Nq * es, Nq * es, es),
                k_strides=(H * Nk * es, Nk * es, es), v_strides=(H * Nk * es, Nk * es, es),
                o_strides=((Nq + G) * C, C), scale=SCALE, **kw)
    torch.cuda.synchronize()
    o = O.cpu()
    f = (o.view(torch.float16) if odt == SPLIT else o).float()
    assert torch.isnan(f[:, Nq:]).all(), "rows past Nq were written"
    assert torch.isfinite(f[:, :Nq]).all(), "a row below Nq was not written"
    return o[:, :Nq].contiguous()


def _check_forms(N, dev, dt, Nq, Nk, **kw):
    """fp32 output against float64; f16 / bf16 / pair outputs and round_output against it."""
    q, k, v, ref = _case(dt, Nq, Nk)
    qd, kd, vd = q.to(dev), k.to(dev), v.to(dev)
    o32 = _launch(N, dev, qd, kd, vd, Nq, Nk, torch.float32, **kw)
    err = (o32.double() - ref).abs().max().item()
    print(f"{dt} {Nq}x{Nk} {kw.get('kv_splits')} fold={kw.get('fold_scale')}: max abs err {err:.3e} "
          f"(bound {TOL[dt]:.0e})")
    assert err < TOL[dt], err
    for odt in LOWP:
        assert torch.equal(_launch(N, dev, qd, kd, vd, Nq, Nk, odt, **kw), o32.to(odt)), odt
    op = _launch(N, dev, qd, kd, vd, Nq, Nk, SPLIT, **kw)
    assert _same(op, _pair(o32))
    rounded = _launch(N, dev, qd, kd, vd, Nq, Nk, torch.float32, round_output=True, **kw)
    # the exact-f32 kernel has no narrower compute dtype to round to
    assert torch.equal(rounded, o32 if dt == torch.float32 else o32.to(dt).float())


@pytest.mark.parametrize("fold", [False, True])
@pytest.mark.parametrize("dt", LOWP)
def test_kw_path(N, dev, dt, fold):
    _check_forms(N, dev, dt, 33, 65, kv_splits=0, fold_scale=fold)


@pytest.mark.parametrize("fold", [False, True])
@pytest.mark.parametrize("splits", [1, 2])
@pytest.mark.parametrize("dt", LOWP)
def test_fwd_path(N, dev, dt, splits, fold):
    _check_forms(N, dev, dt, 129, 65, kv_splits=splits, fold_scale=fold)


@pytest.mark.parametrize("fold", [False, True])
@pytest.mark.parametrize("splits", [1, 3])
@pytest.mark.parametrize("dt", LOWP)
def test_pb2_path(N, dev, dt, splits, fold):
    _check_forms(N, dev, dt, 129, 4097, kv_splits=splits, fold_scale=fold)


@pytest.mark.parametrize("fold", [False, True])
@pytest.mark.parametrize("splits", [1, 3])
def test_pb2_path_bounded_f16(N, dev, splits, fold):
    """The same launches with the K max-norm partials: fixed softmax offsets."""
    km = _kmax2(_case(torch.float16, 129, 4097)[1], B, 4097, H).to(dev)
    _check_forms(N, dev, torch.float16, 129, 4097, kv_splits=splits, fold_scale=fold, kmax2=km, kmax_ld=H,
                 kmax_plane0=0)


@pytest.mark.parametrize("splits", [1, 2])
def test_f32_path(N, dev, splits):
    _check_forms(N, dev, torch.float32, 33, 65, kv_splits=splits)


def test_pair_path(N, dev):
    Nq = Nk = 33
    g = torch.Generator().manual_seed(33)
    q, k, v = (torch.randn(B * Nq, C, generator=g) for _ in range(3))
    heads = lambda x: x.view(B, Nq, H, 32).transpose(1, 2)   # noqa: E731
    ref = _ref64(heads(q), heads(k), heads(v))
    qp, kp, vp = (_pair_heads(x, B, Nq, H).to(dev) for x in (q, k, v))
    o32 = _launch(N, dev, qp, kp, vp, Nq, Nk, torch.float32)
    err = (o32.double() - ref).abs().max().item()
    tol = 4e-6 * ref.abs().max().item() + 1e-6
    print(f"pair {Nq}x{Nk}: max abs err {err:.3e} (bound {tol:.3e})")
    assert err <= tol, (err, tol)
    assert _same(_launch(N, dev, qp, kp, vp, Nq, Nk, SPLIT), _pair(o32))
