"""The task heads' first conv inside the split chain B2 (cmt_chain_args.Wh, OPTIONS.chain_heads):
the kernel against float64, against the same call without head weights, against the GEMM launch it
replaces, and the head with the option on and off."""
import pytest
import torch

from projects.mmdet3d_plugin.runtime import options
from test_gpu_split import SPLIT, _pair, _unpair

pytestmark = pytest.mark.gpu

KEYS = ("center", "height", "dim", "rot", "vel", "cls_logits")

# (B, Nq, last, head_cols): a ragged last row block (8, 2 and 1 live rows), rows crossing a batch edge,
# a last layer (1 + HP workgroups per row block) and an inner one (3 + HP), a half-empty (384), a
# nearly empty (64) and an exactly full (512) tail head block
CASES = [(1, 40, False, 384), (2, 33, True, 384), (1, 32, True, 64), (1, 65, False, 512)]


@pytest.fixture(scope="module")
def N():
    from projects.mmdet3d_plugin import native
    native.lib()
    return native


def _ln(x, w, b, eps=1e-5):
    m = x.mean(-1, keepdim=True)
    v = ((x - m) ** 2).mean(-1, keepdim=True)
    return (x - m) / torch.sqrt(v + eps) * w + b


_RUNS = {}


def _case(N, dev, case):
    """Chains B1 and B2 of one case, built like test_chain_b's SPLIT case, run once and shared:
    B2 without head weights (writing OUT16), with them (H1 pre-filled with NaN), and with them after
    a NaN was planted in one partial; plus the float64 / float32 references of H1."""
    if case in _RUNS:
        return _RUNS[case]
    B, Nq, last, cols = case
    g = torch.Generator().manual_seed(B * 1000 + Nq + cols)
    C, F, rows = 256, 1024, B * Nq
    rn = lambda *s: torch.randn(*s, generator=g)
    X, R, P = _pair(rn(rows, C)), rn(rows, C), rn(rows, C)
    Wo, W1, W2, Wn = _pair(rn(C, C) / 16), _pair(rn(F, C) / 16), _pair(rn(C, F) / 32), _pair(rn(3 * C, C) / 16)
    Wh = _pair(rn(cols, C) / 16)
    v = lambda n, s=0.1: rn(n) * s
    bo, b1, b2, bn = v(C), v(F), v(C), v(3 * C)
    l1w, l2w, pw = (1 + v(C) for _ in range(3))
    l1b, l2b, pb = v(C), v(C), v(C)
    prm = torch.cat([bo, l1w, l1b, b1, b2, l2w, l2b, pw, pb, torch.zeros(3 * C) if last else bn]).to(dev)
    WS = torch.full((N.chain_ws_numel(rows),), float("nan"), device=dev)
    Y1 = torch.empty(rows, C, device=dev)
    N.chain(1, X.to(dev), None, prm, N.pack_chain_pair(Wo.to(dev)), N.pack_chain_pair(W1.to(dev)), Y1, rows=rows,
            Nq=Nq, eps=1e-5, R=R.to(dev), W2=N.pack_chain_fc2_pair(W2.to(dev)), WS=WS)
    wn = None if last else N.pack_chain_pair(Wn.to(dev))
    wh = N.pack_chain_heads(Wh.to(dev))
    Pd = None if last else P.to(dev)

    def b2_run(ws, heads, out16):
        Y = torch.full((rows, C), float("nan"), device=dev)
        OUT = torch.full((rows, C), float("nan"), device=dev)
        QKV = None if last else torch.zeros(B * 24 * Nq * 64, dtype=SPLIT, device=dev)
        O16 = torch.zeros((rows, 2, C), dtype=SPLIT, device=dev) if out16 else None
        H1 = torch.full((rows, cols), float("nan"), device=dev) if heads else None
        kw = dict(Wh=wh, H1=H1, head_cols=cols) if heads else {}
        N.chain(2, None, Pd, prm, None, None, Y, rows=rows, Nq=Nq, eps=1e-5, Wn=wn, OUT=OUT,
                out_flags=N.LN_NAN_TO_NUM, Q=QKV, WS=ws, OUT16=O16, **kw)
        return dict(Y=Y, OUT=OUT, QKV=QKV, OUT16=O16, H1=H1)

    plain = b2_run(WS, False, True)
    heads = b2_run(WS, True, False)
    # the parent's launch on the pair copy the head-less call wrote
    Hg = torch.full((rows, cols), float("nan"), device=dev)
    N.gemm(plain["OUT16"], Wh.to(dev), Hg, M=rows, N=cols, K=C, lda=C, ldw=C, ldc=cols, batch=1)
    # a NaN in partial 0, first value of row block 0 / wave 0 / lane 0: row 0 (rowchain_common.h load_tile)
    WSn = WS.clone()
    WSn[0] = float("nan")
    nan_heads = b2_run(WSn, True, False)
    nan_plain = b2_run(WSn, False, True)
    torch.cuda.synchronize()

    def ref(fdt):
        d = lambda t: t.to(fdt)
        hv = lambda x: d(_unpair(_pair(x)))
        o = _ln(d(_unpair(X)) @ d(_unpair(Wo)).T + d(bo) + d(R), d(l1w), d(l1b))
        h = torch.relu(hv(o) @ d(_unpair(W1)).T + d(b1))
        y = _ln(hv(h) @ d(_unpair(W2)).T + d(b2) + o, d(l2w), d(l2b))
        out = _ln(y, d(pw), d(pb))
        return hv(out) @ d(_unpair(Wh)).T

    res = dict(plain=plain, heads=heads, gemm=Hg, nan_heads=nan_heads, nan_plain=nan_plain, ref64=ref(torch.float64),
               ref32=ref(torch.float32), rows=rows, cols=cols, last=last)
    _RUNS[case] = res
    return res


@pytest.mark.parametrize("case", CASES)
def test_head_part_vs_float64(N, dev, case):
    """H1 against float64 math on the operands' values, to test_chain_b's measured rule: 4 x the
    float32-torch error of the same formula, never below 2e-5 of the scale; every entry written."""
    r = _case(N, dev, case)
    H1 = r["heads"]["H1"].cpu()
    assert H1.shape == (r["rows"], r["cols"]) and torch.isfinite(H1).all()
    scale = r["ref64"].abs().max().item()
    e = (H1.double() - r["ref64"]).abs().max().item()
    e32 = (r["ref32"].double() - r["ref64"]).abs().max().item()
    bound = max(4 * e32, 2e-5 * scale)
    print(f"chain B2 head part {case}: kernel err {e:.2e}, float32 torch err {e32:.2e}, bound {bound:.2e}")
    assert e <= bound, (e, e32, bound)


@pytest.mark.parametrize("case", CASES)
def test_other_outputs_untouched(N, dev, case):
    """Y, OUT and the next layer's Q|K|V are bit-equal to the same call without head weights."""
    r = _case(N, dev, case)
    a, b = r["heads"], r["plain"]
    assert torch.equal(a["Y"], b["Y"]) and torch.equal(a["OUT"], b["OUT"])
    assert torch.isfinite(a["OUT"]).all()
    if not r["last"]:
        assert torch.equal(a["QKV"].view(torch.int16), b["QKV"].view(torch.int16))


@pytest.mark.parametrize("case", CASES)
def test_same_arithmetic_as_gemm_launch(N, dev, case):
    """H1 from chain B2 == cmt_gemm on the OUT16 a call without head weights wrote (the launch this
    replaces): the same three f16 passes per 16-k step in the same order, bit for bit."""
    r = _case(N, dev, case)
    assert torch.isfinite(r["gemm"]).all()
    d = (r["heads"]["H1"] - r["gemm"]).abs().max().item()
    assert torch.equal(r["heads"]["H1"], r["gemm"]), d


@pytest.mark.parametrize("case", CASES[:2])
def test_head_operand_is_the_cleaned_output(N, dev, case):
    """CMT_LN_NAN_TO_NUM: a NaN planted in one partial makes row 0's LayerNorms NaN; OUT holds the
    cleaned zeros, and the head part multiplies those -- row 0 of H1 is exactly zero, the other rows
    are what they were."""
    r = _case(N, dev, case)
    a, b = r["nan_heads"], r["nan_plain"]
    assert torch.equal(a["OUT"], b["OUT"]) and (a["OUT"][0] == 0).all()
    H1 = a["H1"]
    assert torch.isfinite(H1).all() and (H1[0] == 0).all()
    assert torch.equal(H1[1:], r["heads"]["H1"][1:])


def _head(name, dev, **kw):
    from projects.mmdet3d_plugin import synthetic as S
    head, _, _ = S.build_synthetic_head(name, seed=7, grid_size=[256, 256, 40], device=dev, **kw)
    return head


class _Spy:
    """Counts native.gemm calls with N == width and native.chain calls carrying Wh."""

    def __init__(self, native, width):
        self.n, self.width, self.gemms, self.whs = native, width, 0, 0
        self.real = (native.gemm, native.chain)

    def __enter__(self):
        def gemm(*a, **kw):
            self.gemms += kw.get("N") == self.width
            return self.real[0](*a, **kw)

        def chain(*a, **kw):
            self.whs += kw.get("Wh") is not None
            return self.real[1](*a, **kw)
        self.n.gemm, self.n.chain = gemm, chain
        return self

    def __exit__(self, *exc):
        self.n.gemm, self.n.chain = self.real


def _on_off(N, head, fwd, width):
    from projects.mmdet3d_plugin import set_precision
    set_precision("ref")
    head.box_epilogue = False
    outs, seen = {}, {}
    try:
        for on in (True, False):
            with torch.no_grad(), options(chain_heads=on), _Spy(N, width) as spy:
                o = fwd()[0][0]
            torch.cuda.synchronize()
            outs[on] = {k: o[k].clone() for k in KEYS}
            seen[on] = (spy.gemms, spy.whs)
    finally:
        head.box_epilogue = True
    for k in KEYS:
        assert torch.isfinite(outs[True][k]).all(), k
        assert torch.equal(outs[True][k], outs[False][k]), (k, (outs[True][k] - outs[False][k]).abs().max().item())
    return seen


def test_head_level_bit_exact(N, dev, parity_log):
    """The fusion head (final_kernel = 1, one task head) under options(chain_heads=True / False):
    every output bit-identical; on, no GEMM of the heads' width is launched and every chain B2
    carries head weights; off, one such GEMM and none."""
    from projects.mmdet3d_plugin import synthetic as S
    head = _head("cmt_fusion_nus", dev, num_query=96, num_layers=3)
    x = S.synthetic_bev(1, 32, 32, seed=91).to(dev)
    xi = S.synthetic_img(6, 8, 20, seed=92).to(dev)
    metas = S.synthetic_metas(1, pad_shape=(128, 320, 3), seed=93)
    assert len(head.task_heads) == 1 and head.task_heads[0].final_kernel == 1
    width = len(head.task_heads[0].heads) * 64
    seen = _on_off(N, head, lambda: head([x], [xi], metas), width)
    assert seen[True] == (0, 3) and seen[False] == (1, 0), seen
    parity_log.append("task heads' first conv inside chain B2 == its own GEMM launch, bit-exact "
                      "(fusion head, 96 queries, 3 layers)")


def test_fallback_final_kernel_3(N, dev):
    """cmt_lidar_nus (final_kernel = 3: the conv reads neighbouring queries) keeps the GEMM."""
    from projects.mmdet3d_plugin import synthetic as S
    head = _head("cmt_lidar_nus", dev, num_query=64, num_layers=2)
    x = S.synthetic_bev(1, 32, 32, seed=94).to(dev)
    assert head.task_heads[0].final_kernel == 3
    width = len(head.task_heads[0].heads) * 64
    metas = S.synthetic_metas(1, yaws=S.NUS_YAWS[:1], pad_shape=(128, 320, 3), seed=3)
    seen = _on_off(N, head, lambda: head([x], None, metas), width)
    assert seen[True] == seen[False] == (1, 0), seen


def test_fallback_coop_head(N, dev):
    """The cooperative fusion head (final_kernel = 1) max-fuses its agents' outputs before the task
    heads read them: with two agents or one, it keeps the GEMM and never passes head weights."""
    from projects.mmdet3d_plugin import synthetic as S
    head = _head("cmtcoop_fusion_tumtraf", dev, num_query=48, num_layers=2)
    xv, xf = S.synthetic_bev(1, 32, 32, seed=95).to(dev), S.synthetic_bev(1, 32, 32, seed=96).to(dev)
    iv, ii = S.synthetic_img(1, 8, 20, seed=97).to(dev), S.synthetic_img(3, 8, 20, seed=98).to(dev)
    mv = S.synthetic_metas(1, yaws=S.VEHICLE_YAWS, pad_shape=(128, 320, 3), prefix="vehicle_", seed=15)
    mi = S.synthetic_metas(1, yaws=S.INFRA_YAWS, pad_shape=(128, 320, 3), prefix="infrastructure_", seed=16)
    metas = [dict(a, **b) for a, b in zip(mv, mi)]
    assert head.task_heads[0].final_kernel == 1
    width = len(head.task_heads[0].heads) * 64
    seen = _on_off(N, head, lambda: head([xv], [xf], [iv], [ii], metas), width)
    assert seen[True] == seen[False] == (1, 0), seen
    seen = _on_off(N, head, lambda: head([xv], None, [iv], None, metas), width)
    assert seen[True] == seen[False] == (1, 0), seen
