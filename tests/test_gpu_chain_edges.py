"""Edge, non-finite and row-independence tests of the decoder row chains (cmt_chain: rowchain.hip,
rowchain_x3.hip) and of the LayerNorm epilogue they share with cmt_layernorm_ex and cmt_gemm_ln,
against the float64 restatement in chain_oracle.py.

Bounds (chain_oracle.bound32): an fp32 output max(4 e32, 2e-5 scale), e32 the same formula in
float32 torch against float64; a pair output adds 2^-21 of the scale; the f16 / bf16 Q keeps
test_chain_a / test_chain_b's relative bounds.  Every output buffer carries guard space holding a
sentinel bit pattern.  The f16 / bf16 oracle rounds o, h and y + pos to the format where the chain
does, from float64 values; where o or h lies within fp32 error of the midpoint of two 16-bit numbers
the oracle cannot know the kernel's rounding, and chain_oracle.settle_b admits either neighbour for
those elements alone (met once: bf16 (2, 33), one element 7.6e-9 from a midpoint).  The bounds do
not move.  The whole file runs in about 4 s on an MI355X."""
import pytest
import torch

import chain_oracle as O
from chain_oracle import C, F, FMAX, SPLIT, Guarded

pytestmark = pytest.mark.gpu

DTS = [torch.float16, torch.bfloat16, SPLIT]
DT_ID = {torch.float16: "f16", torch.bfloat16: "bf16", SPLIT: "split"}
# (B, Nq): one row; below one 32-row block; exactly one; the batch edge on the block edge; three batch
# elements in block 0 and one live row in block 1; the batch edge inside block 1
GEOMS = [(1, 1), (1, 31), (1, 32), (2, 32), (3, 11), (2, 33)]
Q_REL = {0: 1.5e-2, 2: 2e-2}   # f16 / bf16 Q relative bounds of test_chain_a / test_chain_b
F64, F32 = torch.float64, torch.float32


@pytest.fixture(scope="module")
def N():
    from projects.mmdet3d_plugin import native
    native.lib()
    return native


# ---------------------------------------------------------------------------------------------------
# running the chains with guarded outputs
# ---------------------------------------------------------------------------------------------------
def run_a(N, dev, d, dt, eps=1e-5, with_r=True, frag=True):
    """Chain A -> Y [rows, C] fp32, Q flat (cpu).  frag: fragment-major Wo (the only split form)."""
    split = dt == SPLIT
    op, _ = O.fmt(dt)
    rows, B, Nq = d["rows"], d["B"], d["Nq"]
    Y = Guarded(rows * C, F32, dev, 3 * C)
    Q = Guarded(B * 8 * Nq * 32, torch.float16 if split else dt, dev, 64)
    pack = N.pack_chain_pair if split else N.pack_chain_wn
    Wo = op(d["Wo"]).to(dev)
    N.chain(0, op(d["X"]).to(dev), d["P"].to(dev), O.prm_a(d).to(dev), pack(Wo) if split or frag else Wo,
            pack(op(d["Wq"]).to(dev)), Y.live.view(rows, C), rows=rows, Nq=Nq, eps=eps,
            R=d["R"].to(dev) if with_r else None, Q=Q.live)
    torch.cuda.synchronize()
    for n, gbuf in (("Y", Y), ("Q", Q)):
        assert gbuf.intact(), f"chain A wrote past the end of {n}"
        assert gbuf.written(), f"chain A left live elements of {n} unwritten"
    return dict(Y=Y.live.view(rows, C).cpu(), Q=Q.live.cpu())


def run_b(N, dev, d, dt, eps=1e-5, last=False, flags=0, old=None, with_r=True, slab=False, head_cols=0,
          xpart=None, xround=False, out16=True):
    """Chains B1 then B2 -> Y, OUT, OUT16, Q, H1 (cpu).  slab: OUT / OUT16 are [3, rows, C] with
    out_offset = rows * C, the old values in slab 1."""
    split = dt == SPLIT
    op, _ = O.fmt(dt)
    rows, B, Nq = d["rows"], d["B"], d["Nq"]
    sps = 2 if split else 1
    wn, fc2 = (N.pack_chain_pair, N.pack_chain_fc2_pair) if split else (N.pack_chain_wn, N.pack_chain_fc2)
    prm = O.prm_b(d, last).to(dev)
    nws = N.chain_ws_numel(rows)
    WS = Guarded(nws, F32, dev, 4 * C)
    Y = Guarded(rows * C, F32, dev, 3 * C)
    Wo, W1 = op(d["Wo"]).to(dev), op(d["W1"]).to(dev)
    xkw = dict(xpart=xpart.to(dev), xsplits=N.CHAIN_XSPLITS, xround=xround) if xpart is not None else {}
    N.chain(1, None if xpart is not None else op(d["X"]).to(dev), None, prm, wn(Wo) if split else Wo,
            wn(W1) if split else W1, Y.live.view(rows, C), rows=rows, Nq=Nq, eps=eps,
            R=d["R"].to(dev) if with_r else None, W2=fc2(op(d["W2"]).to(dev)), WS=WS.live, **xkw)
    torch.cuda.synchronize()
    assert WS.intact(), "chain B1 wrote past chain_ws_numel(rows)"
    assert WS.written(), "chain B1 left part of the workspace unwritten"
    assert Y.untouched(0, rows * C) and Y.intact(), "chain B1 wrote Y"
    ns = 3 if slab else 1
    off = rows * C if slab else 0
    OUT = Guarded(ns * rows * C, F32, dev, 3 * C)
    if flags & O.MAX_INTO:
        OUT.live[off:off + rows * C].copy_(old.reshape(-1).to(dev))
    OUT16 = Guarded(ns * rows * C * sps, dt, dev, 3 * C * sps) if out16 else None
    Q = None if last else Guarded(B * 24 * Nq * 32 * sps, dt, dev, 64)
    H1 = Guarded(rows * head_cols, F32, dev, 3 * head_cols) if head_cols else None
    hkw = dict(Wh=N.pack_chain_heads(O.pair(d["Wh"]).to(dev)), H1=H1.live.view(rows, head_cols),
               head_cols=head_cols) if head_cols else {}
    N.chain(2, None, None if last else d["P"].to(dev), prm, None, None, Y.live.view(rows, C), rows=rows, Nq=Nq,
            eps=eps, Wn=None if last else wn(op(d["Wn"]).to(dev)), OUT=OUT.live, out_offset=off, out_flags=flags,
            Q=None if last else Q.live, WS=WS.live, OUT16=None if OUT16 is None else OUT16.live, **hkw)
    torch.cuda.synchronize()
    assert WS.intact(), "chain B2 wrote past the workspace"
    lo, hi = off, off + rows * C
    for n, gbuf, k in (("Y", Y, 0), ("OUT", OUT, 1), ("OUT16", OUT16, sps), ("Q", Q, 0), ("H1", H1, 0)):
        if gbuf is None:
            continue
        assert gbuf.intact(), f"chain B2 wrote past the end of {n}"
        if k == 0:
            assert gbuf.written(), f"chain B2 left live elements of {n} unwritten"
            continue
        if not (n == "OUT" and flags & O.MAX_INTO):
            assert gbuf.written(lo * k, hi * k), f"chain B2 left live elements of {n} unwritten"
        if slab:   # the neighbouring layers' slabs keep their sentinel
            assert gbuf.untouched(0, lo * k) and gbuf.untouched(hi * k, gbuf.n), f"{n}: slabs 0 / 2 touched"
    out16 = None
    if OUT16 is not None:
        out16 = OUT16.live[lo * sps:hi * sps].view(rows, sps, C).cpu()
    return dict(Y=Y.live.view(rows, C).cpu(), OUT=OUT.live[lo:hi].view(rows, C).cpu(), OUT16=out16,
                Q=None if last else Q.live.cpu(), H1=None if H1 is None else H1.live.view(rows, head_cols).cpu())


def same_bits(a, b):
    """Bit equality; two NaNs count as equal whatever their sign and payload."""
    it, ft = (torch.int32, F32) if a.dtype == F32 else (torch.int16, torch.float16 if a.dtype == SPLIT else a.dtype)
    a, b = a.contiguous(), b.contiguous()
    nan = torch.isnan(a.view(ft)) & torch.isnan(b.view(ft))
    return a.shape == b.shape and bool(((a.view(it) == b.view(it)) | nan).all())


def out16_is_rounded_out(r, dt):
    """OUT16 is the rounding of OUT (bit patterns: NaN-free or not), or its pair split."""
    want = O.pair(r["OUT"]) if dt == SPLIT else r["OUT"].to(dt).unsqueeze(1)
    return same_bits(r["OUT16"], want)


class Checker:
    """Collects 'name err/bound' of one test for parity_log; done() logs them and asserts every one
    (all figures of a test are printed, not only the first that misses)."""

    def __init__(self, log, case):
        self.log, self.case, self.parts, self.fails = log, case, [], []

    def add(self, name, e, b):
        self.parts.append(f"{name} {e:.2e}/{b:.2e}")
        if not e <= b:
            self.fails.append((name, e, b))

    def fp32(self, name, got, r64, r32, pair_out=False, mask=None):
        self.add(name, O.err(got, r64, mask), O.bound32(r64, r32, pair_out, mask)[0])

    def rel(self, name, got, r64, rel):
        self.add(name, O.err(got, r64), rel * r64.abs().max().item())

    def q(self, kind, dt, got, r64, r32):
        if dt != SPLIT:
            self.rel("Q", got, r64, Q_REL[kind])
        elif kind == 0:
            self.rel("Q", got, r64, 2 ** -10)    # an f16 Q: one f16 ulp of its scale (test_chain_a)
        else:
            self.fp32("Q", O.unsplit_pairs(got), r64, r32, pair_out=True)

    def done(self):
        self.log.append(f"chain edges {self.case}: " + ", ".join(self.parts))
        assert not self.fails, (self.case, self.fails)


def refs_b(ck, d, dt, r, **kw):
    """(float64 oracle, float32 reference) of chains B1 + B2 for the run r; the f16 / bf16 oracle
    with its near-tie roundings of o and h settled against the kernel's Y (chain_oracle.settle_b)."""
    r64, r32 = (O.oracle_b(d, dt, f, **kw) for f in (F64, F32))
    r64, r32, n = O.settle_b(d, dt, r["Y"], r64, r32, **kw)
    if n:
        ck.parts.append(f"[{n} near-tie roundings settled]")
    return r64, r32


def check_b(ck, tag, r, dt, r64, r32, last, mask=None):
    ck.fp32(tag + "Y", r["Y"], r64["Y"], r32["Y"])
    ck.fp32(tag + "OUT", r["OUT"], r64["OUT"], r32["OUT"], mask=mask)
    if r["OUT16"] is not None:
        assert out16_is_rounded_out(r, dt), (ck.case, tag, "OUT16 is not the rounding of OUT")
    if not last:
        ck.q(2, dt, r["Q"], r64["Q"], r32["Q"])


# ---------------------------------------------------------------------------------------------------
# 2. row geometry
# ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dt", DTS, ids=DT_ID.get)
@pytest.mark.parametrize("B,Nq", GEOMS)
def test_geometry(N, dev, parity_log, dt, B, Nq):
    """Chains A (with and without R), B1 + B2 (inner layer with nan_to_num; last layer with the
    cooperative maximum) at one row geometry: guards untouched, every live element written, values
    within the bounds.  The head-split address ((b heads + h) Nq + rr) 32 is the oracle's own
    explicit permute (chain_oracle.headsplit)."""
    d = O.chain_data(B, Nq, 1000 * B + Nq)
    ck = Checker(parity_log, f"geometry {DT_ID[dt]} ({B} x {Nq})")
    for with_r in (True, False):
        r = run_a(N, dev, d, dt, with_r=with_r)
        r64, r32 = (O.oracle_a(d, dt, f, with_r=with_r) for f in (F64, F32))
        tag = "A " if with_r else "A(R=None) "
        ck.fp32(tag + "Y", r["Y"], r64["Y"], r32["Y"])
        ck.q(0, dt, r["Q"], r64["Q"], r32["Q"])
        if dt != SPLIT:   # the row-major Wo through the LDS weight ring: the same k order, the same bits
            r2 = run_a(N, dev, d, dt, with_r=with_r, frag=False)
            assert same_bits(r["Y"], r2["Y"]) and same_bits(r["Q"], r2["Q"])
    for last, flags in ((False, O.NAN_TO_NUM), (True, O.NAN_TO_NUM | O.MAX_INTO)):
        r = run_b(N, dev, d, dt, last=last, flags=flags, old=d["old"])
        r64, r32 = refs_b(ck, d, dt, r, last=last, flags=flags, old=d["old"])
        check_b(ck, "B(last) " if last else "B ", r, dt, r64, r32, last)
    if (B, Nq) == (3, 11):
        r = run_b(N, dev, d, dt, with_r=False, flags=O.NAN_TO_NUM)
        r64, r32 = refs_b(ck, d, dt, r, with_r=False, flags=O.NAN_TO_NUM)
        check_b(ck, "B(R=None) ", r, dt, r64, r32, False)
    ck.done()


@pytest.mark.parametrize("dt", DTS, ids=DT_ID.get)
def test_out_offset_slab(N, dev, parity_log, dt):
    """OUT / OUT16 as [3, rows, C] with out_offset = rows * C (run_rows' layer slab): slabs 0 and 2
    keep their sentinel, and LN_MAX_INTO reads the old values from slab 1 (the sentinel NaN of
    slab 0 would lose every maximum)."""
    B, Nq = 3, 11
    d = O.chain_data(B, Nq, 77)
    ck = Checker(parity_log, f"out_offset slab {DT_ID[dt]} ({B} x {Nq})")
    old = d["old"] + 1.0   # above about half of the new values
    for flags in (O.NAN_TO_NUM, O.NAN_TO_NUM | O.MAX_INTO):
        r = run_b(N, dev, d, dt, flags=flags, old=old, slab=True)
        r64, r32 = refs_b(ck, d, dt, r, flags=flags, old=old)
        check_b(ck, f"flags={flags} ", r, dt, r64, r32, False)
        if flags & O.MAX_INTO:
            took_old = (r["OUT"] == old).float().mean().item()
            assert 0.1 < took_old < 0.9, took_old
    ck.done()


@pytest.mark.parametrize("B,Nq", [(3, 11), (1, 32)])
@pytest.mark.parametrize("cols", [64, 320])
def test_head_part_geometry(N, dev, parity_log, B, Nq, cols):
    """Split chain B2 with head weights, one and two head workgroups per row block, guard rows
    after H1; H1 against float64 with test_gpu_chain_heads' bound."""
    d = O.chain_data(B, Nq, 500 + B * 100 + Nq + cols, head_cols=cols)
    ck = Checker(parity_log, f"head part ({B} x {Nq}, {cols} cols)")
    for last in (False, True):
        r = run_b(N, dev, d, SPLIT, last=last, flags=O.NAN_TO_NUM, head_cols=cols, out16=False)
        r64, r32 = (O.oracle_b(d, SPLIT, f, last=last, flags=O.NAN_TO_NUM, heads=True) for f in (F64, F32))
        check_b(ck, "last " if last else "", r, SPLIT, r64, r32, last)
        ck.fp32("H1", r["H1"], r64["H1"], r32["H1"])
    ck.done()


# ---------------------------------------------------------------------------------------------------
# 3. rows do not see each other
# ---------------------------------------------------------------------------------------------------
def _rows_of(r, d, kind, dt):
    """Every output of a run as [rows, ...] tensors of bit patterns (Q / QKV un-head-split)."""
    B, Nq, rows = d["B"], d["Nq"], d["rows"]
    out = {}
    for k, t in r.items():
        if t is None:
            continue
        if k == "Q":
            w = 64 if (dt == SPLIT and kind == 2) else 32
            t = t.view(torch.int16).view(B, -1, Nq, w).permute(0, 2, 1, 3).reshape(rows, -1)
        else:
            t = t.contiguous().view(torch.int32 if t.dtype == F32 else torch.int16).reshape(rows, -1)
        out[k] = t
    return out


@pytest.mark.parametrize("dt", DTS, ids=DT_ID.get)
def test_poisoned_row_stays_alone(N, dev, dt):
    """An inf in one element of row 5 of (2, 33) -- of X for chain A, of R for chain B1: that row
    of Y is all NaN, every other row of every output is bit-equal to the clean run."""
    B, Nq, bad = 2, 33, 5
    d = O.chain_data(B, Nq, 31)
    keep = torch.arange(B * Nq) != bad
    dp = dict(d, X=d["X"].clone(), R=d["R"].clone())
    dp["X"][bad, 17] = float("inf")
    clean, dirty = run_a(N, dev, d, dt), run_a(N, dev, dp, dt)
    a, b = _rows_of(clean, d, 0, dt), _rows_of(dirty, d, 0, dt)
    assert torch.isnan(dirty["Y"][bad]).all()
    for k in a:
        assert torch.equal(a[k][keep], b[k][keep]), ("chain A", k)
    dp = dict(d, R=d["R"].clone())
    dp["R"][bad, 17] = float("inf")
    clean = run_b(N, dev, d, dt, flags=O.NAN_TO_NUM)
    dirty = run_b(N, dev, dp, dt, flags=O.NAN_TO_NUM)
    a, b = _rows_of(clean, d, 2, dt), _rows_of(dirty, d, 2, dt)
    assert torch.isnan(dirty["Y"][bad]).all()
    assert (dirty["OUT"][bad] == 0).all()   # nan_to_num of a NaN row
    for k in a:
        assert torch.equal(a[k][keep], b[k][keep]), ("chain B", k)


@pytest.mark.parametrize("dt", DTS, ids=DT_ID.get)
def test_row_position_does_not_matter(N, dev, dt):
    """B = 1, 64 rows: permuting the rows of X, R, P and the old OUT permutes every output the
    same way, bit for bit (a row's arithmetic depends on neither its lane nor its block); and row
    32 of a 33-row run (alone in its block, its lanes' neighbours clamped copies) equals row 32 of
    the 64-row run on the same data."""
    d = O.chain_data(1, 64, 64)
    perm = torch.randperm(64, generator=torch.Generator().manual_seed(5))
    dp = dict(d, **{k: d[k][perm].contiguous() for k in ("X", "R", "P", "old")})
    d33 = dict(d, Nq=33, rows=33, **{k: d[k][:33].contiguous() for k in ("X", "R", "P", "old")})
    fl = O.NAN_TO_NUM | O.MAX_INTO
    for kind in (0, 2):
        run = (lambda x: run_a(N, dev, x, dt)) if kind == 0 else (lambda x: run_b(N, dev, x, dt, flags=fl, old=x["old"]))
        a, b, c = _rows_of(run(d), d, kind, dt), _rows_of(run(dp), dp, kind, dt), _rows_of(run(d33), d33, kind, dt)
        for k in a:
            assert torch.equal(a[k][perm], b[k]), (kind, k, "permuted rows")
            assert torch.equal(a[k][32], c[k][32]), (kind, k, "row 32 of 33")


# ---------------------------------------------------------------------------------------------------
# 4. LayerNorm epilogue semantics, the same cases in the four implementations
# ---------------------------------------------------------------------------------------------------
ROWS4 = 37   # one row block and a tail
C1, C2, C3 = 9, 100, 201   # columns with w = +inf, b = -inf, w = nan
LN_IMPLS = ["layernorm", "gemm_ln-f16", "gemm_ln-bf16", "gemm_ln-split"]


def _ln_inputs(seed, x_scale=1.0, x_mean=0.0, a_zero=False):
    g = torch.Generator().manual_seed(seed)
    rn = lambda *s: torch.randn(*s, generator=g)
    return dict(x=rn(ROWS4, C) * x_scale + x_mean, A=torch.zeros(ROWS4, C) if a_zero else rn(ROWS4, C),
                W=rn(C, C) / 16, bias=torch.zeros(C) if a_zero else rn(C) * 0.1,
                w=1 + 0.1 * rn(C), b=0.1 * rn(C), w2=1 + 0.1 * rn(C), b2=0.1 * rn(C), old=rn(ROWS4, C), old2=rn(ROWS4, C))


def _ln_oracle(impl, i, fdt, eps, flags, flags2):
    c = lambda t: t.to(fdt)
    t = c(i["x"])
    if impl != "layernorm":
        op, val = O.fmt(_impl_dt(impl))
        t = c(val(op(i["A"]))) @ c(val(op(i["W"]))).T + c(i["bias"]) + t
    y = O.ln(t, c(i["w"]), c(i["b"]), eps)
    y2 = O.ln(y, c(i["w2"]), c(i["b2"]), eps)    # of the first LN's raw output
    return O.post(y, flags, i["old"]), O.post(y2, flags2, i["old2"])


def _impl_dt(impl):
    return {"gemm_ln-f16": torch.float16, "gemm_ln-bf16": torch.bfloat16, "gemm_ln-split": SPLIT}[impl]


def _ln_run(N, dev, impl, i, eps, flags=0, flags2=0):
    """(Y, Y2) of the first and second LN through native.layernorm or native.gemm_ln (x is the LN
    input itself, or gemm_ln's R behind A W^T + bias), guard rows after both."""
    Y = Guarded(ROWS4 * C, F32, dev, 3 * C, fill=i["old"] if flags & O.MAX_INTO else None)
    Y2 = Guarded(ROWS4 * C, F32, dev, 3 * C, fill=i["old2"] if flags2 & O.MAX_INTO else None)
    t = lambda k: i[k].to(dev)
    if impl == "layernorm":
        N.layernorm(t("x"), t("w"), t("b"), Y.live.view(ROWS4, C), rows=ROWS4, C=C, ldx=C, ldy=C, eps=eps, flags=flags,
                    W2=t("w2"), B2=t("b2"), Y2=Y2.live.view(ROWS4, C), ldy2=C, flags2=flags2)
    else:
        op, _ = O.fmt(_impl_dt(impl))
        N.gemm_ln(op(i["A"]).to(dev), op(i["W"]).to(dev), M=ROWS4, K=C, lda=C, ldw=C, bias=t("bias"), R=t("x"), ldr=C,
                  ln_w=t("w"), ln_b=t("b"), eps=eps, Y=Y.live.view(ROWS4, C), flags=flags, W2=t("w2"), B2=t("b2"),
                  Y2=Y2.live.view(ROWS4, C), flags2=flags2)
    torch.cuda.synchronize()
    assert Y.intact() and Y2.intact(), "LayerNorm wrote past its rows"
    assert (flags & O.MAX_INTO or Y.written()) and (flags2 & O.MAX_INTO or Y2.written())
    return Y.live.view(ROWS4, C).cpu(), Y2.live.view(ROWS4, C).cpu()


def _offset(d):
    return dict(d, X=torch.zeros_like(d["X"]), R=d["R"] + 300.0)


@pytest.mark.parametrize("impl", LN_IMPLS)
def test_ln_offset_rows(N, dev, parity_log, impl):
    """LN input N(0, 1) + 300: a two-pass variance stays within the bound (float32 torch is 7e-5
    from float64 here), a one-pass E[x^2] - mean^2 is 5e-2 off."""
    ck = Checker(parity_log, f"offset rows {impl}")
    i = _ln_inputs(41, x_mean=300.0, a_zero=True)
    got = _ln_run(N, dev, impl, i, 1e-5)
    r64, r32 = (_ln_oracle(impl, i, f, 1e-5, 0, 0) for f in (F64, F32))
    ck.fp32("Y", got[0], r64[0], r32[0])
    ck.fp32("Y2", got[1], r64[1], r32[1])
    ck.done()


@pytest.mark.parametrize("dt", DTS, ids=DT_ID.get)
def test_chain_offset_rows(N, dev, parity_log, dt):
    """The same through the chains' R (X = 0): chain A's norms[0], chain B1's norms[1]."""
    d = _offset(O.chain_data(1, ROWS4, 42))
    ck = Checker(parity_log, f"offset rows chains {DT_ID[dt]}")
    ck.fp32("A Y", run_a(N, dev, d, dt)["Y"], *(O.oracle_a(d, dt, f)["Y"] for f in (F64, F32)))
    r = run_b(N, dev, d, dt, flags=O.NAN_TO_NUM)
    check_b(ck, "B ", r, dt, *refs_b(ck, d, dt, r, flags=O.NAN_TO_NUM), False)
    ck.done()


@pytest.mark.parametrize("impl", LN_IMPLS)
def test_ln_constant_row_known_answer(N, dev, impl):
    """X = 0, bias 0, R = 3.0 in every column: sum, mean and deviations are exact, so the LN
    output is the LN bias bit for bit; with a constant LN bias the second LN's output is its own
    bias, whatever eps > 0 is."""
    i = _ln_inputs(43, a_zero=True)
    i["x"] = torch.full((ROWS4, C), 3.0)
    for eps in (1e-5, 1e-3):
        y, _ = _ln_run(N, dev, impl, i, eps)
        assert same_bits(y, i["b"].expand(ROWS4, C))
        _, y2 = _ln_run(N, dev, impl, dict(i, b=torch.full((C,), 0.5)), eps)
        assert same_bits(y2, i["b2"].expand(ROWS4, C))


@pytest.mark.parametrize("dt", DTS, ids=DT_ID.get)
def test_chain_constant_row_known_answer(N, dev, dt):
    """The chains: X = 0, out-proj bias 0, R = 3.0 -> chain A's Y is norms[0]'s bias exactly.
    Chain B with a constant norms[1] bias, fc2 = 0 and a constant fc2 bias hands norms[2] a
    constant row: Y is norms[2]'s bias, and with that constant too OUT is post_norm's bias."""
    d = O.chain_data(1, ROWS4, 44)
    z = torch.zeros(C)
    d.update(X=torch.zeros(ROWS4, C), R=torch.full((ROWS4, C), 3.0), a_bo=z, bo=z, l1b=torch.full((C,), 0.5),
             W2=torch.zeros(C, F), b2=torch.full((C,), 0.25))
    for eps in (1e-5, 1e-3):
        assert same_bits(run_a(N, dev, d, dt, eps=eps)["Y"], d["a_lb"].expand(ROWS4, C))
        r = run_b(N, dev, d, dt, eps=eps, last=True)
        assert same_bits(r["Y"], d["l2b"].expand(ROWS4, C))
        r = run_b(N, dev, dict(d, l2b=torch.full((C,), 2.0)), dt, eps=eps, last=True)
        assert same_bits(r["OUT"], d["pb"].expand(ROWS4, C))
        assert out16_is_rounded_out(r, dt)


def _two_eps(ck, run, oracle, names, refs_of=None):
    """Runs at eps 1e-5 and 1e-3 match the oracle at their own eps, and the two oracles differ by
    more than 100 x the bound: no hard-coded eps passes both."""
    refs = {}
    for eps in (1e-5, 1e-3):
        got = run(eps)
        refs[eps] = refs_of(got, eps) if refs_of else (oracle(F64, eps), oracle(F32, eps))
        for n in names:
            ck.fp32(f"eps={eps:g} {n}", got[n], refs[eps][0][n], refs[eps][1][n])
    for n in names:
        gap = O.err(refs[1e-5][0][n], refs[1e-3][0][n])
        b = max(O.bound32(refs[e][0][n], refs[e][1][n])[0] for e in refs)
        assert gap > 100 * b, (n, gap, b)


@pytest.mark.parametrize("impl", LN_IMPLS)
def test_ln_eps(N, dev, parity_log, impl):
    """Rows of standard deviation 1e-3 (the first LN's input; the second LN's through a first LN
    weight of 1e-3 scale and zero bias)."""
    i = _ln_inputs(45, x_scale=1e-3, a_zero=True)
    i.update(w=i["w"] * 1e-3, b=torch.zeros(C))
    ck = Checker(parity_log, f"eps {impl}")
    run = lambda eps: dict(zip(("Y", "Y2"), _ln_run(N, dev, impl, i, eps)))
    oracle = lambda f, eps: dict(zip(("Y", "Y2"), _ln_oracle(impl, i, f, eps, 0, 0)))
    _two_eps(ck, run, oracle, ("Y", "Y2"))
    ck.done()


@pytest.mark.parametrize("dt", DTS, ids=DT_ID.get)
def test_chain_eps(N, dev, parity_log, dt):
    """Chain A's norms[0] and chain B1's norms[1] see rows of deviation 1e-3 through R (X = 0);
    post_norm sees them through a norms[2] weight of 1e-3 scale and zero bias."""
    d = O.chain_data(1, ROWS4, 46)
    z = torch.zeros(C)
    d.update(X=torch.zeros(ROWS4, C), R=d["R"] * 1e-3, a_bo=z, bo=z, l2w=d["l2w"] * 1e-3, l2b=z)
    ck = Checker(parity_log, f"eps chains {DT_ID[dt]}")
    _two_eps(ck, lambda eps: run_a(N, dev, d, dt, eps=eps), lambda f, eps: O.oracle_a(d, dt, f, eps=eps), ("Y",))
    _two_eps(ck, lambda eps: run_b(N, dev, d, dt, eps=eps, last=True), None, ("Y", "OUT"),
             refs_of=lambda got, eps: refs_b(ck, d, dt, got, eps=eps, last=True))
    ck.done()


def _special(w, b):
    w, b = w.clone(), b.clone()
    w[C1], b[C2], w[C3] = float("inf"), float("-inf"), float("nan")
    return w, b


PLAIN = torch.ones(C, dtype=torch.bool)
PLAIN[[C1, C2, C3]] = False


def _check_special(got, ref, flags, old=None):
    """The three special columns, exactly.  ref: the oracle's float32 output with the same flags."""
    sp = [C1, C2, C3]
    assert same_bits(got[:, sp], ref[:, sp]), (got[:3, sp], ref[:3, sp])
    if flags == 0:
        assert torch.isinf(got[:, C1]).all() and (got[:, C2] == float("-inf")).all() and torch.isnan(got[:, C3]).all()
    elif flags == O.NAN_TO_NUM:
        assert (got[:, C1].abs() == FMAX).all() and (got[:, C1] > 0).any() and (got[:, C1] < 0).any()
        assert (got[:, C2] == -FMAX).all() and (got[:, C3] == 0).all()
    else:   # nan_to_num, then the maximum with old = -1: the other order leaves -1 in the NaN column
        assert (got[:, C3] == 0).all() and (got[:, C2] == -1).all()
        assert ((got[:, C1] == FMAX) | (got[:, C1] == -1)).all() and (got[:, C1] == FMAX).any()


@pytest.mark.parametrize("which", ["first", "second"])
@pytest.mark.parametrize("impl", LN_IMPLS)
def test_ln_nan_to_num_branches(N, dev, parity_log, impl, which):
    """w = +inf, b = -inf and w = nan in three columns of the LN that carries the flag (W / B for
    flags, W2 / B2 for flags2): with LN_NAN_TO_NUM the columns are +-FLT_MAX by the sign of the
    normalised value, -FLT_MAX and 0 exactly; without it +-inf, -inf and NaN; with LN_MAX_INTO on
    old values of -1.0 the NaN column is 0 and the -inf column -1 (nan_to_num first)."""
    i = _ln_inputs(47)
    i["old"] = i["old2"] = torch.full((ROWS4, C), -1.0)
    first = which == "first"
    if first:
        i["w"], i["b"] = _special(i["w"], i["b"])
    else:
        i["w2"], i["b2"] = _special(i["w2"], i["b2"])
    ck = Checker(parity_log, f"nan_to_num {impl} {which} LN")
    for flags in (0, O.NAN_TO_NUM, O.NAN_TO_NUM | O.MAX_INTO):
        f1, f2 = (flags, 0) if first else (0, flags)
        got = _ln_run(N, dev, impl, i, 1e-5, f1, f2)
        r64, r32 = (_ln_oracle(impl, i, f, 1e-5, f1, f2) for f in (F64, F32))
        k = 0 if first else 1
        ck.fp32(f"flags={flags} ", got[k], r64[k], r32[k], mask=PLAIN)
        _check_special(got[k], r64[k], flags)
        if not first:
            ck.fp32(f"flags={flags} Y ", got[0], r64[0], r32[0])
    ck.done()


@pytest.mark.parametrize("dt", DTS, ids=DT_ID.get)
def test_chain_nan_to_num_branches(N, dev, parity_log, dt):
    """The same three columns in chain B2's post_norm (post_w / post_b of the parameter block);
    OUT16 holds the rounding (or pair split) of OUT bit for bit, non-finite values included; Y and
    the next layer's Q|K|V do not see post_norm."""
    d = O.chain_data(1, ROWS4, 48)
    d["pw"], d["pb"] = _special(d["pw"], d["pb"])
    old = torch.full((ROWS4, C), -1.0)
    ck = Checker(parity_log, f"nan_to_num chain B2 {DT_ID[dt]}")
    for flags in (0, O.NAN_TO_NUM, O.NAN_TO_NUM | O.MAX_INTO):
        r = run_b(N, dev, d, dt, flags=flags, old=old)
        r64, r32 = refs_b(ck, d, dt, r, flags=flags, old=old)
        check_b(ck, f"flags={flags} ", r, dt, r64, r32, False, mask=PLAIN)
        _check_special(r["OUT"], r64["OUT"], flags)
    ck.done()


def test_nan_row_into_head_part(N, dev):
    """Split chain B2 with head weights, one row NaN through B1's R: that row of OUT and of H1 is
    exactly 0 (the head part multiplies the cleaned output), every other row is the clean run's."""
    B, Nq, cols, bad = 3, 11, 320, 12
    d = O.chain_data(B, Nq, 49, head_cols=cols)
    dn = dict(d, R=d["R"].clone())
    dn["R"][bad] = float("nan")
    kw = dict(flags=O.NAN_TO_NUM, head_cols=cols, out16=False)
    clean, dirty = run_b(N, dev, d, SPLIT, **kw), run_b(N, dev, dn, SPLIT, **kw)
    assert (dirty["OUT"][bad] == 0).all() and (dirty["H1"][bad] == 0).all()
    assert torch.isnan(dirty["Y"][bad]).all()
    keep = torch.arange(B * Nq) != bad
    a, b = _rows_of(clean, d, 2, SPLIT), _rows_of(dirty, d, 2, SPLIT)
    for k in a:
        assert torch.equal(a[k][keep], b[k][keep]), k


# ---------------------------------------------------------------------------------------------------
# 5. cmt_layernorm_ex beyond C = 256
# ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("lp", DTS, ids=DT_ID.get)
@pytest.mark.parametrize("Cw,nparts", [(64, 1), (192, 2), (256, 1), (256, 2), (256, 3), (256, 4), (1024, 1)])
def test_layernorm_ex_widths(N, dev, parity_log, Cw, nparts, lp):
    """Widths 64 .. 1024, 1 / 4 / 5 rows (a workgroup takes 4), the templated (1, 2, 4 at C = 256)
    and run-time nparts loops, ldx / ldy / ldy2 > C with sentinel columns between the rows, and
    Yl / Yp in f16, bf16 and pairs equal to the rounding of Y and Y + P."""
    ck = Checker(parity_log, f"layernorm_ex C={Cw} nparts={nparts} {DT_ID[lp]}")
    sps = 2 if lp == SPLIT else 1
    for rows in (1, 4, 5):
        g = torch.Generator().manual_seed(Cw + 10 * nparts + rows)
        rn = lambda *s: torch.randn(*s, generator=g)
        ldx, ldy, ldy2 = Cw + 8, Cw + 4, Cw + 12
        x = rn(nparts, rows, ldx) * 2 + 0.5
        w, b, w2, b2, P = 1 + 0.1 * rn(Cw), 0.1 * rn(Cw), 1 + 0.1 * rn(Cw), 0.1 * rn(Cw), rn(rows, Cw)
        Y, Y2 = Guarded(rows * ldy, F32, dev, 3 * ldy), Guarded(rows * ldy2, F32, dev, 3 * ldy2)
        Yl, Yp = (Guarded(rows * Cw * sps, lp, dev, 3 * Cw * sps) for _ in range(2))
        N.layernorm_ex(x.to(dev), w.to(dev), b.to(dev), rows=rows, C=Cw, ldx=ldx, eps=1e-5, Y=Y.live, ldy=ldy,
                       W2=w2.to(dev), B2=b2.to(dev), Y2=Y2.live, ldy2=ldy2,
                       Yl=Yl.live.view(rows, sps, Cw) if sps == 2 else Yl.live.view(rows, Cw),
                       Yp=Yp.live.view(rows, sps, Cw) if sps == 2 else Yp.live.view(rows, Cw), P=P.to(dev), nparts=nparts)
        torch.cuda.synchronize()
        for n, gbuf, ld in (("Y", Y, ldy), ("Y2", Y2, ldy2)):
            assert gbuf.intact(), n
            bits = gbuf.bits[:gbuf.n].view(rows, ld)
            assert (bits[:, Cw:] == O.SENT[torch.int32]).all(), f"{n}: columns past C written"
            assert (bits[:, :Cw] != O.SENT[torch.int32]).all(), f"{n}: live columns unwritten"
        assert Yl.intact() and Yp.intact() and Yl.written() and Yp.written()
        y, y2 = Y.live.view(rows, ldy)[:, :Cw].cpu(), Y2.live.view(rows, ldy2)[:, :Cw].cpu()
        refs = []
        for f in (F64, F32):
            t = x[:, :, :Cw].to(f).sum(0)
            r1 = O.ln(t, w.to(f), b.to(f), 1e-5)
            refs.append((r1, O.ln(r1, w2.to(f), b2.to(f), 1e-5)))
        ck.fp32(f"rows={rows} Y", y, refs[0][0], refs[1][0])
        ck.fp32(f"rows={rows} Y2", y2, refs[0][1], refs[1][1])
        shape = (rows, sps, Cw) if sps == 2 else (rows, Cw)
        rnd = O.pair if sps == 2 else (lambda t: t.to(lp))
        assert same_bits(Yl.live.view(shape).cpu(), rnd(y.contiguous()))
        assert same_bits(Yp.live.view(shape).cpu(), rnd(y + P))
    ck.done()


# ---------------------------------------------------------------------------------------------------
# 6. the in-chain combine of the attention's split partials (xpart)
# ---------------------------------------------------------------------------------------------------
def _xpart(B, Nq, seed):
    """Partials in the workspace layout of cmt_attn_fwd with CMT_ATTN_KEEP_PARTIALS
    (attention.hip's split write: row = ((split B + b) H + h) Nq + q): O [8][B][8][Nq][32] fp32,
    then M [8][B][8][Nq], then L [8][B][8][Nq]."""
    g = torch.Generator().manual_seed(seed)
    S, n = 8, B * 8 * Nq
    Ov = torch.randn(S, n, 32, generator=g)
    M = (torch.rand(S, n, generator=g) - 0.5) * 40
    L = 0.5 + 1.5 * torch.rand(S, n, generator=g)
    for r in range(0, n, 3):   # every third (b, h, q): 1 .. 7 empty splits, never all 8
        k = 1 + (r // 3) % 7
        dead = torch.randperm(S, generator=g)[:k]
        Ov[dead, r], L[dead, r] = 0.0, 0.0
        M[dead, r] = 0.0 if (r // 3) % 2 else 60.0   # the placeholder, or a bounded-max offset
    return Ov, M, L


def _combine(Ov, M, L, B, Nq, fdt, xround):
    """attn_combine_kernel's formula in fdt -> X rows [B * Nq, 256] (head h in columns 32 h ..)."""
    Ov, M, L = Ov.to(fdt), M.to(fdt), L.to(fdt)
    live = L > 0
    mx = torch.where(live, M, torch.full_like(M, float("-inf"))).max(0).values
    w = torch.where(live, torch.exp2(M - mx), torch.zeros_like(M))
    x = (w.unsqueeze(-1) * Ov).sum(0) / (w * L).sum(0).unsqueeze(-1)          # [B 8 Nq, 32]
    if xround:
        x = x.half().to(fdt)
    return x.view(B, 8, Nq, 32).permute(0, 2, 1, 3).reshape(B * Nq, C)


@pytest.mark.parametrize("xround", [False, True])
@pytest.mark.parametrize("B,Nq", [(3, 11), (2, 32)])
def test_xpart_combine(N, dev, parity_log, B, Nq, xround):
    """Split chain B1 fed the cross-attention's eight split partials directly.  M is in exp2
    units (the writer stores the running maximum of s * scale * log2(e), or the bounded offset P
    was taken against; the combine weighs a split by exp2(M - max M)).  An empty split holds O = 0,
    L = 0 and a finite M that must be ignored: the placeholder 0.0 of the online path or the
    bounded offset -- here 0.0 and 60.0, the latter above every live M.  Compared through B2's
    Y / OUT / QKV with the float64 combine (rounded to f16 when xround) in front of the oracle.
    Against the same chain fed pair rows of a float32 CPU combine the outputs agree to the bound,
    not bit for bit: the kernel's v_exp_f32 and its fused multiply-adds are not torch's float32
    exp2, multiply and sum."""
    d = O.chain_data(B, Nq, 600 + Nq)
    Ov, M, L = _xpart(B, Nq, 61 + Nq)
    xp = torch.cat([Ov.reshape(-1), M.reshape(-1), L.reshape(-1)])
    ck = Checker(parity_log, f"xpart ({B} x {Nq}) xround={xround}")
    r = run_b(N, dev, d, SPLIT, flags=O.NAN_TO_NUM, xpart=xp, xround=xround)
    r64, r32 = (O.oracle_b(d, SPLIT, f, flags=O.NAN_TO_NUM, xv=_combine(Ov, M, L, B, Nq, f, xround)) for f in (F64, F32))
    check_b(ck, "", r, SPLIT, r64, r32, False)
    fed = run_b(N, dev, dict(d, X=_combine(Ov, M, L, B, Nq, F32, xround)), SPLIT, flags=O.NAN_TO_NUM)
    ck.add("Y vs fed-X", O.err(r["Y"], fed["Y"]), O.bound32(r64["Y"], r32["Y"])[0])
    ck.done()
