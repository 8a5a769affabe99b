"""The decoder row chains (cmt_chain kinds 0 / 1 / 2) and their LayerNorm epilogue restated once in
plain torch, for tests/test_gpu_chain_edges.py: the same function in float64 is the oracle and in
float32 the reference arithmetic whose own error (e32) scales the bounds.  Also the sentinel-guarded
buffers those tests hand to the kernels.  No test in here: pytest does not collect this module."""
import torch

SPLIT = torch.uint16          # the f16 pair format (native.DT: CMT_F16P)
C, F, HEADS = 256, 1024, 8
FMAX = torch.finfo(torch.float32).max
NAN_TO_NUM, MAX_INTO = 1, 2   # native.LN_NAN_TO_NUM / LN_MAX_INTO


def pair(x):
    """fp32 [..., C] -> [..., 2, C] uint16: hi = f16(x), lo = f16(x - hi)."""
    hi = x.float().half()
    lo = (x.float() - hi.float()).half()
    return torch.stack([hi, lo], -2).contiguous().view(SPLIT)


def unpair(p):
    b = p.view(torch.float16).double()
    return b[..., 0, :] + b[..., 1, :]


def fmt(dt):
    """(op, val) of an operand format: op(x) is the tensor a kernel gets for the values x, val(o)
    the float64 values that tensor holds."""
    if dt == SPLIT:
        return pair, unpair
    return (lambda x: x.to(dt)), (lambda o: o.double())


def ln(x, w, b, eps):
    """nn.LayerNorm in x's dtype: two-pass, biased variance."""
    m = x.mean(-1, keepdim=True)
    v = ((x - m) ** 2).mean(-1, keepdim=True)
    return (x - m) / torch.sqrt(v + eps) * w + b


def post(out, flags, old):
    """The flagged epilogue on the value cast to float32: nan_to_num first (+inf is then exactly
    FMAX), then the cooperative maximum with the old output."""
    o = out.to(torch.float32)
    if flags & NAN_TO_NUM:
        o = torch.nan_to_num(o)
    if flags & MAX_INTO:
        # fmaxf: a NaN operand loses (only met without NAN_TO_NUM)
        o = torch.where(torch.isnan(o), old, torch.where(torch.isnan(old), o, torch.maximum(o, old)))
    return o


def headsplit(q, B, Nq):
    """rows [B * Nq, 32 H] -> flat [B][H][Nq][32]: element (b, h, rr, d) at ((b H + h) Nq + rr) 32 + d."""
    H = q.shape[1] // 32
    out = torch.empty(B, H, Nq, 32, dtype=q.dtype)
    for b in range(B):
        for h in range(H):
            out[b, h] = q[b * Nq:(b + 1) * Nq, 32 * h:32 * h + 32]
    return out.reshape(-1)


def unsplit_pairs(Q):
    """head-split pairs [B][24][Nq][64] (hi 32 | lo 32) -> float64 flat [B][24][Nq][32]."""
    return Q.view(torch.float16).view(-1, 2, 32).double().sum(1).reshape(-1)


def chain_data(B, Nq, seed, head_cols=0):
    """fp32 values of every input of chains A, B1 and B2 (test_chain_a / test_chain_b's scales)."""
    g = torch.Generator().manual_seed(seed)
    rn = lambda *s: torch.randn(*s, generator=g)
    v = lambda n, s=0.1: rn(n) * s
    rows = B * Nq
    d = dict(B=B, Nq=Nq, rows=rows, X=rn(rows, C), R=rn(rows, C), P=rn(rows, C), old=rn(rows, C),
             Wo=rn(C, C) / 16, Wq=rn(C, C) / 16, W1=rn(F, C) / 16, W2=rn(C, F) / 32, Wn=rn(3 * C, C) / 16,
             a_bo=v(C), a_lw=1 + v(C), a_lb=v(C), a_bq=v(C),
             bo=v(C), l1w=1 + v(C), l1b=v(C), b1=v(F), b2=v(C), l2w=1 + v(C), l2b=v(C), pw=1 + v(C), pb=v(C),
             bn=v(3 * C))
    if head_cols:
        d["Wh"] = rn(head_cols, C) / 16
    return d


def prm_a(d):
    return torch.cat([d["a_bo"], d["a_lw"], d["a_lb"], d["a_bq"]])


def prm_b(d, last):
    return torch.cat([d["bo"], d["l1w"], d["l1b"], d["b1"], d["b2"], d["l2w"], d["l2b"], d["pw"], d["pb"],
                      torch.zeros(3 * C) if last else d["bn"]])


def oracle_a(d, dt, fdt, eps=1e-5, with_r=True):
    """Chain A in fdt arithmetic on the values the operands hold -> y, head-split q."""
    op, val = fmt(dt)
    c = lambda t: t.to(fdt)
    hv = lambda x: c(val(op(x)))   # a GEMM operand: rounded to the format where the chain rounds it
    t = hv(d["X"]) @ hv(d["Wo"]).T + c(d["a_bo"]) + (c(d["R"]) if with_r else 0)
    y = ln(t, c(d["a_lw"]), c(d["a_lb"]), eps)
    q = hv(y + c(d["P"])) @ hv(d["Wq"]).T + c(d["a_bq"])
    return dict(Y=y, Q=headsplit(q, d["B"], d["Nq"]))


def other16(x, dt):
    """The 16-bit neighbour of x on the other side of x from its rounding (what a rounding of a
    slightly different x gives once x is close to the midpoint of the two)."""
    r = x.to(dt)
    rb = r.view(torch.int16).to(torch.int32) & 0xFFFF
    key = torch.where(rb >= 0x8000, -(rb & 0x7FFF), rb)          # ordered like the values
    key = key + torch.where(x > r.to(x.dtype), 1, -1)
    bits = torch.where(key < 0, (-key) | 0x8000, key)
    return torch.where(bits >= 0x8000, bits - 0x10000, bits).to(torch.int16).view(dt)


def near_tie(x, dt, tau):
    """Elements of the float64 x within tau of the midpoint of their two 16-bit neighbours."""
    mid = (x.to(dt).double() + other16(x, dt).double()) / 2
    return (x - mid).abs() <= tau


def oracle_b(d, dt, fdt, eps=1e-5, last=False, flags=0, old=None, with_r=True, xv=None, heads=False, flips=None,
             wc=None):
    """Chains B1 + B2 in fdt arithmetic -> Y, OUT (float32, after post()), head-split QKV, H1.
    xv: the attention output's values (fdt) in place of d['X'] (the in-chain split combine).
    flips: masks 'o' / 'h' of the elements of o and h that take the other 16-bit neighbour, or the
    values 'o_val' / 'h_val' where given (settle_b); wc: a dict that keeps the weights' values
    between calls."""
    op, val = fmt(dt)
    c = lambda t: t.to(fdt)
    hv = lambda x: c(val(op(x)))
    hw = lambda k: hv(d[k]) if wc is None else wc.setdefault(k, hv(d[k]))

    def rnd(x, k):   # an operand the chain rounds itself
        if flips is None:
            return hv(x)
        oth = flips[k + "_val"] if k + "_val" in flips else other16(x, dt).double()
        return torch.where(flips[k], c(oth), hv(x))
    x = hv(d["X"]) if xv is None else hv(xv)
    o = ln(x @ hw("Wo").T + c(d["bo"]) + (c(d["R"]) if with_r else 0), c(d["l1w"]), c(d["l1b"]), eps)
    ro = rnd(o, "o")
    h = torch.relu(ro @ hw("W1").T + c(d["b1"]))
    rh = rnd(h, "h")
    y = ln(rh @ hw("W2").T + c(d["b2"]) + o, c(d["l2w"]), c(d["l2b"]), eps)
    out = post(ln(y, c(d["pw"]), c(d["pb"]), eps), flags, old)
    r = dict(Y=y, OUT=out, Q=None, H1=None, o=o, h=h, ro=ro, rh=rh)
    if not last:
        wn = hv(d["Wn"])
        qk = hv(y + c(d["P"])) @ wn[:2 * C].T + c(d["bn"][:2 * C])
        vv = hv(y) @ wn[2 * C:].T + c(d["bn"][2 * C:])
        r["Q"] = headsplit(torch.cat([qk, vv], 1), d["B"], d["Nq"])
    if heads:
        r["H1"] = hv(out) @ hv(d["Wh"]).T
    return r


def settle_b(d, dt, got_y, r64, r32, **kw):
    """The f16 / bf16 oracle rounds o and h to 16 bits where chain B1 does, but from float64 values.
    Where one lies within fp32 error of the midpoint of two 16-bit numbers the oracle is undecided:
    the kernel's (and any float32 reference's) rounding may be the other neighbour, and one such
    element of o moves its row of Y by 3e-4 (f16) to 2e-3 (bf16).  Measured: bf16 (2, 33), o[48, 174]
    lies 7.6e-9 from a midpoint; the kernel and one host's float32 torch round it down, float64 and
    another host's float32 torch up.  So for every row of the kernel's Y beyond the bound, among
    the elements within tau = 4 x the float32 error of their stage of a midpoint (and whose two
    neighbours are further apart than tau), the one whose other neighbour brings the row closest
    is taken, until the row is within the bound or none brings it closer: the kernel has to match
    the oracle under some admissible rounding.  The bound is unchanged and every other element
    keeps its rounding.  Returns the oracle and the float32 reference under the settled roundings
    (both on the same operand values, so e32 stays the reference's arithmetic error) and how many
    were changed."""
    if dt == SPLIT:
        return r64, r32, 0
    bound = bound32(r64["Y"], r32["Y"])[0]
    rowerr = lambda y, rows=slice(None): (got_y[rows].double() - y).abs().amax(1)
    e = rowerr(r64["Y"])
    bad = (e > bound).nonzero().flatten().tolist()
    if not bad:
        return r64, r32, 0
    op, val = fmt(dt)
    hv = lambda x: val(op(x))
    # the float32 error of each stage from the float64 stage's own (rounded) input: no flip in it
    h32 = torch.relu(hv(r64["o"]).float() @ hv(d["W1"]).float().T + d["b1"])
    tau = dict(o=4 * err(r32["o"], r64["o"]), h=4 * err(h32, r64["h"]))
    amb = {k: near_tie(r64[k], dt, tau[k]) &
           ((r64[k].to(dt).double() - other16(r64[k], dt).double()).abs() > tau[k]) for k in ("o", "h")}
    flips = {k: torch.zeros_like(amb[k]) for k in amb}
    rkw = {k: v for k, v in kw.items() if k in ("eps", "with_r")}
    wc, n = {}, 0
    for row in bad:
        sl = slice(row, row + 1)
        dr = dict(d, B=1, Nq=1, rows=1, **{k: d[k][sl] for k in ("X", "R", "P")})
        xv = kw["xv"][sl] if kw.get("xv") is not None else None
        cands = [(k, c) for k in ("o", "h") for c in amb[k][row].nonzero().flatten().tolist()]
        while e[row] > bound and cands:
            tried = []
            for k, c in cands:
                flips[k][row, c] = True
                y = oracle_b(dr, dt, torch.float64, last=True, xv=xv, flips={j: flips[j][sl] for j in flips},
                             wc=wc, **rkw)["Y"]
                flips[k][row, c] = False
                tried.append((rowerr(y, sl).item(), k, c))
            e_new, k, c = min(tried)
            if not e_new < e[row]:
                break
            flips[k][row, c] = True
            cands.remove((k, c))
            e[row], n = e_new, n + 1
    if not n:
        return r64, r32, 0
    s64 = oracle_b(d, dt, torch.float64, flips=flips, **kw)
    same = dict(flips, o_val=s64["ro"], h_val=s64["rh"])
    return s64, oracle_b(d, dt, torch.float32, flips=same, **kw), n


def err(a, r, mask=None):
    """max |a - r| in float64 over the entries of mask (columns or a full mask); NaN if any is NaN."""
    e = (a.double() - r.double()).abs()
    if mask is not None:
        e = e[..., mask] if mask.dim() == 1 else e[mask]
    return float("nan") if torch.isnan(e).any() else e.max().item()


def bound32(r64, r32, pair_out=False, mask=None):
    """An fp32 output's bound: 4 x the float32 reference's own error against float64 (another
    summation order), never below 2e-5 of the scale (cmt_gemm_ln's bound); a pair output adds its
    own precision 2^-21 of the scale."""
    sel = r64 if mask is None else (r64[..., mask] if mask.dim() == 1 else r64[mask])
    scale = sel.double().abs().max().item()
    return max(4 * err(r32, r64, mask), 2e-5 * scale) + (2 ** -21 * scale if pair_out else 0.0), scale


SENT = {torch.int32: 0x7FC0DEAD, torch.int16: 0x7EAD}   # a NaN with a payload no arithmetic produces


class Guarded:
    """n live elements of `dtype` followed by `guard` more, all holding the sentinel bit pattern
    (or `fill` in the live part); .live is what a kernel is given."""

    def __init__(self, n, dtype, dev, guard, fill=None):
        self.it = torch.int32 if dtype == torch.float32 else torch.int16
        self.n = n
        self.bits = torch.full((n + guard,), SENT[self.it], dtype=self.it, device=dev)
        self.live = self.bits.view(dtype)[:n]
        if fill is not None:
            self.live.copy_(fill.reshape(-1).to(dev))

    def intact(self):
        return bool((self.bits[self.n:] == SENT[self.it]).all())

    def written(self, lo=0, hi=None):
        return bool((self.bits[lo:self.n if hi is None else hi] != SENT[self.it]).all())

    def untouched(self, lo, hi):
        return bool((self.bits[lo:hi] == SENT[self.it]).all())
