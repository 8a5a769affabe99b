"""cmt_gemm / cmt_gemm_ln, one small case per kernel family and shared tile piece.

The table holds the smallest shapes at which each family's pieces can go wrong: one valid
row in the last row tile, fewer k stages than ring slots and a refilling ring, a tap that is
one stage or several, head-split tiles below a batch and across two, every C dtype's staged
store.  A case's id names the family cmt_gemm's dispatch rules (gemm.hip, bottom) send it to;
the kernel name itself is not asserted.  Every call goes through the C ABI and is checked
against a float64 product of the operands as the kernel reads them.

Bounds (those of the neighbouring tests):
  pair operands        _tol of test_gpu_split.py, + 2^-21 max|ref| for a pair output
  fp32 / 16-bit        1e-4 / 5e-3 absolute with W / sqrt(K) (test_gemm_plain); a 16-bit C adds its
                       own rounding, half an ulp: at most 2^-11 (f16) / 2^-8 (bf16) of max|ref|
  cmt_gemm_ln          LN moves a pre-norm error e by at most 2 max|w| e / min(row std); on top the
                       2e-5 max|ref| of test_gemm_ln_split for the fp32 LN itself

run_case(native, dev, id) returns the raw outputs, so a job can compare two libraries byte by byte.
"""
import math

import pytest
import torch

from test_gpu_split import SPLIT, _pair, _tol, _unpair

pytestmark = pytest.mark.gpu

DT = {"f16": torch.float16, "bf16": torch.bfloat16}
HALF_ULP = {"f16": 2 ** -11, "bf16": 2 ** -8}   # 11 / 8 significant bits: half an ulp of x is at most this times |x|


@pytest.fixture(scope="module")
def N():
    from projects.mmdet3d_plugin import native
    native.lib()
    return native


def _operand(x, kind):
    """(device tensor, float64 value the kernel computes with) of an fp32 host operand"""
    if kind == "pair":
        return _pair(x), x.double()
    if kind in DT:
        return x.to(DT[kind]), x.to(DT[kind]).double()
    return x, x.double()


def _bound(kind, ref, K, cdt):
    m = ref.abs().max().item()
    base = _tol(ref, K) if kind == "pair" else (1e-4 if kind == "f32" else 5e-3)
    return base + (2 ** -21 * m if cdt == "pair" else HALF_ULP[cdt] * m if cdt in DT else 0.0)


def _new_c(shape, cdt, dev):
    if cdt == "pair":
        return torch.full(shape[:-1] + (2, shape[-1]), 0x7e00, dtype=torch.int16, device=dev).view(SPLIT)
    return torch.full(shape, float("nan"), dtype=DT.get(cdt, torch.float32), device=dev)


def _value(c, cdt):
    return _unpair(c.cpu()) if cdt == "pair" else c.cpu().double()


def rows(kind, M, N_, K, *, wkind=None, cdt="f32", relu=False, rdt=None, batch=1, rpb=0, k_splits=0, a2=None,
         a2_cols=0):
    """Row-mode A.  kind: A's dtype; wkind: W's (default the same; fp32 A with 16-bit W is the
    register-staged kernel); rpb: head-split rows per batch; a2: 'select' | 'add'."""
    wkind = wkind or kind

    def run(N, dev):
        g = torch.Generator().manual_seed(M + 3 * N_ + 7 * K + batch)
        A = torch.randn(batch, M, K, generator=g)
        A2 = torch.randn(batch, M, K, generator=g)
        W = torch.randn(N_, K, generator=g) / math.sqrt(K)
        b = torch.randn(N_, generator=g)
        R = torch.randn(batch, M, N_, generator=g)
        Ad, Av = _operand(A, kind)
        Wd, Wv = _operand(W, wkind)
        if wkind in DT and kind == "f32":          # fp32 A is cast to W's dtype in registers
            Av = A.to(DT[wkind]).double()
        ref = Av @ Wv.t()
        kw = {}
        if a2 == "select":
            A2d, A2v = _operand(A2, kind)
            ref = torch.cat([(A2v @ Wv.t())[..., :a2_cols], ref[..., a2_cols:]], -1)
            kw.update(A2=A2d.to(dev), lda2=K, a2_cols=a2_cols)
        elif a2 == "add":
            s = (A + A2).to(DT[wkind]).double() if wkind in DT else (A + A2).double()
            ref = torch.cat([(s @ Wv.t())[..., :a2_cols], ref[..., a2_cols:]], -1)
            kw.update(A2=A2.to(dev), lda2=K, a2_cols=a2_cols)
        ref = ref + b.double()
        if relu:
            ref = torch.relu(ref)
        if rdt:
            Rd, Rv = _operand(R, rdt)
            ref = ref + Rv
            kw.update(R=Rd.to(dev), ldr=N_, r_bstride=M * N_)
        if k_splits:
            C = torch.full((k_splits, M, N_), float("nan"), device=dev)
            kw.update(k_splits=k_splits)
        elif rpb:
            C = _new_c((batch * M // rpb, N_ // 32, rpb, 32), cdt, dev)
            kw.update(headsplit_rows=rpb)
        else:
            C = _new_c((batch, M, N_), cdt, dev)
            kw.update(c_bstride=M * N_)
        N.gemm(Ad.to(dev), Wd.to(dev), C, M=M, N=N_, K=K, lda=K, ldw=K, ldc=0 if rpb else N_, bias=b.to(dev),
               relu=relu, batch=batch, a_bstride=M * K, **kw)
        if k_splits:
            got = C.cpu().double().sum(0)[None]
        elif rpb and cdt == "pair":                # [B][N/32][S][hi 32 | lo 32]
            h = C.cpu().view(torch.float16).double().view(-1, N_ // 32, rpb, 64)
            got = (h[..., :32] + h[..., 32:]).permute(0, 2, 1, 3).reshape(batch, M, N_)
        elif rpb:
            got = C.cpu().double().permute(0, 2, 1, 3).reshape(batch, M, N_)
        else:
            got = _value(C, cdt)
        return [C], [("C", (got - ref).abs().max().item(), _bound(wkind, ref, K, cdt))]
    return run


def conv3x3(kind, B, H, Wd_, Cin, N_, *, cdt="f32", in_m=False):
    """Implicit 3x3 conv on NHWC rows (CMT_A_CONV3X3); in_m: the B images are consecutive rows of
    one problem (M = B H W) instead of a batch."""
    def run(N, dev):
        g = torch.Generator().manual_seed(H * Wd_ + Cin)
        x = torch.randn(B, Cin, H, Wd_, generator=g)
        w = torch.randn(N_, Cin, 3, 3, generator=g) / math.sqrt(9 * Cin)
        b = torch.randn(N_, generator=g)
        xd, xv = _operand(x.permute(0, 2, 3, 1).reshape(B * H * Wd_, Cin).contiguous(), kind)
        wd, wv = _operand(w.permute(0, 2, 3, 1).reshape(N_, 9 * Cin).contiguous(), kind)
        xv = xv.view(B, H, Wd_, Cin).permute(0, 3, 1, 2)
        wv = wv.view(N_, 3, 3, Cin).permute(0, 3, 1, 2)
        ref = torch.relu(torch.nn.functional.conv2d(xv, wv, b.double(), padding=1)).flatten(2).permute(0, 2, 1)
        C = _new_c((B, H * Wd_, N_), cdt, dev)
        hw = H * Wd_
        N.gemm(xd.to(dev), wd.to(dev), C, M=B * hw if in_m else hw, N=N_, K=9 * Cin, lda=Cin, ldw=9 * Cin, ldc=N_,
               bias=b.to(dev), relu=True, a_mode=N.A_CONV3X3, conv=(H, Wd_, Cin), batch=1 if in_m else B,
               a_bstride=hw * Cin, c_bstride=hw * N_)
        return [C], [("C", (_value(C, cdt) - ref).abs().max().item(), _bound(kind, ref, 9 * Cin, cdt))]
    return run


def conv1d3(kind, seg, nseg, Cin, N_, *, wkind=None):
    """Implicit k = 3 conv along segments of seg rows (CMT_A_CONV1D3), K = 3 Cin."""
    wkind = wkind or kind

    def run(N, dev):
        g = torch.Generator().manual_seed(seg + Cin)
        M = seg * nseg
        x = torch.randn(M, Cin, generator=g)
        w = torch.randn(N_, Cin, 3, generator=g) / math.sqrt(3 * Cin)
        xd, xv = _operand(x, kind)
        wd, wv = _operand(w.permute(0, 2, 1).reshape(N_, 3 * Cin).contiguous(), wkind)
        if wkind in DT and kind == "f32":
            xv = x.to(DT[wkind]).double()
        wv = wv.view(N_, 3, Cin).permute(0, 2, 1)
        ref = torch.nn.functional.conv1d(xv.view(nseg, seg, Cin).permute(0, 2, 1), wv, padding=1)
        ref = ref.permute(0, 2, 1).reshape(M, N_)
        C = _new_c((M, N_), "f32", dev)
        N.gemm(xd.to(dev), wd.to(dev), C, M=M, N=N_, K=3 * Cin, lda=Cin, ldw=3 * Cin, ldc=N_, a_mode=N.A_CONV1D3,
               seg_len=seg)
        return [C], [("C", (C.cpu().double() - ref).abs().max().item(), _bound(wkind, ref, 3 * Cin, "f32"))]
    return run


def halo(wkind, H, Wd_, Cin, N_, *, cdt, second=False):
    """conv_halo_x3_kernel: 3x3 conv from the fp32 NCHW map, pair W or one 16-bit pass."""
    def run(N, dev):
        g = torch.Generator().manual_seed(H + Wd_ + Cin)
        x = torch.randn(1, Cin, H, Wd_, generator=g)
        w = torch.randn(N_, Cin, 3, 3, generator=g) / math.sqrt(9 * Cin)
        b = torch.randn(N_, generator=g)
        P = torch.randn(H * Wd_, N_, generator=g)
        wd, wv = _operand(w.permute(0, 2, 3, 1).reshape(N_, 9 * Cin).contiguous(), wkind)
        xv = x.double() if wkind == "pair" else x.to(DT[wkind]).double()
        wv = wv.view(N_, 3, 3, Cin).permute(0, 3, 1, 2)
        ref = torch.relu(torch.nn.functional.conv2d(xv, wv, b.double(), padding=1)).flatten(2).permute(0, 2, 1)[0]
        hw = H * Wd_
        C, C2 = _new_c((hw, N_), cdt, dev), _new_c((hw, N_), cdt, dev)
        kw = dict(A2=P.to(dev), lda2=N_, c2=C2) if second else {}
        N.gemm(x.to(dev), wd.to(dev), C, M=hw, N=N_, K=9 * Cin, lda=hw, ldw=9 * Cin, ldc=N_, bias=b.to(dev), relu=True,
               a_mode=N.A_CONV3X3_NCHW, conv=(H, Wd_, Cin), a_bstride=Cin * hw, c_bstride=hw * N_, **kw)
        # one pass: fp32 accumulation order over K = 9 Cin on top of the plain bound's operands
        bd = _bound(wkind, ref, 9 * Cin, cdt)
        checks = [("C", (_value(C, cdt) - ref).abs().max().item(), bd)]
        if second:
            ref2 = ref + P.double()
            checks.append(("C2", (_value(C2, cdt) - ref2).abs().max().item(), _bound(wkind, ref2, 9 * Cin, cdt)))
        return [C] + ([C2] if second else []), checks
    return run


def gemm_ln(kind, M, K, *, with_r, y2=False):
    def run(N, dev):
        g = torch.Generator().manual_seed(M + K + with_r)
        C = 256
        A = torch.randn(M, K, generator=g)
        W = torch.randn(C, K, generator=g) / math.sqrt(K)
        b, lw, lb, w2, b2 = (torch.randn(C, generator=g) for _ in range(5))
        R = torch.randn(M, C, generator=g)
        Ad, Av = _operand(A, kind)
        Wd, Wv = _operand(W, kind)
        t = Av @ Wv.t() + b.double() + (R.double() if with_r else 0)
        ref = torch.nn.functional.layer_norm(t, (C,), lw.double(), lb.double(), 1e-5)
        Y = torch.full((M, C), float("nan"), device=dev)
        Y2 = torch.full((M, C), float("nan"), device=dev) if y2 else None
        kw = dict(W2=w2.to(dev), B2=b2.to(dev), Y2=Y2) if y2 else {}
        N.gemm_ln(Ad.to(dev), Wd.to(dev), M=M, K=K, lda=K, ldw=K, bias=b.to(dev), R=R.to(dev) if with_r else None,
                  ldr=C if with_r else 0, ln_w=lw.to(dev), ln_b=lb.to(dev), eps=1e-5, Y=Y, **kw)
        e = _bound(kind, t, K, "f32")
        by = 2 * lw.abs().max().item() * e / t.std(-1, unbiased=False).min().item() + 2e-5 * ref.abs().max().item()
        checks = [("Y", (Y.cpu().double() - ref).abs().max().item(), by)]
        if y2:
            ref2 = torch.nn.functional.layer_norm(ref, (C,), w2.double(), b2.double(), 1e-5)
            b2y = (2 * w2.abs().max().item() * by / ref.std(-1, unbiased=False).min().item()
                   + 2e-5 * ref2.abs().max().item())
            checks.append(("Y2", (Y2.cpu().double() - ref2).abs().max().item(), b2y))
        return [Y] + ([Y2] if y2 else []), checks
    return run


CASES = {
    # gemm_x3_kernel, rows: 80 row tiles x 2 = 160 workgroups (the threshold), one valid row in the last tile
    "x3-rows-K32-f32": rows("pair", 20225, 256, 32),
    "x3-rows-K160-f32": rows("pair", 20225, 256, 160),
    "x3-rows-K160-pair-relu-pairR": rows("pair", 20225, 256, 160, cdt="pair", relu=True, rdt="pair"),
    "x3-rows-batch2": rows("pair", 10000, 256, 160, batch=2),
    "x3-rows-N1024-M7553-K64": rows("pair", 7553, 1024, 64, cdt="pair"),      # pair rows of the 128 x 128 shape
    "x3-rows-N1024-M7553-K192": rows("pair", 7553, 1024, 192),
    # gemm_x3_kernel, 3x3 conv rows: a tap is one 32-k stage, or two
    "x3-conv3x3-c32": conv3x3("pair", 1, 143, 143, 32, 256, cdt="pair"),
    "x3-conv3x3-c64": conv3x3("pair", 1, 143, 143, 64, 256),
    # LDS-DMA 64 x 64
    "dma64-f16-K64": rows("f16", 65, 64, 64, relu=True, rdt="f32"),
    "dma64-f16-K320": rows("f16", 65, 64, 320, cdt="f16"),
    "dma64-bf16-K64": rows("bf16", 65, 64, 64, cdt="bf16"),
    "dma64-bf16-K320": rows("bf16", 65, 64, 320, relu=True, rdt="bf16"),
    "dma64-pair-K64": rows("pair", 65, 64, 64, cdt="pair", relu=True, rdt="pair"),
    "dma64-pair-K320": rows("pair", 65, 64, 320),
    "dma64-f16-headsplit-rpb33": rows("f16", 66, 64, 64, cdt="f16", rpb=33),
    "dma64-bf16-headsplit-rpb70": rows("bf16", 140, 64, 64, cdt="bf16", rpb=70),
    "dma64-f16-headsplit-rpb70-f32": rows("f16", 140, 64, 64, rpb=70),
    "dma64-pair-headsplit-rpb33": rows("pair", 66, 64, 64, cdt="pair", rpb=33),
    "dma64-pair-headsplit-rpb70": rows("pair", 140, 64, 64, cdt="pair", rpb=70),
    "dma64-f16-splitk2": rows("f16", 65, 64, 256, k_splits=2, rdt="f32"),
    "dma64-pair-splitk2": rows("pair", 65, 64, 256, k_splits=2),
    "dma64-f16-conv1d3": conv1d3("f16", 5, 13, 64, 64),
    "dma64-pair-conv1d3": conv1d3("pair", 5, 13, 64, 64),
    "dma64-bf16-conv3x3": conv3x3("bf16", 2, 5, 7, 64, 64, in_m=True),
    "dma64-pair-conv3x3": conv3x3("pair", 2, 5, 7, 64, 64, in_m=True),
    "dma64-f16-a2select": rows("f16", 65, 256, 64, a2="select", a2_cols=128),
    "dma64-pair-a2select": rows("pair", 65, 256, 64, a2="select", a2_cols=128),
    # LDS-DMA 128 x 128: 8 x 60 = 480 tiles (the threshold), last row tile one row; a pair problem of this
    # shape with a row-mode C belongs to gemm_x3_kernel (above), head-split keeps it on this tile
    "dma128-f16-K64": rows("f16", 7553, 1024, 64, cdt="f16"),
    "dma128-bf16-K192": rows("bf16", 7553, 1024, 192, relu=True, rdt="f32"),
    "dma128-pair-K64-headsplit": rows("pair", 7553, 1024, 64, cdt="pair", rpb=581),
    "dma128-pair-K192-headsplit": rows("pair", 7553, 1024, 192, cdt="f16", rpb=7553),
    # LDS-DMA 128 x 64: 3 x 160 = 480 tiles, 16-bit 3 stages / pair 2
    "dma128x64-f16": rows("f16", 20353, 192, 512),
    "dma128x64-bf16": rows("bf16", 20353, 192, 512, cdt="bf16", relu=True),
    "dma128x64-pair": rows("pair", 20353, 192, 512, cdt="pair", rdt="f32"),
    # gemm_ln_kernel
    "ln-f16-K64-R": gemm_ln("f16", 33, 64, with_r=True),
    "ln-f16-K256": gemm_ln("f16", 33, 256, with_r=False),
    "ln-bf16-K64": gemm_ln("bf16", 33, 64, with_r=False),
    "ln-bf16-K256-R-Y2": gemm_ln("bf16", 33, 256, with_r=True, y2=True),
    "ln-pair-K64-R-Y2": gemm_ln("pair", 33, 64, with_r=True, y2=True),
    "ln-pair-K256": gemm_ln("pair", 33, 256, with_r=False),
    # conv_halo_x3_kernel: 323 pixels = two 256-pixel tiles, the second ragged
    "halo-pair-c16": halo("pair", 17, 19, 16, 128, cdt="f32"),
    "halo-pair-c48-second": halo("pair", 17, 19, 48, 128, cdt="pair", second=True),
    "halo-f16-c48-onepass": halo("f16", 17, 19, 48, 128, cdt="f16"),
    # gemm_lowp_kernel (fp32 A, 16-bit W): the three stage depths, A2 add, the 128 x 128 tile, conv1d3
    "lowp64-f16-K32": rows("f32", 65, 64, 32, wkind="f16", relu=True, rdt="f32"),
    "lowp64-bf16-K64": rows("f32", 65, 64, 64, wkind="bf16"),
    "lowp64-f16-K128": rows("f32", 65, 64, 128, wkind="f16", cdt="f16"),
    "lowp64-bf16-a2add": rows("f32", 65, 256, 64, wkind="bf16", a2="add", a2_cols=128),
    "lowp128-f16-K32": rows("f32", 6017, 1024, 32, wkind="f16"),
    "lowp64-f16-conv1d3": conv1d3("f32", 5, 13, 32, 64, wkind="f16"),
    # gemm_f32_kernel
    "f32-rows": rows("f32", 65, 64, 32, relu=True, rdt="f32"),
    "f32-conv3x3": conv3x3("f32", 2, 5, 7, 32, 64, in_m=True),
    "f32-conv1d3": conv1d3("f32", 5, 13, 32, 64),
}


def run_case(native, dev, cid):
    """(raw output tensors, [(name, max abs error, bound)]) of one table entry"""
    return CASES[cid](native, dev)


@pytest.mark.parametrize("cid", list(CASES))
def test_gemm_path(N, dev, cid):
    _, checks = run_case(N, dev, cid)
    for name, err, bound in checks:
        print(f"{cid} {name}: max abs err {err:.3e} (bound {bound:.3e})")
    for name, err, bound in checks:
        assert err <= bound, (cid, name, err, bound)
