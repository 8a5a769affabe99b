"""Training-path kernels (train.hip, attn_train.hip) against float64 CPU restatements at the
strides, edge shapes and saturated inputs that tests/test_gpu_train_kernels.py leaves out.
Every output buffer is pre-filled with NaN; strided outputs live in a parent buffer whose gap
columns and guard tail must come back bit-unchanged, strided inputs carry NaN in their gaps.

C-ABI arguments pinned per test (arguments the wrappers do not expose go through the raw struct):

test_det_loss_shapes            cmt_det_loss_args: R / ncls / Rb (0 rows, one trip and several trips of the
                                1 024-thread loop), labels (all background, all foreground, mixed), label_w
                                NULL / given, ld_logits / ld_boxes != width, dlogits / dboxes NULL, box_w == 0,
                                d == 0, two launches bit-equal
test_det_loss_gscale            gscale = 0.125 scales the gradients and not the losses
test_det_loss_saturated         logits up to +-104 as positive and as negative class, gamma 2 / 0 / 1.5
test_match_cost_shapes          cmt_match_cost_args: Nq / ngt, the query-row index of boxes, gt_labels 0 and
                                ncls - 1, ld_logits / ld_boxes, channels 8 / 9 (NaN) outside the cost,
                                code_w with zeros
test_match_cost_saturated       the logit grid: conditioning bound for |x| <= 8, the reference's own fp32
                                arithmetic as the yardstick beyond
test_ln_train_raw               cmt_ln_train_args: rows (not a multiple of 4, > 2 048 grouped rows, one row
                                per weight set), C 64 / 256, rows_per_wset, ldx / ldy / lddx != C,
                                accumulate, dW / dB added to / NULL
test_ln_train_common_offset     x = 1000 + noise, bound derived from rstd
test_ln_train_rejects           C = 128 and rows = 0 -> CMT_EINVAL
test_bn_relu_train_raw          cmt_bn_args: rows 1 / 63 / 65 / 1 000 / 40 000, C > 256 and C % 32 != 0, eps,
                                momentum, running_* given / NULL, dW / dB NULL, the Y > 0 gate on a tied column
test_bn_relu_train_40000_bitwise  run-to-run bit equality with 80 rows per block
test_adamw_and_sumsq            cmt_sumsq n 1 / 255 / 257 / 300 001 into a non-zero *out; cmt_adamw_args:
                                max_norm (clipped, not clipped, 0), sumsq NULL, weight_decay 0, step 1 / 2 / 1 000
test_im2col3x3_is_unfold        cmt_im2col3x3 bit for bit against unfold (1 x 1, one row, one column, ragged),
                                C = 6 rejected
test_attn_train_layouts         cmt_attn_train_args: q / k / v / o _bs / _hs / _rs of sequence-first, arena-slice
                                and head-split tensors, H 1 / 3, tiny Nq / Nk, fp16_inputs, dropout_p, LSE
test_attn_train_explicit_splits kv_splits 2 / 3 with workspace from cmt_attn_train_workspace_bytes
test_attn_train_hidden_split    a key split wholly hidden by the DN mask (the combine pass's l == 0 branch),
                                explicit and automatic split
"""
import ctypes
import math

import pytest
import torch
import torch.nn.functional as F

from test_gpu_train_kernels import dn_mask, keep_mask

pytestmark = pytest.mark.gpu

NAN = float("nan")
CMT_EINVAL = 1001
U = 2.0 ** -24          # fp32 unit roundoff


def _N():
    from projects.mmdet3d_plugin import native as N
    return N


def _call(name, a):
    N = _N()
    N._check(getattr(N.lib(), name)(ctypes.byref(a), N._stream()), name)


def _rc(name, a):
    N = _N()
    return getattr(N.lib(), name)(ctypes.byref(a), N._stream())


def _ptr(t):
    return None if t is None else t.data_ptr()


def _bits(t):
    return t.detach().cpu().contiguous().view(torch.int32)


class Buf:
    """A [rows, width] fp32 view at column ``off`` of a [rows, ld] parent followed by a guard tail,
    all in one flat device buffer filled with ``fill`` (NaN).  ``src`` (CPU) is copied into the view.
    check_gaps(): every element outside the view is bit-unchanged since construction / mark()."""
    TAIL = 64

    def __init__(self, dev, rows, width, ld=None, off=0, src=None, fill=NAN):
        ld = width if ld is None else ld
        assert off + width <= ld
        self.rows, self.width, self.ld, self.off = rows, width, ld, off
        self.flat = torch.full((rows * ld + self.TAIL,), fill, dtype=torch.float32, device=dev)
        self.view = self.flat[:rows * ld].view(rows, ld)[:, off:off + width]
        if src is not None:
            self.view.copy_(src.to(torch.float32))
        self.mark()

    def mark(self):
        self.before = self.flat.clone()

    @property
    def ptr(self):
        return self.flat.data_ptr() + 4 * self.off

    def cpu(self):
        return self.view.detach().cpu().double()

    def _outside(self, flat):
        f = flat.clone()
        f[:self.rows * self.ld].view(self.rows, self.ld)[:, self.off:self.off + self.width] = 0
        return _bits(f)

    def check_gaps(self, what=""):
        assert torch.equal(self._outside(self.flat), self._outside(self.before)), f"{what}: gap / guard tail written"


def _maxerr(got, want):
    """max |got - want|; NaN (an unwritten or non-finite element) stays NaN and fails any bound"""
    if want.numel() == 0:
        return 0.0
    return (got.double() - want.double()).abs().max().item()


# ---------------------------------------------------------------------------------------------
# 1. cmt_det_loss
# ---------------------------------------------------------------------------------------------
DET_CFG = dict(gamma=2.0, alpha=0.25, cls_weight=2.0, box_weight=0.25, cls_avg=37.5, box_avg=12.0)


def _det_ref(logits, labels, lw, boxes, tg, bw, cfg):
    from oracle import cmt_train_oracle as TO
    ld, bd = logits.double().requires_grad_(), boxes.double().requires_grad_()
    w = torch.ones(logits.shape[0], dtype=torch.float64) if lw is None else lw.double()
    lc = TO.focal_loss(ld, labels, w, cfg["gamma"], cfg["alpha"], cfg["cls_weight"], cfg["cls_avg"])
    lb = TO.l1_loss(bd, tg.double(), bw.double(), cfg["box_weight"], cfg["box_avg"])
    (lc + lb).backward()
    grads = [torch.zeros_like(t) if t.grad is None else t.grad for t in (ld, bd)]   # empty operands
    return lc.item(), lb.item(), grads[0], grads[1]


def _det_run(dev, logits, labels, lw, boxes, tg, bw, cfg, *, strided=False, need_grad=True, gscale=1.0):
    """cmt_det_loss through the raw struct; returns (out [2] cpu, dlogits, dboxes as float64 cpu or None)"""
    N = _N()
    R, ncls = logits.shape
    Rb = boxes.shape[0]
    ll, lo, lb_ = (16, 3, 12) if strided else (ncls, 0, 10)
    L = Buf(dev, R, ncls, ll, lo, src=logits)
    Bx = Buf(dev, Rb, 10, lb_, 0, src=boxes)
    dL = Buf(dev, R, ncls, ll, lo) if need_grad else None
    dB = Buf(dev, Rb, 10, lb_, 0) if need_grad else None
    out = Buf(dev, 1, 2)
    lab = labels.int().to(dev)
    lwd = None if lw is None else lw.to(dev)
    tgd, bwd = tg.contiguous().to(dev), bw.contiguous().to(dev)
    a = N.DetLossArgs()
    a.R, a.ncls, a.Rb = R, ncls, Rb
    a.logits, a.ld_logits, a.labels, a.label_w = L.ptr, ll, lab.data_ptr(), _ptr(lwd)
    a.boxes, a.ld_boxes, a.targets, a.box_w = Bx.ptr, lb_, tgd.data_ptr(), bwd.data_ptr()
    a.gamma, a.alpha, a.cls_weight, a.box_weight = cfg["gamma"], cfg["alpha"], cfg["cls_weight"], cfg["box_weight"]
    a.cls_avg, a.box_avg, a.gscale = cfg["cls_avg"], cfg["box_avg"], gscale
    a.out, a.dlogits, a.dboxes = out.ptr, (dL.ptr if dL else None), (dB.ptr if dB else None)
    _call("cmt_det_loss", a)
    torch.cuda.synchronize()
    out.check_gaps("det_loss out")
    for b, nm in ((dL, "dlogits"), (dB, "dboxes"), (L, "logits"), (Bx, "boxes")):
        if b is not None:
            b.check_gaps(nm)
    return out.view.cpu()[0], (dL.cpu() if dL else None), (dB.cpu() if dB else None)


def _det_check(got, ref, gscale=1.0, what=""):
    out, dl, db = got
    lc, lb, gl, gb = ref
    assert torch.isfinite(out).all(), what
    assert abs(out[0].item() - lc) < 1e-4 * max(1, abs(lc)), (what, out[0].item(), lc)
    assert abs(out[1].item() - lb) < 1e-4 * max(1, abs(lb)), (what, out[1].item(), lb)
    if dl is not None:
        e1, e2 = _maxerr(dl, gl * gscale), _maxerr(db, gb * gscale)
        assert (dl.numel() == 0 or e1 < 1e-5 * gscale) and (db.numel() == 0 or e2 < 1e-6 * gscale), (what, e1, e2)
        return e1, e2
    return 0.0, 0.0


def _det_inputs(R, ncls, Rb, labels_mode, seed=0):
    g = torch.Generator().manual_seed(1000 * R + 10 * ncls + Rb + seed)
    logits = torch.randn(R, ncls, generator=g) * 2
    if labels_mode == "bg":
        labels = torch.full((R,), ncls, dtype=torch.long)
    elif labels_mode == "fg":
        labels = torch.arange(R) % ncls
    else:
        labels = torch.randint(0, ncls + 1, (R,), generator=g)
    lw = torch.rand(R, generator=g)
    boxes = torch.randn(Rb, 10, generator=g)
    tg = torch.randn(Rb, 10, generator=g)
    bw = torch.rand(Rb, 10, generator=g)
    # exact ties (d == 0) and zero weights in the box term
    tie = (torch.arange(Rb * 10).view(Rb, 10) % 7) == 0
    tg = torch.where(tie, boxes, tg)
    zero_w = (torch.arange(Rb * 10).view(Rb, 10) % 5) == 1
    bw = torch.where(zero_w, torch.zeros(()), bw)
    return logits, labels, lw, boxes, tg, bw, tie, zero_w


@pytest.mark.parametrize("labels_mode", ["bg", "fg", "mixed"])
@pytest.mark.parametrize("R,ncls,Rb", [(1, 1, 1), (7, 3, 0), (0, 10, 5), (103, 10, 17), (1500, 2, 40)])
def test_det_loss_shapes(dev, parity_log, R, ncls, Rb, labels_mode):
    logits, labels, lw, boxes, tg, bw, tie, zero_w = _det_inputs(R, ncls, Rb, labels_mode)
    worst = (0.0, 0.0)
    for use_lw in (False, True):
        w = lw if use_lw else None
        ref = _det_ref(logits, labels, w, boxes, tg, bw, DET_CFG)
        for strided in (False, True):
            what = f"det_loss R={R} ncls={ncls} Rb={Rb} {labels_mode} lw={use_lw} strided={strided}"
            got = _det_run(dev, logits, labels, w, boxes, tg, bw, DET_CFG, strided=strided)
            e = _det_check(got, ref, what=what)
            worst = (max(worst[0], e[0]), max(worst[1], e[1]))
            # d == 0 and w == 0 give an exactly zero box gradient
            assert (got[2][tie] == 0).all() and (got[2][zero_w] == 0).all(), what
            # need_grad = False: NULL gradient pointers, the same losses bit for bit
            nog = _det_run(dev, logits, labels, w, boxes, tg, bw, DET_CFG, strided=strided, need_grad=False)
            _det_check(nog, ref, what=what + " no grad")
            assert torch.equal(_bits(nog[0]), _bits(got[0])), what
            # the header's fixed reduction order: a second launch is bit-equal
            again = _det_run(dev, logits, labels, w, boxes, tg, bw, DET_CFG, strided=strided)
            for x, y in zip(got, again):
                assert torch.equal(x.view(torch.int64), y.view(torch.int64)) if x.dtype == torch.float64 \
                    else torch.equal(_bits(x), _bits(y)), what
    parity_log.append(f"det_loss R={R} ncls={ncls} Rb={Rb} {labels_mode}: dlogits {worst[0]:.2e} (1e-5) "
                      f"dboxes {worst[1]:.2e} (1e-6)")


def test_det_loss_gscale(dev):
    logits, labels, lw, boxes, tg, bw, _, _ = _det_inputs(103, 10, 17, "mixed", seed=1)
    ref = _det_ref(logits, labels, lw, boxes, tg, bw, DET_CFG)
    one = _det_run(dev, logits, labels, lw, boxes, tg, bw, DET_CFG, strided=True)
    got = _det_run(dev, logits, labels, lw, boxes, tg, bw, DET_CFG, strided=True, gscale=0.125)
    _det_check(got, ref, gscale=0.125, what="gscale 0.125")
    assert torch.equal(_bits(got[0]), _bits(one[0]))                       # the losses do not scale
    assert torch.equal(got[1], one[1] * 0.125) and torch.equal(got[2], one[2] * 0.125)   # a power of two: exact


GRID = [s * v for v in (8.0, 15.0, 30.0, 60.0, 90.0, 104.0) for s in (1.0, -1.0)]


@pytest.mark.parametrize("gamma", [2.0, 0.0, 1.5])
def test_det_loss_saturated(dev, parity_log, gamma):
    """Each grid value once as the positive class (column 0, label 0) and once as a negative (column 1):
    1 - p and powf(1 - p, gamma) in fp32 lose all relative accuracy there, the losses and gradients must
    stay finite and within the dense-shape bounds (the lost terms are below them in absolute size)."""
    cfg = dict(DET_CFG, gamma=gamma)
    x = torch.tensor(GRID)
    logits = torch.stack([x, x], 1)
    labels = torch.zeros(len(GRID), dtype=torch.long)
    g = torch.Generator().manual_seed(4)
    lw = torch.rand(len(GRID), generator=g) + 0.5
    boxes, tg, bw = torch.randn(3, 10, generator=g), torch.randn(3, 10, generator=g), torch.rand(3, 10, generator=g)
    ref = _det_ref(logits, labels, lw, boxes, tg, bw, cfg)
    assert math.isfinite(ref[0]) and torch.isfinite(ref[2]).all()
    got = _det_run(dev, logits, labels, lw, boxes, tg, bw, cfg)
    assert torch.isfinite(got[1]).all() and torch.isfinite(got[2]).all()
    e = _det_check(got, ref, what=f"saturated gamma={gamma}")
    parity_log.append(f"det_loss saturated gamma={gamma}: loss {abs(got[0][0].item() - ref[0]):.2e} "
                      f"(1e-4 rel of {ref[0]:.3f}) dlogits {e[0]:.2e} (1e-5)")


# ---------------------------------------------------------------------------------------------
# 2. cmt_match_cost
# ---------------------------------------------------------------------------------------------
MC_CFG = dict(gamma=2.0, alpha=0.25, cls_weight=2.0, reg_weight=0.25)
CODE_W = torch.tensor([2.0, 2.0, 0.0, 1.0, 1.0, 0.0, 1.0, 1.0, 0.2, 0.2])


def _mc_run(dev, logits, boxes, gt, gl, cw, cfg, strided=False):
    N = _N()
    Nq, ncls = logits.shape
    ngt = gt.shape[0]
    ll, lo, lb_ = (16, 3, 12) if strided else (ncls, 0, 10)
    L = Buf(dev, Nq, ncls, ll, lo, src=logits)
    Bx = Buf(dev, Nq, 10, lb_, 0, src=boxes)
    cost = Buf(dev, Nq, ngt)
    gtd, gld, cwd = gt.contiguous().to(dev), gl.int().to(dev), cw.to(dev)
    a = N.MatchCostArgs()
    a.Nq, a.ngt = Nq, ngt
    a.logits, a.ld_logits, a.boxes, a.ld_boxes = L.ptr, ll, Bx.ptr, lb_
    a.gt, a.gt_labels, a.code_w = gtd.data_ptr(), gld.data_ptr(), cwd.data_ptr()
    a.gamma, a.alpha, a.cls_weight, a.reg_weight, a.cost = cfg["gamma"], cfg["alpha"], cfg["cls_weight"], \
        cfg["reg_weight"], cost.ptr
    _call("cmt_match_cost", a)
    torch.cuda.synchronize()
    cost.check_gaps("match cost")
    return cost.view.cpu()


def _mc_ref(logits, boxes, gt, gl, cw, cfg, dtype=torch.float64):
    from oracle import cmt_train_oracle as TO
    return TO.match_cost(logits.to(dtype), boxes.to(dtype), gt.to(dtype), gl, cw.to(dtype), cfg["cls_weight"],
                         cfg["reg_weight"], cfg["gamma"], cfg["alpha"])


def _mc_bound(x, ref, cfg):
    """Elementwise fp32 bound of the cost at logit x.  p = 1 / (1 + e^-x) carries three roundings
    (expf, the sum, the reciprocal; 1 - p is exact), so 1 - p (x > 0) has a relative error of up to
    3u (1 + e^|x|); through -log that is an absolute error of the same size, times the focal weight
    (<= max(alpha, 1 - alpha)) and cls_weight.  Every other operation (logf, powf, the products, the
    eight weighted differences and their sum: <= 16 roundings or libm ulps along any path) is relative
    to the size of the terms it feeds: 16 u A with A = cls_weight (|pos| + |neg|) + reg_weight l1."""
    x = x.double()
    p = x.sigmoid()
    neg = -(1 - p + 1e-12).log() * (1 - cfg["alpha"]) * p.pow(cfg["gamma"])
    pos = -(p + 1e-12).log() * cfg["alpha"] * (1 - p).pow(cfg["gamma"])
    reg = (ref - cfg["cls_weight"] * (pos - neg)).clamp_min(0)
    A = cfg["cls_weight"] * (pos + neg) + reg
    fw = max(cfg["alpha"], 1 - cfg["alpha"]) * cfg["cls_weight"]
    return fw * 3 * U * (1 + x.abs().exp()) + 16 * U * A


@pytest.mark.parametrize("strided", [False, True])
@pytest.mark.parametrize("Nq,ngt", [(1, 1), (37, 1), (900, 3), (300, 100)])
def test_match_cost_shapes(dev, parity_log, Nq, ngt, strided):
    """Independent boxes per query (a wrong row index on boxes shows), labels 0 and ncls - 1, NaN in
    channels 8 / 9 of boxes and GT (only 8 channels enter the cost), code weights with zeros."""
    ncls = 10
    g = torch.Generator().manual_seed(Nq * 131 + ngt)
    logits = (torch.randn(Nq, ncls, generator=g) * 2).clamp(-8, 8)
    boxes = torch.randn(Nq, 10, generator=g) * 3
    gt = torch.randn(ngt, 10, generator=g) * 3
    gl = torch.randint(0, ncls, (ngt,), generator=g)
    gl[0] = 0
    gl[-1] = ncls - 1 if ngt > 1 else 0
    if ngt == 1 and Nq > 1:
        gl[0] = ncls - 1
    ref = _mc_ref(logits, boxes, gt, gl, CODE_W, MC_CFG)
    got = _mc_run(dev, logits, boxes, gt, gl, CODE_W, MC_CFG, strided)
    bound = _mc_bound(logits[:, gl], ref, MC_CFG)
    err = (got.double() - ref).abs()
    assert torch.isfinite(got).all()
    assert (err <= bound).all(), (err.max().item(), bound.max().item())
    bn, gn = boxes.clone(), gt.clone()
    bn[:, 8:] = NAN
    gn[:, 8:] = NAN
    got_nan = _mc_run(dev, logits, bn, gn, gl, CODE_W, MC_CFG, strided)
    assert torch.isfinite(got_nan).all() and torch.equal(_bits(got_nan), _bits(got))
    parity_log.append(f"match_cost Nq={Nq} ngt={ngt} strided={strided}: {err.max().item():.2e} "
                      f"(elementwise, largest bound {bound.max().item():.2e})")


def test_match_cost_saturated(dev, parity_log):
    """The logit grid in every class column.  |x| <= 8: the conditioning bound of _mc_bound.  Beyond, the
    reference formula -(1 - p + 1e-12).log() is itself ill-conditioned in fp32 (the epsilon vanishes
    until p == 1): the kernel must stay finite and its worst error against float64 in each bucket
    (8 < |x| <= 16, |x| > 16) is at most twice that of the same formula evaluated in torch.float32 on
    the host (the factor covers the few-ulp difference of device and host expf / logf)."""
    ncls = 4
    vals = torch.tensor(GRID + [0.5, -2.0, 4.0, -6.0])
    Nq = len(vals)
    logits = torch.stack([vals.roll(c) for c in range(ncls)], 1)
    g = torch.Generator().manual_seed(8)
    boxes, gt = torch.randn(Nq, 10, generator=g), torch.randn(6, 10, generator=g)
    gl = torch.tensor([0, 1, 2, 3, 3, 0])
    ref = _mc_ref(logits, boxes, gt, gl, CODE_W, MC_CFG)
    host32 = _mc_ref(logits, boxes, gt, gl, CODE_W, MC_CFG, torch.float32)
    got = _mc_run(dev, logits, boxes, gt, gl, CODE_W, MC_CFG)
    assert torch.isfinite(got).all()
    x = logits[:, gl].abs()
    err, herr = (got.double() - ref).abs(), (host32.double() - ref).abs()
    lo = x <= 8
    assert (err[lo] <= _mc_bound(logits[:, gl], ref, MC_CFG)[lo]).all(), err[lo].max().item()
    parity_log.append(f"match_cost grid |x|<=8: {err[lo].max().item():.2e} (conditioning bound, elementwise)")
    for name, sel in (("8<|x|<=16", (x > 8) & (x <= 16)), ("|x|>16", x > 16)):
        k, h = err[sel].max().item(), herr[sel].max().item()
        parity_log.append(f"match_cost grid {name}: kernel {k:.3e} vs host fp32 formula {h:.3e} (bound 2x)")
        assert k <= 2 * h, (name, k, h)


# ---------------------------------------------------------------------------------------------
# 3. cmt_ln_train_fwd / bwd through the raw struct
# ---------------------------------------------------------------------------------------------
def _ln_ref(x, w, b, dy, sets, eps):
    rows, C = x.shape
    xd, wd, bd = (t.double().requires_grad_() for t in (x, w, b))
    R = rows // sets
    ref = torch.cat([F.layer_norm(xd[i * R:(i + 1) * R], (C,), wd[i * C:(i + 1) * C], bd[i * C:(i + 1) * C], eps)
                     for i in range(sets)])
    ref.backward(dy.double())
    mean = x.double().mean(1)
    rstd = (x.double().var(1, unbiased=False) + eps).rsqrt()
    return ref.detach(), xd.grad, wd.grad, bd.grad, mean, rstd


def _ln_run(dev, x, w, b, dy, sets, eps, *, strided, accumulate=False, null_dw=False, seed=0):
    """forward then backward; returns float64 cpu (y, mean, rstd, dx, dw, db, dx_old, dw_old, db_old)"""
    N = _N()
    rows, C = x.shape
    ldx, ldy, lddx = (C + 8, C + 4, C + 12) if strided else (C, C, C)
    g = torch.Generator().manual_seed(77 + seed)
    X = Buf(dev, rows, C, ldx, src=x)
    Y = Buf(dev, rows, C, ldy)
    mean, rstd = Buf(dev, 1, rows), Buf(dev, 1, rows)
    wd_, bd_ = w.to(dev), b.to(dev)
    a = N.LnTrainArgs()
    a.rows, a.C, a.X, a.ldx, a.W, a.B, a.eps = rows, C, X.ptr, ldx, wd_.data_ptr(), bd_.data_ptr(), eps
    a.rows_per_wset = rows // sets if sets > 1 else 0
    a.Y, a.ldy, a.mean, a.rstd = Y.ptr, ldy, mean.ptr, rstd.ptr
    _call("cmt_ln_train_fwd", a)
    torch.cuda.synchronize()
    for bf, nm in ((X, "X"), (Y, "Y"), (mean, "mean"), (rstd, "rstd")):
        bf.check_gaps("ln fwd " + nm)
    y = Y.cpu()
    dY = Buf(dev, rows, C, ldy, src=dy)
    dx_old = torch.randn(rows, C, generator=g) if accumulate else None
    dX = Buf(dev, rows, C, lddx, src=dx_old)
    dw_old, db_old = torch.randn(sets * C, generator=g), torch.randn(sets * C, generator=g)
    dW = None if null_dw else Buf(dev, 1, sets * C, src=dw_old[None])
    dB = None if null_dw else Buf(dev, 1, sets * C, src=db_old[None])
    a.Y = None
    a.dY, a.dX, a.lddx, a.accumulate = dY.ptr, dX.ptr, lddx, int(accumulate)
    a.dW, a.dB = (dW.ptr if dW else None), (dB.ptr if dB else None)
    _call("cmt_ln_train_bwd", a)
    torch.cuda.synchronize()
    for bf, nm in ((X, "X"), (dY, "dY"), (dX, "dX"), (dW, "dW"), (dB, "dB"), (mean, "mean"), (rstd, "rstd")):
        if bf is not None:
            bf.check_gaps("ln bwd " + nm)
    return dict(y=y, mean=mean.cpu()[0], rstd=rstd.cpu()[0], dx=dX.cpu(), dw=dW.cpu()[0] if dW else None,
                db=dB.cpu()[0] if dB else None, dx_old=dx_old, dw_old=dw_old, db_old=db_old)


@pytest.mark.parametrize("variant", ["dense", "strided", "strided+accumulate", "strided+null_dw"])
@pytest.mark.parametrize("rows,C,sets", [(1, 256, 1), (5, 64, 1), (333, 64, 1), (6, 256, 3), (2100, 64, 7),
                                         (9, 64, 9)])
def test_ln_train_raw(dev, parity_log, rows, C, sets, variant):
    eps = 1e-5
    g = torch.Generator().manual_seed(rows * 3 + C + sets)
    x = torch.randn(rows, C, generator=g) * 2 + 0.5
    w, b = torch.randn(sets * C, generator=g), torch.randn(sets * C, generator=g)
    dy = torch.randn(rows, C, generator=g)
    want_y, want_dx, want_dw, want_db, want_mean, want_rstd = _ln_ref(x, w, b, dy, sets, eps)
    acc, null_dw = "accumulate" in variant, "null_dw" in variant
    r = _ln_run(dev, x, w, b, dy, sets, eps, strided="strided" in variant, accumulate=acc, null_dw=null_dw)
    ey = _maxerr(r["y"], want_y)
    assert ey < 1e-5, ey
    assert _maxerr(r["mean"], want_mean) < 1e-5
    assert ((r["rstd"] - want_rstd).abs() / want_rstd).max().item() < 1e-5
    if acc:
        want_dx = want_dx + r["dx_old"].double()          # accumulate: old + gradient
    edx = _maxerr(r["dx"], want_dx)
    assert edx < 1e-4 * max(1.0, want_dx.abs().max().item()), edx
    if not null_dw:
        # the kernel ADDS its column sums to dW / dB (the dw_into contract of ln_train_bwd)
        for got, old, want in ((r["dw"], r["dw_old"], want_dw), (r["db"], r["db_old"], want_db)):
            e = _maxerr(got, old.double() + want)
            assert e < 1e-4 * max(1.0, want.abs().max().item()), e
    parity_log.append(f"ln_train rows={rows} C={C} sets={sets} {variant}: y {ey:.2e} (1e-5) dx {edx:.2e} (1e-4)")


@pytest.mark.parametrize("rows,C,sets", [(333, 64, 1), (6, 256, 3)])
def test_ln_train_common_offset(dev, parity_log, rows, C, sets):
    """x = 1000 + noise, against float64 of the same fp32 inputs.  The row mean is a sum of C values
    near 1000 in C/64 - 1 sequential adds, 6 shuffle levels and a division: E = C/64 + 6 roundings of
    relative size u at |x| ~ 1000 (the variance is taken from centred values and keeps its relative
    accuracy).  dm = E u max|x| shifts xhat by dx = dm rstd, so
      y:      1e-5 + dx |w|
      dX:     1e-4 max(1, |want|) + rstd dx max|dy w| (1 + max|xhat|)   (the two projections)
      dW:     1e-4 max(1, |want|) + dx max_c sum_rows |dy|;   dB does not see xhat."""
    eps = 1e-5
    g = torch.Generator().manual_seed(rows + C)
    x = 1000.0 + torch.randn(rows, C, generator=g)
    w, b = torch.randn(sets * C, generator=g), torch.randn(sets * C, generator=g)
    dy = torch.randn(rows, C, generator=g)
    want_y, want_dx, want_dw, want_db, want_mean, want_rstd = _ln_ref(x, w, b, dy, sets, eps)
    r = _ln_run(dev, x, w, b, dy, sets, eps, strided=True)
    dm = (C // 64 + 6) * U * x.abs().max().item()
    rstd = want_rstd.max().item()
    dxh = dm * rstd
    xh_max = ((x.double() - want_mean[:, None]) * want_rstd[:, None]).abs().max().item()
    R = rows // sets
    wrow = w.view(sets, 1, C).expand(sets, R, C).reshape(rows, C)
    gw_max = (dy * wrow).abs().max().item()
    by = 1e-5 + dxh * w.abs().max().item()
    bdx = 1e-4 * max(1.0, want_dx.abs().max().item()) + rstd * dxh * gw_max * (1 + xh_max)
    bdw = 1e-4 * max(1.0, want_dw.abs().max().item()) + dy.abs().view(sets, R, C).sum(1).max().item() * dxh
    em, ey, edx = _maxerr(r["mean"], want_mean), _maxerr(r["y"], want_y), _maxerr(r["dx"], want_dx)
    edw, edb = _maxerr(r["dw"], r["dw_old"].double() + want_dw), _maxerr(r["db"], r["db_old"].double() + want_db)
    parity_log.append(f"ln_train offset 1000 rows={rows} C={C}: mean {em:.2e} ({dm:.2e}) y {ey:.2e} ({by:.2e}) "
                      f"dx {edx:.2e} ({bdx:.2e}) dw {edw:.2e} ({bdw:.2e})")
    assert em <= dm and ey < by and edx < bdx and edw < bdw
    assert ((r["rstd"] - want_rstd).abs() / want_rstd).max().item() < 1e-5 + 2 * dm * dm   # centred squares
    assert edb < 1e-4 * max(1.0, want_db.abs().max().item())


def test_ln_train_rejects(dev):
    N = _N()
    for rows, C in ((8, 128), (0, 64)):
        X = Buf(dev, max(rows, 1), C)
        v = torch.zeros(max(rows, 1) * C, device=dev)
        a = N.LnTrainArgs()
        a.rows, a.C, a.X, a.ldx, a.W, a.B, a.eps = rows, C, X.ptr, C, v.data_ptr(), v.data_ptr(), 1e-5
        a.Y, a.ldy, a.mean, a.rstd = X.ptr, C, v.data_ptr(), v.data_ptr()
        a.dY, a.dX, a.lddx = X.ptr, X.ptr, C
        assert _rc("cmt_ln_train_fwd", a) == CMT_EINVAL
        assert _rc("cmt_ln_train_bwd", a) == CMT_EINVAL
        torch.cuda.synchronize()
        X.check_gaps("rejected launch")
        assert torch.isnan(X.view).all()


# ---------------------------------------------------------------------------------------------
# 4. cmt_bn_relu_train_fwd / bwd
# ---------------------------------------------------------------------------------------------
BN_EPS, BN_MOM = 1e-3, 0.3


def _bn_inputs(rows, C):
    g = torch.Generator().manual_seed(rows * 7 + C)
    x = torch.randn(rows, C, generator=g) * 2 + 0.5
    w = torch.rand(C, generator=g) + 0.5
    b = torch.rand(C, generator=g) - 0.5
    w[1], b[1] = 0.0, 0.0     # a pre-activation of exactly 0 in every row: Y > 0 is the gradient gate
    dy = torch.randn(rows, C, generator=g)
    rm, rv = torch.randn(C, generator=g), torch.rand(C, generator=g) + 0.5
    return x, w, b, dy, rm, rv


def _bn_ref(x, w, b, dy, rm, rv):
    xd, wd, bd = (t.double().requires_grad_() for t in (x, w, b))
    rm, rv = rm.double().clone(), rv.double().clone()
    rows = x.shape[0]
    mean, var = xd.detach().mean(0), xd.detach().var(0, unbiased=False)
    if rows > 1:
        y = torch.relu(F.batch_norm(xd, rm, rv, wd, bd, True, BN_MOM, BN_EPS))
    else:
        # torch refuses one value per channel; the kernel's contract there: the biased variance (0)
        # also feeds running_var
        m1 = xd.mean(0)
        v1 = ((xd - m1) ** 2).mean(0)
        y = torch.relu((xd - m1) * (v1 + BN_EPS).rsqrt() * wd + bd)
        rm = (1 - BN_MOM) * rm + BN_MOM * mean
        rv = (1 - BN_MOM) * rv + BN_MOM * var
    y.backward(dy.double())
    return y.detach(), xd.grad, wd.grad, bd.grad, mean, (var + BN_EPS).rsqrt(), rm, rv


def _bn_run(dev, x, w, b, dy, rm, rv, *, running=True, null_dw=False):
    N = _N()
    rows, C = x.shape
    X, Y, dX = Buf(dev, rows, C, src=x), Buf(dev, rows, C), Buf(dev, rows, C)
    dY = Buf(dev, rows, C, src=dy)
    mean, rstd = Buf(dev, 1, C), Buf(dev, 1, C)
    RM, RV = (Buf(dev, 1, C, src=rm[None]), Buf(dev, 1, C, src=rv[None])) if running else (None, None)
    dW, dB = (None, None) if null_dw else (Buf(dev, 1, C), Buf(dev, 1, C))
    wd_, bd_ = w.to(dev), b.to(dev)
    ws = torch.empty(int(N.lib().cmt_bn_workspace_bytes(C)), dtype=torch.uint8, device=dev)
    a = N.BnArgs()
    a.rows, a.C, a.X, a.Y, a.W, a.B, a.eps, a.momentum = rows, C, X.ptr, Y.ptr, wd_.data_ptr(), bd_.data_ptr(), \
        BN_EPS, BN_MOM
    a.running_mean, a.running_var = (RM.ptr if RM else None), (RV.ptr if RV else None)
    a.mean_save, a.rstd_save, a.workspace = mean.ptr, rstd.ptr, ws.data_ptr()
    _call("cmt_bn_relu_train_fwd", a)
    a.running_mean = a.running_var = None
    a.dY, a.dX, a.dW, a.dB = dY.ptr, dX.ptr, (dW.ptr if dW else None), (dB.ptr if dB else None)
    _call("cmt_bn_relu_train_bwd", a)
    torch.cuda.synchronize()
    for bf in (X, Y, dX, dY, mean, rstd, RM, RV, dW, dB):
        if bf is not None:
            bf.check_gaps("bn")
    one = lambda t: None if t is None else t.cpu()[0]   # noqa: E731
    return dict(y=Y.cpu(), dx=dX.cpu(), mean=one(mean), rstd=one(rstd), rm=one(RM), rv=one(RV), dw=one(dW),
                db=one(dB))


@pytest.mark.parametrize("variant", ["running", "no_running", "null_dw"])
@pytest.mark.parametrize("rows,C", [(1, 8), (63, 96), (65, 300), (1000, 40), (40000, 8)])
def test_bn_relu_train_raw(dev, parity_log, rows, C, variant):
    """Bounds of the existing BatchNorm tests (y 1e-4, dW / dB 1e-3, mean 1e-5, rstd 1e-5 relative,
    running mean / var 1e-5 / 1e-4), dX at 1e-4 max(1, |want|) like the LayerNorm backward.  At 40 000
    rows the column sums are 80 sequential adds per block, 63 per reduction group and 8 group sums; a
    random walk of their roundings is about 2u sqrt(rows * 151) rms(term) ~ 4e-4 for terms of size ~1,
    inside the 1e-3 the smaller shapes use, so no bound moves."""
    x, w, b, dy, rm, rv = _bn_inputs(rows, C)
    want = dict(zip(("y", "dx", "dw", "db", "mean", "rstd", "rm", "rv"), _bn_ref(x, w, b, dy, rm, rv)))
    r = _bn_run(dev, x, w, b, dy, rm, rv, running=variant != "no_running", null_dw=variant == "null_dw")
    e = {k: _maxerr(r[k], want[k]) for k in r if r[k] is not None and k != "rstd"}
    e["rstd"] = ((r["rstd"] - want["rstd"]).abs() / want["rstd"]).max().item()
    parity_log.append(f"bn_relu_train rows={rows} C={C} {variant}: " + " ".join(f"{k} {v:.2e}" for k, v in e.items()))
    assert e["y"] < 1e-4 and e["mean"] < 1e-5 and e["rstd"] < 1e-5
    assert e["dx"] < 1e-4 * max(1.0, want["dx"].abs().max().item())
    # the tied column: y == 0 in every row, so no gradient passes
    assert (r["y"][:, 1] == 0).all() and (r["dx"][:, 1] == 0).all()
    if variant != "no_running":
        assert e["rm"] < 1e-5 and e["rv"] < 1e-4
    if variant != "null_dw":
        assert e["dw"] < 1e-3 and e["db"] < 1e-3
        assert r["dw"][1] == 0 and r["db"][1] == 0


def test_bn_relu_train_40000_bitwise(dev):
    x, w, b, dy, rm, rv = _bn_inputs(40000, 8)
    r0 = _bn_run(dev, x, w, b, dy, rm, rv)
    r1 = _bn_run(dev, x, w, b, dy, rm, rv)
    for k in r0:
        assert torch.equal(r0[k].view(torch.int64), r1[k].view(torch.int64)), k


# ---------------------------------------------------------------------------------------------
# 5. cmt_sumsq / cmt_adamw_step
# ---------------------------------------------------------------------------------------------
LR, B1, B2, ADAM_EPS = 1e-3, 0.9, 0.999, 1e-8


def _adam64(p, g, m, v, step, wd, coef):
    g = g * coef
    p = p * (1 - LR * wd)
    m = B1 * m + (1 - B1) * g
    v = B2 * v + (1 - B2) * g * g
    bc1, bc2 = 1 - B1 ** step, 1 - B2 ** step
    return p - (LR / bc1) * m / (v.sqrt() / math.sqrt(bc2) + ADAM_EPS), m, v


@pytest.mark.parametrize("cfg,step,wd", [("clipped", 1, 0.5), ("unclipped", 2, 0.5), ("no_clip_null", 1000, 0.5),
                                         ("clipped", 1000, 0.0), ("unclipped", 1, 0.0), ("clipped", 2, 0.5)])
@pytest.mark.parametrize("n", [1, 255, 257, 300001])
def test_adamw_and_sumsq(dev, parity_log, n, cfg, step, wd):
    """One AdamW step with clip_grad_norm_ against a float64 restatement; the moments come from a few
    float64 steps.  Bounds: (1 - beta) is formed from the fp32 beta, relative error u beta / (1 - beta)
    (6e-5 at beta2 = 0.999) on the new-gradient term of each moment; the update p_new - p_old is held
    to 2e-4 of its largest element (the bias correction 1 - beta2^step carries the same 6e-5, halved by
    the square root, plus a few fp32 roundings).  The update is read off fp32 parameters, so it also
    carries their two roundings, 2 u |p|: parameters of size 0.01 keep that below 2e-4 of the update
    even where one element's moments happen to give a 1e-5 step (n = 1), and weight_decay = 0.5 makes
    the decay term lr wd p at least 2e-3 of the update, ten times the bound, so a dropped decay fails."""
    N = _N()
    gen = torch.Generator().manual_seed(n + step)
    p0 = (torch.randn(n, generator=gen) * 0.01).float()
    m64, v64 = torch.zeros(n, dtype=torch.float64), torch.zeros(n, dtype=torch.float64)
    p64 = p0.double()
    for s in range(1, min(step, 6)):       # moments carried in from a float64 run
        g = torch.randn(n, generator=gen).double() * 3
        _, m64, v64 = _adam64(p64, g, m64, v64, s, wd, 1.0)
    m0, v0 = m64.float(), v64.float()
    grad = (torch.randn(n, generator=gen) * 3).float()
    norm = grad.double().norm().item()
    max_norm = {"clipped": 0.5 * norm, "unclipped": 2.0 * norm + 1.0, "no_clip_null": 0.0}[cfg]
    coef = min(1.0, max_norm / (norm + 1e-6)) if max_norm > 0 else 1.0
    if cfg == "clipped":
        assert coef < 0.51
    want_p, want_m, want_v = _adam64(p0.double(), grad.double(), m0.double(), v0.double(), step, wd, coef)

    P, G = Buf(dev, 1, n, src=p0[None]), Buf(dev, 1, n, src=grad[None])
    M, V = Buf(dev, 1, n, src=m0[None]), Buf(dev, 1, n, src=v0[None])
    ss = None
    if cfg != "no_clip_null":
        # cmt_sumsq ADDS into *out: start from a non-zero value, check, then remove it again
        ss = Buf(dev, 1, 1, src=torch.tensor([[3.5]]))
        N._check(N.lib().cmt_sumsq(G.ptr, n, ss.ptr, N._stream()), "cmt_sumsq")
        torch.cuda.synchronize()
        ss.check_gaps("sumsq")
        got_ss = ss.cpu().item()
        # per-thread sums of <= 2 squares, 6 shuffle levels, then one atomic per wave (<= 4 096): a random
        # walk of roundings, 2 u (sqrt(waves) + 8) relative (all terms are positive)
        waves = min(-(-n // 256), 1024) * 4
        bss = 2 * U * (math.sqrt(waves) + 8)
        ess = abs(got_ss - (3.5 + norm * norm)) / (3.5 + norm * norm)
        parity_log.append(f"sumsq n={n}: rel {ess:.2e} ({bss:.2e})")
        assert ess < bss
        ss.view.fill_(float(torch.tensor(norm * norm, dtype=torch.float64).float()))
        ss.mark()
    a = N.AdamwArgs()
    a.n, a.step, a.lr, a.beta1, a.beta2, a.eps = n, step, LR, B1, B2, ADAM_EPS
    a.weight_decay, a.max_norm = wd, max_norm
    a.param, a.grad, a.exp_avg, a.exp_avg_sq, a.sumsq = P.ptr, G.ptr, M.ptr, V.ptr, (ss.ptr if ss else None)
    _call("cmt_adamw_step", a)
    torch.cuda.synchronize()
    for bf in (P, G, M, V, ss):
        if bf is not None:
            bf.check_gaps("adamw")
    assert torch.equal(_bits(G.view), _bits(grad[None]))          # the gradient is not rescaled in place
    gc = grad.double().abs() * coef
    em = ((M.cpu()[0] - want_m).abs() - (U * B1 / (1 - B1) + 8 * U) * (B1 * m0.double().abs() + (1 - B1) * gc)).max().item()
    ev = ((V.cpu()[0] - want_v).abs() / want_v.clamp_min(1e-30)).max().item()
    bv = U * B2 / (1 - B2) + 12 * U
    upd, want_upd = P.cpu()[0] - p0.double(), want_p - p0.double()
    eu = (upd - want_upd).abs().max().item() / want_upd.abs().max().item()
    parity_log.append(f"adamw n={n} {cfg} step={step} wd={wd}: exp_avg_sq rel {ev:.2e} ({bv:.2e}) update rel {eu:.2e} "
                      f"(2e-4)")
    assert em <= 0, em
    assert ev < bv
    assert eu < 2e-4


# ---------------------------------------------------------------------------------------------
# 6. cmt_im2col3x3
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("nimg,H,W,C", [(1, 1, 1, 4), (2, 1, 7, 8), (1, 5, 1, 4), (2, 9, 11, 36)])
def test_im2col3x3_is_unfold(dev, nimg, H, W, C):
    """a copy: bit-exact against unfold (NCHW, channel-major taps) rearranged to tap-major NHWC rows"""
    N = _N()
    g = torch.Generator().manual_seed(H * W + C)
    x = torch.randn(nimg, C, H, W, generator=g)
    want = F.unfold(x, 3, padding=1).view(nimg, C, 9, H * W).permute(0, 3, 2, 1).reshape(nimg * H * W, 9 * C)
    X = Buf(dev, nimg * H * W, C, src=x.permute(0, 2, 3, 1).reshape(-1, C))
    out = Buf(dev, nimg * H * W, 9 * C)
    N._check(N.lib().cmt_im2col3x3(X.ptr, nimg, H, W, C, out.ptr, N._stream()), "cmt_im2col3x3")
    torch.cuda.synchronize()
    out.check_gaps("im2col")
    X.check_gaps("im2col input")
    assert torch.equal(_bits(out.view), _bits(want))


def test_im2col3x3_rejects_c6(dev):
    N = _N()
    X, out = Buf(dev, 4, 6), Buf(dev, 4, 54)
    assert N.lib().cmt_im2col3x3(X.ptr, 1, 2, 2, 6, out.ptr, N._stream()) == CMT_EINVAL
    torch.cuda.synchronize()
    out.check_gaps("rejected im2col")
    assert torch.isnan(out.view).all()


# ---------------------------------------------------------------------------------------------
# 7. cmt_attn_train_fwd / bwd
# ---------------------------------------------------------------------------------------------
class Heads:
    """A logical [B, H, N, 32] fp32 device tensor laid out as ``layout`` inside a NaN-filled flat buffer
    with a guard tail: "dense" [B, N, H*32], "seq" [N, B, H*32], "heads" [B, H, N, 32], or slot 0..2 of
    an arena [B, N, 3*H*32] (several Heads may share one arena buffer)."""
    TAIL = 64

    def __init__(self, dev, B, H, N, layout, src=None, arena=None):
        C = H * 32
        width = 3 * C if isinstance(layout, int) else C
        if arena is None:
            arena = torch.full((B * N * width + self.TAIL,), NAN, dtype=torch.float32, device=dev)
        self.flat = arena
        body = self.flat[:B * N * width]
        if layout == "dense":
            v = body.view(B, N, H, 32).permute(0, 2, 1, 3)
        elif layout == "seq":
            v = body.view(N, B, H, 32).permute(1, 2, 0, 3)
        elif layout == "heads":
            v = body.view(B, H, N, 32)
        else:
            v = body.view(B, N, 3, H, 32)[:, :, layout].permute(0, 2, 1, 3)
        self.view = v
        self.strides = (v.stride(0), v.stride(1), v.stride(2))
        if src is not None:
            v.copy_(src.to(torch.float32))

    @property
    def ptr(self):
        return self.view.data_ptr()

    def cpu(self):
        return self.view.detach().cpu().double()


def _outside_bits(flat, views):
    f = flat.clone()
    for v in views:   # the views alias ``flat``; rebuild them on the clone
        torch.as_strided(f, v.shape, v.stride(), v.storage_offset() - flat.storage_offset()).zero_()
    return _bits(f)


def _attn_ref(q, k, v, do, *, pad, grp, fp16, p, seed):
    """float64 autograd of softmax(q k^T / sqrt(32) + DN mask) (hash dropout) v on [B, H, N, 32];
    LSE in base 2 (before dropout)"""
    B, H, Nq, _ = q.shape
    Nk = k.shape[2]

    def r(t):
        return t.half().double() if fp16 else t
    qd, kd, vd = (t.double().requires_grad_() for t in (q, k, v))
    s = r(qd) @ r(kd).transpose(-1, -2) / math.sqrt(32)
    if pad:
        s = s.masked_fill(dn_mask(Nq, Nk, pad, grp), float("-inf"))
    lse2 = torch.logsumexp(s.detach(), -1) / math.log(2.0)
    pr = torch.softmax(s, -1)
    if p > 0:
        pr = pr * keep_mask(seed, B, H, Nq, Nk, p).double() / (1 - p)
    out = pr @ r(vd)
    out.backward(do.double())
    return out.detach(), lse2, qd.grad, kd.grad, vd.grad


def _attn_run(dev, q, k, v, do, *, layout, pad=0, grp=0, fp16=False, p=0.0, seed=1234, kv_splits=0):
    """raw cmt_attn_train_fwd + bwd; q / k / v / do are CPU [B, H, N, 32]; returns float64 cpu
    (o, lse, dq, dk, dv) after checking every gap and guard tail"""
    N = _N()
    B, H, Nq, _ = q.shape
    Nk = k.shape[2]
    if layout == "arena":
        kv = Heads(dev, B, H, Nk, 1).flat
        K, V = Heads(dev, B, H, Nk, 1, src=k, arena=kv), Heads(dev, B, H, Nk, 2, src=v, arena=kv)
        dkv = Heads(dev, B, H, Nk, 1).flat
        dK, dV = Heads(dev, B, H, Nk, 1, arena=dkv), Heads(dev, B, H, Nk, 2, arena=dkv)
        ql = "dense"
    else:
        K, V = Heads(dev, B, H, Nk, layout, src=k), Heads(dev, B, H, Nk, layout, src=v)
        dK, dV = Heads(dev, B, H, Nk, layout), Heads(dev, B, H, Nk, layout)
        ql = layout
    Q, dO = Heads(dev, B, H, Nq, ql, src=q), Heads(dev, B, H, Nq, ql, src=do)
    O, dQ = Heads(dev, B, H, Nq, ql), Heads(dev, B, H, Nq, ql)
    lse, delta = Buf(dev, 1, B * H * Nq), Buf(dev, 1, B * H * Nq)
    groups = [(Q.flat, [Q.view]), (dO.flat, [dO.view]), (O.flat, [O.view]), (dQ.flat, [dQ.view])]
    if layout == "arena":
        groups += [(K.flat, [K.view, V.view]), (dK.flat, [dK.view, dV.view])]
    else:
        groups += [(t.flat, [t.view]) for t in (K, V, dK, dV)]
    before = [_outside_bits(f, vs) for f, vs in groups]
    a = N.AttnTrainArgs()
    a.B, a.H, a.Nq, a.Nk = B, H, Nq, Nk
    a.Q, (a.q_bs, a.q_hs, a.q_rs) = Q.ptr, Q.strides
    a.K, (a.k_bs, a.k_hs, a.k_rs) = K.ptr, K.strides
    a.V, (a.v_bs, a.v_hs, a.v_rs) = V.ptr, V.strides
    a.O, (a.o_bs, a.o_hs, a.o_rs) = O.ptr, O.strides
    a.LSE = lse.ptr
    a.scale, a.dn_pad, a.dn_group = 1 / math.sqrt(32), pad, grp
    a.fp16_inputs, a.dropout_p, a.seed, a.kv_splits = int(fp16), p, seed, kv_splits
    need = N.lib().cmt_attn_train_workspace_bytes(ctypes.byref(a))
    ws = None
    if need > 0:
        ws = torch.full((need // 4 + Buf.TAIL,), NAN, dtype=torch.float32, device=dev)
        a.workspace, a.workspace_bytes = ws.data_ptr(), need
    _call("cmt_attn_train_fwd", a)
    a.dO, a.dQ, a.dK, a.dV, a.delta = dO.ptr, dQ.ptr, dK.ptr, dV.ptr, delta.ptr
    _call("cmt_attn_train_bwd", a)
    torch.cuda.synchronize()
    for (f, vs), b4 in zip(groups, before):
        assert torch.equal(_outside_bits(f, vs), b4), "attention: gap or guard tail written"
    lse.check_gaps("LSE")
    delta.check_gaps("delta")
    if ws is not None:
        assert torch.isnan(ws[need // 4:]).all(), "workspace overrun"
    return O.cpu(), lse.cpu()[0].view(B, H, Nq), dQ.cpu(), dK.cpu(), dV.cpu(), need


def _attn_case(dev, parity_log, name, *, B, H, Nq, Nk, layout, pad=0, grp=0, fp16=False, p=0.0, kv_splits=0):
    g = torch.Generator().manual_seed(Nq * 7 + Nk + H)
    q, k, v, do = (torch.randn(B, H, n, 32, generator=g) for n in (Nq, Nk, Nk, Nq))
    seed = 1234
    want = _attn_ref(q, k, v, do, pad=pad, grp=grp, fp16=fp16, p=p, seed=seed)
    assert all(torch.isfinite(t).all() for t in want)        # no fully masked row
    *got, need = _attn_run(dev, q, k, v, do, layout=layout, pad=pad, grp=grp, fp16=fp16, p=p, seed=seed,
                           kv_splits=kv_splits)
    tol_o, tol_g = (2e-3, 5e-3) if fp16 else (2e-5, 2e-5)
    eo = _maxerr(got[0], want[0])
    el = _maxerr(got[1], want[1])
    # relative to the largest gradient, and to 1 where the gradient vanishes (one key: dQ == 0 is the
    # cancellation of unit-size terms)
    eg = [_maxerr(gt_, wt) / max(wt.abs().max().item(), 1.0) for gt_, wt in zip(got[2:], want[2:])]
    parity_log.append(f"attn_train {name} fp16={fp16} p={p}: o {eo:.2e} ({tol_o}) lse {el:.2e} dq/dk/dv "
                      + "/".join(f"{e:.2e}" for e in eg) + f" ({tol_g})")
    assert eo < tol_o, (name, eo)
    # LSE = m + log2(l): fp32 roundings of a value of size |lse| and of the sum l, like the output
    assert el < tol_o * max(1.0, want[1].abs().max().item()), (name, el)
    for e, nm in zip(eg, ("dq", "dk", "dv")):
        assert e < tol_g, (name, nm, e)
    return need


@pytest.mark.parametrize("B,Nq,Nk", [(1, 1, 1), (2, 5, 33), (1, 33, 64), (1, 130, 65)])
@pytest.mark.parametrize("H", [1, 3])
@pytest.mark.parametrize("layout", ["seq", "arena", "heads"])
def test_attn_train_layouts(dev, parity_log, layout, H, B, Nq, Nk):
    lines = []
    for fp16 in (False, True):
        for p in (0.0, 0.25):
            _attn_case(dev, lines, f"{layout} H={H} B={B} {Nq}x{Nk}", B=B, H=H, Nq=Nq, Nk=Nk, layout=layout,
                       fp16=fp16, p=p)
    parity_log.extend(lines[1::2])      # the summary keeps the dropout runs; every run is asserted


@pytest.mark.parametrize("fp16", [False, True])
@pytest.mark.parametrize("kv_splits", [2, 3])
def test_attn_train_explicit_splits(dev, parity_log, kv_splits, fp16):
    """(1, 70, 300): five key tiles; 2 splits -> 3 + 2 tiles, 3 splits -> 2 + 2 + 1, the last tile ragged
    (44 keys); workspace of exactly cmt_attn_train_workspace_bytes behind a NaN guard"""
    for p in (0.0, 0.25):
        need = _attn_case(dev, parity_log, f"kv_splits={kv_splits} 70x300", B=1, H=3, Nq=70, Nk=300, layout="arena",
                          fp16=fp16, p=p, kv_splits=kv_splits)
        assert need == kv_splits * 1 * 3 * 70 * 34 * 4


@pytest.mark.parametrize("fp16", [False, True])
@pytest.mark.parametrize("Nq,Nk,pad,grp,kv_splits,H", [(200, 200, 128, 16, 2, 3), (700, 1100, 600, 10, 0, 2)])
def test_attn_train_hidden_split(dev, parity_log, Nq, Nk, pad, grp, kv_splits, H, fp16):
    """Queries q >= dn_pad see no key below dn_pad: the first key split (keys 0..127 of 2 explicit
    splits; keys 0..319 of the 4 automatic ones) is wholly hidden from them and reaches the combine
    pass with l == 0, m == -inf and a zero partial output (the forward's m_use keeps exp2(-inf - -inf)
    out of them; the combine pass then gives such a split the weight exp2(-inf) = 0 whether or not it
    tests l > 0).  Nk > dn_pad: no row is fully masked."""
    need = _attn_case(dev, parity_log, f"hidden split {Nq}x{Nk} pad={pad} splits={kv_splits or 'auto'}", B=1, H=H,
                      Nq=Nq, Nk=Nk, layout="dense", pad=pad, grp=grp, fp16=fp16, kv_splits=kv_splits)
    splits = kv_splits or 4
    assert need == splits * H * Nq * 34 * 4        # the automatic choice is the 4 splits described above
