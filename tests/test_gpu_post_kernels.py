"""The kernels around the decoder (csrc/elementwise.hip: pos2embed, the task-head
tail, the camera geometry, the masked view sum, the dtype cast) called through
the C ABI and held to plain torch references written here: float64 on the CPU
for the arithmetic, bit-exact CPU float32 where the operation is exact.  Shapes
are ragged against every kernel's tile (16 queries, 8 outputs, 8 depths, 256
threads) and every output buffer starts NaN-filled."""
import math

import numpy as np
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

PC = [-54.0, -54.0, -5.0, 54.0, 54.0, 3.0]
NAN = float("nan")
# reference points that exercise the clamp and the eps of inverse_sigmoid (parts 2 and 3)
CLAMP_ROWS = [[0.0, 1.0, 0.5], [-0.2, 1.3, 1.0], [1e-6, 1 - 1e-6, 0.0]]


@pytest.fixture(scope="module")
def N():
    from projects.mmdet3d_plugin import native
    native.lib()
    return native


def inverse_sigmoid(x, eps=1e-5):
    """mmdet's inverse_sigmoid (as oracle/cmt_oracle.py), in x's dtype."""
    x = x.clamp(min=0, max=1)
    return torch.log(x.clamp(min=eps) / (1 - x).clamp(min=eps))


# ---------------------------------------------------------------------------
# 1. cmt_pos2embed
# ---------------------------------------------------------------------------
def pos2embed_ref64(xy, F_):
    """[n, 2] (x, y) -> [n, 2F] float64: dim_t = 2 (j // 2) / F + 1, sin on even and cos on odd
    features of 2 pi p / dim_t, the y half first."""
    xy = xy.double()
    j = torch.arange(F_, dtype=torch.float64)
    dim_t = 2 * torch.div(j, 2, rounding_mode="floor") / F_ + 1
    even = (torch.arange(F_) % 2 == 0)

    def half(p):
        a = 2 * math.pi * p[:, None] / dim_t
        return torch.where(even, a.sin(), a.cos())
    return torch.cat([half(xy[:, 1]), half(xy[:, 0])], 1)


def _pos_points(n, stride, seed):
    g = torch.Generator().manual_seed(seed)
    pos = torch.rand(n, stride, generator=g)
    pos[0, :2] = torch.tensor([0.0, 1.0])
    pos[1, :2] = torch.tensor([1.0, 0.0])
    pos[2, :2] = torch.tensor([-0.25, 1.5])
    pos[3, :2] = torch.tensor([1.5, -0.25])
    return pos


@pytest.mark.parametrize("F_", [12, 4, 20])
def test_pos2embed_rejects_f_not_multiple_of_8(N, dev, F_):
    """A thread writes 8 consecutive outputs from ONE half of [y(F) | x(F)]: with F % 8 == 4 the
    group at F - 4 would straddle the halves, so the entry point refuses such an F."""
    pos = torch.rand(5, 2, device=dev)
    out = torch.zeros(5, 2 * F_ + 8, device=dev)
    with pytest.raises(RuntimeError, match="multiple of 8"):
        N.pos2embed(pos, out, n=5, F=F_, ldo=2 * F_ + 8)


@pytest.mark.parametrize("stride", [2, 3])
@pytest.mark.parametrize("mode", [0, 1])
@pytest.mark.parametrize("F_", [8, 24, 128])
def test_pos2embed_f64(N, dev, F_, mode, stride):
    """F = 8: one thread per half; 24: the two_k / F path of a non-power-of-two F; points at 0, 1,
    -0.25 and 1.5 (mode 1 clamps them, then eps 1e-5); padded rows (ldo = 2F + 8) stay untouched."""
    n = 37
    pos = _pos_points(n, stride, seed=F_ + mode)
    ldo = 2 * F_ + 8
    out = torch.full((n, ldo), NAN, device=dev)
    N.pos2embed(pos.to(dev), out, n=n, F=F_, mode=mode, pos_stride=stride, ldo=ldo)
    xy = pos[:, :2].double()
    if mode == 1:
        xy = torch.sigmoid(inverse_sigmoid(xy))
    ref = pos2embed_ref64(xy, F_)
    got = out.cpu()
    err = (got[:, :2 * F_].double() - ref).abs().max().item()
    print(f"pos2embed F={F_} mode={mode} stride={stride}: max abs err {err:.2e} (bound 2e-5)")
    assert err < 2e-5, err
    assert torch.isnan(got[:, 2 * F_:]).all()
    for dt in (torch.bfloat16, torch.float16):
        low = torch.full((n, ldo), NAN, dtype=dt, device=dev)
        N.pos2embed(pos.to(dev), low, n=n, F=F_, mode=mode, pos_stride=stride, ldo=ldo)
        low = low.cpu()
        assert torch.equal(low[:, :2 * F_], got[:, :2 * F_].to(dt))
        assert torch.isnan(low[:, 2 * F_:].float()).all()


@pytest.mark.parametrize("F_", [8, 24])
def test_pos2embed_grid_non_square(N, dev, F_):
    """Grid mode on a 5 x 9 grid against the oracle's coords_bev (whose x / y naming swap puts
    x = (c + 0.5) / 5 with c up to 8, i.e. beyond 1)."""
    from oracle import cmt_oracle as O
    gh, gw = 5, 9
    cb = O.coords_bev([gw * 8, gh * 8, 40], 8)          # x_size = grid_size[1] // 8 = 5, y_size = 9
    assert cb.shape == (gh * gw, 2)
    out = torch.full((gh * gw, 2 * F_), NAN, device=dev)
    N.pos2embed(None, out, n=gh * gw, F=F_, grid=(gh, gw))
    err = (out.cpu().double() - pos2embed_ref64(cb, F_)).abs().max().item()
    assert err < 2e-5, err


# ---------------------------------------------------------------------------
# 2. cmt_task_head_tail
# ---------------------------------------------------------------------------
def task_tail_ref64(H1, gw, gb, W2, B2, ref, *, B, Nq, head_out, k, center_col, height_col, pc_range, hc=64):
    """float64 GroupLayerNorm1d (biased variance, eps 1e-6) + ReLU + grouped conv #2 + box epilogue.
    H1 [L, B*Nq, nheads*hc], gw / gb [L, nheads*hc], W2 [L, out_total, k, hc], B2 [L, out_total],
    ref [B, Nq, 3] -> [L, B, Nq, out_total]."""
    d = torch.float64
    L, nh = H1.shape[0], len(head_out)
    h = H1.to(d).view(L, B, Nq, nh, hc)
    mu = h.mean(-1, keepdim=True)
    var = ((h - mu) ** 2).mean(-1, keepdim=True)
    y = (h - mu) / torch.sqrt(var + 1e-6) * gw.to(d).view(L, 1, 1, nh, hc) + gb.to(d).view(L, 1, 1, nh, hc)
    y = torch.relu(y)
    out = torch.empty(L, B, Nq, sum(head_out), dtype=d)
    o0 = 0
    for hd, n in enumerate(head_out):
        for l in range(L):
            x = y[l, :, :, hd, :].permute(0, 2, 1)                       # [B, hc, Nq]
            w = W2[l, o0:o0 + n].to(d).permute(0, 2, 1)                  # [n, k, hc] -> [n, hc, k]
            out[l, :, :, o0:o0 + n] = F.conv1d(x, w, B2[l, o0:o0 + n].to(d), padding=k // 2).permute(0, 2, 1)
        o0 += n
    inv = inverse_sigmoid(ref.to(d))
    cols = ([(center_col, 0), (center_col + 1, 1)] if center_col >= 0 else []) + \
           ([(height_col, 2)] if height_col >= 0 else [])
    for c, a in cols:
        out[..., c] = torch.sigmoid(out[..., c] + inv[None, :, :, a]) * (pc_range[3 + a] - pc_range[a]) + pc_range[a]
    return out


def _tail_inputs(L, B, Nq, head_out, k, seed):
    g = torch.Generator().manual_seed(seed)
    nh, hc, ot = len(head_out), 64, sum(head_out)
    H1 = torch.randn(L, B * Nq, nh * hc, generator=g) * 2 + 0.5
    gw = 1 + 0.1 * torch.randn(L, nh * hc, generator=g)
    gb = 0.1 * torch.randn(L, nh * hc, generator=g)
    W2 = torch.randn(L, ot, k, hc, generator=g) / math.sqrt(k * hc)
    B2 = torch.randn(L, ot, generator=g)
    ref = torch.rand(B, Nq, 3, generator=g)
    rows = torch.tensor(CLAMP_ROWS)
    nr = min(Nq, len(rows))
    ref[:, Nq - nr:] = rows[:nr]          # the last rows: inside the ragged block when Nq % 16 != 0
    return H1, gw, gb, W2, B2, ref


def _tail_run(N, dev, H1, gw, gb, W2, B2, ref, *, L, B, Nq, head_out, k, center_col, height_col):
    out = torch.full((L, B, Nq, sum(head_out)), NAN, device=dev)
    N.task_head_tail(H1, gw, gb, W2, B2, ref, out, L=L, B=B, Nq=Nq, nheads=len(head_out), hc=64,
                     head_out=head_out, k=k, center_col=center_col, height_col=height_col, pc_range=PC)
    return out.cpu()


def _tail_check(got, want, center_col, height_col):
    assert torch.isfinite(got).all()
    err = (got.double() - want).abs()
    scale = torch.ones(got.shape[-1], dtype=torch.float64)
    if center_col >= 0:
        scale[center_col], scale[center_col + 1] = PC[3] - PC[0], PC[4] - PC[1]
    if height_col >= 0:
        scale[height_col] = PC[5] - PC[2]
    rel = (err / scale).max().item()
    print(f"task_head_tail: max err / column scale {rel:.2e} (bound 1e-4)")
    assert rel < 1e-4, rel


@pytest.mark.parametrize("epilogue", [True, False])
@pytest.mark.parametrize("k", [1, 3])
def test_task_head_tail_f64(N, dev, k, epilogue):
    """Two full 16-query blocks and a block of 5 (its halo rows past Nq are the conv's zero pad), six
    heads, reference points at and beyond 0 / 1; with and without the box epilogue; a per-layer call
    and a second batch element of another magnitude leave the result bit-identical."""
    L, B, Nq, head_out = 2, 2, 37, [2, 1, 3, 2, 2, 3]
    cc, hcol = (0, 2) if epilogue else (-1, -1)
    cpu = _tail_inputs(L, B, Nq, head_out, k, seed=10 + k)
    d = [t.to(dev) for t in cpu]
    keep = d[0].clone()
    kw = dict(B=B, Nq=Nq, head_out=head_out, k=k, center_col=cc, height_col=hcol)
    got = _tail_run(N, dev, *d, L=L, **kw)
    assert torch.equal(d[0], keep)                       # "H1 is only read"
    want = task_tail_ref64(*cpu, pc_range=PC, **kw)
    _tail_check(got, want, cc, hcol)
    # the layer-1 slices alone (the engine's per-layer call)
    H1, gw, gb, W2, B2, ref = d
    one = _tail_run(N, dev, H1[1:2], gw[1:2], gb[1:2], W2[1:2], B2[1:2], ref, L=1, **kw)
    assert torch.equal(one[0], got[1])
    if k == 3:                                           # batch isolation across the halo
        H1b = H1.clone().view(L, B, Nq, -1)
        H1b[:, 1] *= 1e3
        iso = _tail_run(N, dev, H1b.view(L, B * Nq, -1), gw, gb, W2, B2, ref, L=L, **kw)
        assert torch.equal(iso[:, 0], got[:, 0])


@pytest.mark.parametrize("Nq", [1, 16, 17])
@pytest.mark.parametrize("k", [1, 3])
def test_task_head_tail_block_edges(N, dev, k, Nq):
    """Nq = 1: both halo rows outside; 16: exactly one block; 17: a block of one query."""
    L, B, head_out = 1, 1, [5]
    cpu = _tail_inputs(L, B, Nq, head_out, k, seed=100 + 3 * Nq + k)
    kw = dict(B=B, Nq=Nq, head_out=head_out, k=k, center_col=0, height_col=2)
    got = _tail_run(N, dev, *[t.to(dev) for t in cpu], L=L, **kw)
    _tail_check(got, task_tail_ref64(*cpu, pc_range=PC, **kw), 0, 2)


# ---------------------------------------------------------------------------
# 3 / 4. camera geometry: cmt_rv_query_coords(_ex), cmt_rv_pe_coords
# ---------------------------------------------------------------------------
PAD_H, PAD_W = 128.0, 320.0


def _cameras(B, seed):
    """l2i: float32 of the metas' matrices; i2l: float32 of their float64 host inverse; [B, V, 4, 4]"""
    from projects.mmdet3d_plugin import synthetic as S
    metas = S.synthetic_metas(B, yaws=S.NUS_YAWS[:3], pad_shape=(128, 320, 3), seed=seed)
    m64 = np.stack([np.stack([np.asarray(m, dtype=np.float64) for m in meta["lidar2img"]]) for meta in metas])
    return torch.from_numpy(m64).float(), torch.from_numpy(np.linalg.inv(m64)).float(), m64


def rv_query_ref(ref, l2i, i2l, D, dt):
    """_rv_query_embed up to `back` and `mask` (oracle.cmt_oracle.rv_query_embed before the MLP),
    evaluated in dt.  Returns back [B, V, Nq, 3D], mask [B, V, Nq] (bool), the projected pixel
    coordinates [B, V, Nq, 2] and the camera depth z [B, V, Nq]."""
    pcr = torch.tensor(PC, dtype=torch.float32).to(dt)
    r = torch.sigmoid(inverse_sigmoid(ref.to(dt)))
    p = r * (pcr[3:] - pcr[:3]) + pcr[:3]
    ph = torch.cat([p, p.new_ones(*p.shape[:-1], 1)], -1)
    proj = torch.einsum("bnd,bvcd->bvnc", ph, l2i.to(dt))
    z = proj[..., 2:3]
    zpos = z > 0
    den = z + torch.where(zpos, torch.tensor(1e-6, dtype=dt), torch.tensor(-1e-6, dtype=dt))
    pr = proj[..., :3] / den
    mask = (pr[..., 0] < PAD_W) & (pr[..., 0] >= 0) & (pr[..., 1] < PAD_H) & (pr[..., 1] >= 0) & zpos[..., 0]
    depth = 1 + torch.arange(D).to(dt) * (PC[3] - 1) / D
    fr = torch.einsum("bvnc,d->bvndc", pr, depth)
    fr = torch.cat([fr, fr.new_ones(*fr.shape[:-1], 1)], -1)
    back = torch.einsum("bvndo,bvco->bvndc", fr, i2l.to(dt))
    back = (back[..., :3] - pcr[:3]) / (pcr[3:] - pcr[:3])
    return back.reshape(*back.shape[:-2], -1), mask, pr[..., :2], z[..., 0]


# (pixel, expected mask) of the eight edge points: 2 px inside / outside each image edge
EDGE_PIXELS = [((2.0, PAD_H / 2), 1), ((-2.0, PAD_H / 2), 0), ((PAD_W - 2, PAD_H / 2), 1), ((PAD_W + 2, PAD_H / 2), 0),
               ((PAD_W / 2, 2.0), 1), ((PAD_W / 2, -2.0), 0), ((PAD_W / 2, PAD_H - 2), 1), ((PAD_W / 2, PAD_H + 2), 0)]
BEHIND_PIXELS = [(PAD_W / 2, PAD_H / 2), (PAD_W / 4, PAD_H / 4)]


def _back_project(m64, pix, depth):
    """pixel at camera depth `depth` -> normalised reference point (float64)"""
    pt = np.linalg.inv(m64) @ np.array([pix[0] * depth, pix[1] * depth, depth, 1.0])
    lo, hi = np.array(PC[:3]), np.array(PC[3:])
    return (pt[:3] / pt[3] - lo) / (hi - lo)


def _query_case(seed, B=2, V=3, Nq=203):
    """ref [B, Nq, 3] = random points + the clamp rows + constructed points of batch 0:
    returns also the list of (v, q, expected mask) of the constructed points."""
    l2i, i2l, m64 = _cameras(B, seed)
    g = torch.Generator().manual_seed(1000 + seed)
    ref = torch.rand(B, Nq, 3, generator=g)
    ref[:, :3] = torch.tensor(CLAMP_ROWS)
    built, q = [], 3
    for v in range(V):
        # the float32 matrix is what the kernel and the references project with
        m = l2i[0, v].double().numpy()
        for pix, want in EDGE_PIXELS:
            # 10 m deep; the two points at the top edge 8 m: at 10 m they lie 1.58 m above the
            # camera (itself 1.4-1.6 m up), beyond pc_range's z = 3 m, and the clamp would move them
            depth = 8.0 if pix[1] <= 2.0 else 10.0
            built.append((v, q, want, _back_project(m, pix, depth)))
            q += 1
        for pix in BEHIND_PIXELS:
            built.append((v, q, 0, _back_project(m, pix, -10.0)))
            q += 1
    for v, q, want, r in built:
        assert (r > 1e-4).all() and (r < 1 - 1e-4).all(), (v, q, r)   # inside pc_range: neither clamp nor eps moves it
        ref[0, q] = torch.from_numpy(r).float()
    return ref, l2i, i2l, [(v, q, want) for v, q, want, _ in built]


def _nerr(got, ref64):
    return (got.double() - ref64).abs() / (1 + ref64.abs())


@pytest.mark.parametrize("seed", [0, 1, 2])
def test_rv_query_coords_f64(N, dev, seed):
    """Mask: exact against float64 outside a band of 1e-3 of the image size around the four edges
    and |z| < 1e-3 (at most 2 % of the entries; no constructed point in it).  Coordinates: within
    4 x the error of the same expression evaluated in CPU float32 (E32), per class of rows.
    Measured on the MI355X, seeds 0 / 1 / 2: undecided 0.08 / 0.25 / 0.25 %; E32 (kernel error):
    mask 1: 7.4e-7 (7.4e-7), 5.4e-7 (5.4e-7), 6.3e-7 (5.2e-7); |z| >= 0.5: 8.9e-6 (6.2e-6),
    9.3e-6 (5.6e-6), 9.1e-6 (1.05e-5); all rows: 1.2e-4 (1.0e-4), 5.0e-4 (6.6e-4), 2.3e-4 (1.3e-4):
    the largest kernel / E32 ratio is 1.31."""
    B, V, Nq, D = 2, 3, 203, 64
    ref, l2i, i2l, built = _query_case(seed, B, V, Nq)
    b64, m64, px64, z64 = rv_query_ref(ref, l2i, i2l, D, torch.float64)
    b32, m32, _, _ = rv_query_ref(ref, l2i, i2l, D, torch.float32)
    x, y = px64[..., 0], px64[..., 1]
    bx, by = 1e-3 * PAD_W, 1e-3 * PAD_H
    undecided = (x.abs() < bx) | ((x - PAD_W).abs() < bx) | (y.abs() < by) | ((y - PAD_H).abs() < by) | (z64.abs() < 1e-3)
    share = undecided.double().mean().item()
    print(f"rv_query_coords seed {seed}: undecided share {100 * share:.3f} %")
    assert share <= 0.02
    for v, q, want in built:
        assert not undecided[0, v, q]
        assert int(m64[0, v, q]) == want
    assert torch.equal(m32[~undecided], m64[~undecided])          # the CPU float32 evaluation agrees too

    out = torch.full((B * V * Nq, 3 * D), NAN, device=dev)
    mask = torch.full((B * V * Nq,), NAN, device=dev)
    N.rv_query_coords(ref.to(dev), l2i.to(dev), i2l.to(dev), out, mask, B=B, V=V, Nq=Nq, D=D, pad_h=PAD_H,
                      pad_w=PAD_W, pc_range=PC)
    got, gm = out.cpu().view(B, V, Nq, 3 * D), mask.cpu().view(B, V, Nq)
    assert torch.isfinite(got).all()
    assert ((gm == 0) | (gm == 1)).all()
    assert torch.equal(gm[~undecided] == 1, m64[~undecided])
    for v, q, want in built:
        assert gm[0, v, q].item() == want

    classes = {"mask 1": m64, "|z| >= 0.5": z64.abs() >= 0.5, "all": torch.ones_like(m64)}
    e32, ek = _nerr(b32, b64).amax(-1), _nerr(got, b64).amax(-1)
    bad = []
    for name, rows in classes.items():
        E32, EK = e32[rows].max().item(), ek[rows].max().item()
        print(f"rv_query_coords seed {seed} [{name}]: E32 {E32:.3e}  kernel {EK:.3e}  ratio {EK / E32:.2f} (bound 4)")
        if not EK <= 4 * E32:
            bad.append((name, E32, EK))
    assert not bad, bad

    # _ex: rounded coordinates, the same mask
    for dt in (torch.float16, torch.bfloat16):
        low = torch.full((B * V * Nq, 3 * D), NAN, dtype=dt, device=dev)
        lm = torch.full((B * V * Nq,), NAN, device=dev)
        N.rv_query_coords_lowp(ref.to(dev), l2i.to(dev), i2l.to(dev), low, lm, B=B, V=V, Nq=Nq, D=D, pad_h=PAD_H,
                               pad_w=PAD_W, pc_range=PC)
        assert torch.equal(low.cpu(), out.cpu().to(dt))
        assert torch.equal(lm.cpu(), mask.cpu())
    o2 = torch.full((B * V * Nq, 3 * D), NAN, device=dev)
    m2 = torch.full((B * V * Nq,), NAN, device=dev)
    N.rv_query_coords_lowp(ref.to(dev), l2i.to(dev), i2l.to(dev), o2, m2, B=B, V=V, Nq=Nq, D=D, pad_h=PAD_H,
                           pad_w=PAD_W, pc_range=PC)
    assert torch.equal(o2, out) and torch.equal(m2, mask)


def rv_pe_ref(i2l, h, w, D, depth_max, dt):
    """_rv_pe before the MLP (oracle.cmt_oracle.rv_pe), in dt -> [BV * h * w, 3D]"""
    pcr = torch.tensor(PC, dtype=torch.float32).to(dt)
    ch = torch.arange(h).to(dt) * PAD_H / h
    cw = torch.arange(w).to(dt) * PAD_W / w
    cd = 1 + torch.arange(D).to(dt) * (depth_max - 1) / D
    ch, cw, cd = torch.meshgrid([ch, cw, cd], indexing="ij")
    c = torch.stack([cw * cd, ch * cd, cd, torch.ones_like(cd)], -1)
    p = torch.einsum("hwdo,bco->bhwdc", c, i2l.to(dt))[..., :3]
    p = (p - pcr[:3]) / (pcr[3:] - pcr[:3])
    return p.reshape(i2l.shape[0] * h * w, 3 * D)


@pytest.mark.parametrize("D", [64, 12])
def test_rv_pe_coords_f64(N, dev, D):
    """D = 64: the eight-depths-per-thread kernel; D = 12: the one-thread-per-depth kernel (the only
    one a D % 8 != 0 can take).  Bound: 4 x the error of the CPU float32 evaluation (E32).
    Measured on the MI355X: E32 1.94e-7 (D = 64) / 1.89e-7 (D = 12), the kernel's error the same."""
    BV, h, w = 3, 5, 7
    _, i2l, _ = _cameras(1, 0)
    i2l = i2l[0]
    r64 = rv_pe_ref(i2l, h, w, D, PC[3], torch.float64)
    r32 = rv_pe_ref(i2l, h, w, D, PC[3], torch.float32)
    out = torch.full((BV * h * w, 3 * D), NAN, device=dev)
    N.rv_pe_coords(i2l.to(dev), out, BV=BV, h=h, w=w, D=D, pad_h=PAD_H, pad_w=PAD_W, depth_max=PC[3], pc_range=PC)
    got = out.cpu()
    assert torch.isfinite(got).all()
    E32, EK = _nerr(r32, r64).max().item(), _nerr(got, r64).max().item()
    print(f"rv_pe_coords D={D}: E32 {E32:.3e}  kernel {EK:.3e}  ratio {EK / E32:.2f} (bound 4)")
    assert EK <= 4 * E32, (E32, EK)
    if D == 64:
        for dt in (torch.float16, torch.bfloat16):
            low = torch.full((BV * h * w, 3 * D), NAN, dtype=dt, device=dev)
            N.rv_pe_coords(i2l.to(dev), low, BV=BV, h=h, w=w, D=D, pad_h=PAD_H, pad_w=PAD_W, depth_max=PC[3],
                           pc_range=PC)
            assert torch.equal(low.cpu(), got.to(dt))


# ---------------------------------------------------------------------------
# 5. cmt_masked_view_sum(_ex)
# ---------------------------------------------------------------------------
def _view_sum_case(B, V, Nq, C, seed):
    g = torch.Generator().manual_seed(seed)
    X = torch.randn(B, V, Nq, C, generator=g)
    mask = (torch.rand(B, V, Nq, generator=g) < 0.3).float()
    mask[:, :, 5] = 0.0
    mask[:, :, 11] = 1.0
    s = torch.zeros(B, Nq, C)
    for v in range(V):          # the kernel's order; with {0, 1} masks every product is exact
        s = s + X[:, v] * mask[:, v, :, None]
    return X, mask, s, torch.randn(B, Nq, C, generator=g), torch.randn(Nq, C, generator=g)


@pytest.mark.parametrize("C", [256, 64])
def test_masked_view_sum_accumulate(N, dev, C):
    """The plain entry (base == NULL, no low-precision outputs): Y += sum_v X * mask, bit for bit."""
    B, V, Nq = 2, 3, 37
    X, mask, s, Y0, _ = _view_sum_case(B, V, Nq, C, seed=C)
    Y = Y0.clone().to(dev)
    N.masked_view_sum(X.to(dev), mask.to(dev), Y, B=B, V=V, Nq=Nq, C=C)
    assert torch.equal(Y.cpu(), Y0 + s)


@pytest.mark.parametrize("dt", [torch.float16, torch.bfloat16])
def test_masked_view_sum_ex(N, dev, dt):
    B, V, Nq, C = 2, 3, 37, 256
    X, mask, s, Y0, base = _view_sum_case(B, V, Nq, C, seed=7)
    Xd, md, based = X.to(dev), mask.to(dev), base.to(dev)
    want = base[None] + s

    def nan(d):
        return torch.full((B, Nq, C), NAN, dtype=d, device=dev)
    # base + both low-precision outputs
    Y, Yl, Yp = nan(torch.float32), nan(dt), nan(dt)
    N.masked_view_sum(Xd, md, Y, B=B, V=V, Nq=Nq, C=C, base=based, Yl=Yl, Yp=Yp)
    assert torch.equal(Y.cpu(), want)
    assert torch.equal(Yp.cpu(), want.to(dt))
    assert torch.equal(Yl.cpu(), torch.zeros(B, Nq, C, dtype=dt))
    # one of the two alone: the other is still written
    Y, Yp = nan(torch.float32), nan(dt)
    N.masked_view_sum(Xd, md, Y, B=B, V=V, Nq=Nq, C=C, base=based, Yp=Yp)
    assert torch.equal(Y.cpu(), want) and torch.equal(Yp.cpu(), want.to(dt))
    Y, Yl = nan(torch.float32), nan(dt)
    N.masked_view_sum(Xd, md, Y, B=B, V=V, Nq=Nq, C=C, base=based, Yl=Yl)
    assert torch.equal(Y.cpu(), want) and torch.equal(Yl.cpu(), torch.zeros(B, Nq, C, dtype=dt))
    # base alone
    Y = nan(torch.float32)
    N.masked_view_sum(Xd, md, Y, B=B, V=V, Nq=Nq, C=C, base=based)
    assert torch.equal(Y.cpu(), want)
    # accumulate form of _ex
    Y, Yp = Y0.clone().to(dev), nan(dt)
    N.masked_view_sum(Xd, md, Y, B=B, V=V, Nq=Nq, C=C, Yp=Yp)
    assert torch.equal(Y.cpu(), Y0 + s)
    assert torch.equal(Yp.cpu(), (Y0 + s).to(dt))


# ---------------------------------------------------------------------------
# 6. cmt_cast
# ---------------------------------------------------------------------------
def _cast_values():
    g = torch.Generator().manual_seed(6)
    special = [0.0, -0.0, 1.0, -1.0,
               1 + 2.0 ** -11, 1 + 3 * 2.0 ** -11,          # f16 ties: to 1 and to 1 + 2^-9
               1 + 2.0 ** -8, 1 + 3 * 2.0 ** -8,            # bf16 ties: to 1 and to 1 + 2^-6
               65504.0, 65519.0, 65520.0, 1e5,              # f16: max, below / at the tie to inf, inf
               2.0 ** -24, 3 * 2.0 ** -25,                  # f16 subnormals (the second a tie to 2^-23)
               float("inf"), float("-inf"), NAN, 3.4e38]
    return torch.cat([torch.tensor(special, dtype=torch.float32), torch.randn(1000, generator=g)])


def _bits(t):
    return t.view(torch.int32 if t.dtype == torch.float32 else torch.int16)


@pytest.mark.parametrize("n", [1, 255, 256, 257, 1031])
@pytest.mark.parametrize("src,dst", [(torch.float32, torch.float16), (torch.float32, torch.bfloat16),
                                     (torch.float32, torch.float32), (torch.float16, torch.float32),
                                     (torch.bfloat16, torch.float32)])
def test_cast_exact(N, dev, src, dst, n):
    vals = _cast_values()
    X = vals.repeat(-(-n // vals.numel()))[:n].to(src)      # n = 1031 wraps into the special values again
    want = X.to(dst)
    fill = 777.25 if src == dst else NAN                    # a sentinel no input equals
    Y = torch.full((n + 8,), fill, dtype=dst, device=dev)
    N.cast(X.to(dev), Y[:n])
    got = Y.cpu()
    nanm = torch.isnan(want.float())
    assert torch.equal(torch.isnan(got[:n].float()), nanm)
    assert torch.equal(_bits(got[:n])[~nanm], _bits(want)[~nanm])
    tail = got[n:].float()
    assert (tail == fill).all() if src == dst else torch.isnan(tail).all()


def test_cast_rejects_unsupported_pair(N, dev):
    X = torch.zeros(16, dtype=torch.float16, device=dev)
    Y = torch.zeros(16, dtype=torch.bfloat16, device=dev)
    with pytest.raises(RuntimeError, match="unsupported dtype pair"):
        N.cast(X, Y)
