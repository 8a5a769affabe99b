"""cmt_mlp2_affine (csrc/mlp.hip): rv_embedding over the _rv_pe frustum coordinates
(cmt_head.py:417-433, 297-301) with the first layer as an affine map of the pixel per
camera -- no coordinates, no fc1 GEMM -- against

  * a float64 restatement of _rv_pe + rv_embedding + the residual from the fp32 inverse
    camera matrices, the fp32 weights and the pair value of the features: within 2^-19 of
    each output's accumulated magnitude (the bound and the magnitude of test_gpu_mlp.py);
  * the coordinates + fc1 GEMM launch it replaces (cmt_mlp2_x3's fused camera-row form,
    OPTIONS.rv_affine=False) on the same inputs: within 2 x 2^-19 of the same magnitude.

Shapes: the smallest at which each branch can fail (one wave per view and two hidden
blocks; 160 rows per view, so a workgroup holds two views and the last one is partial;
the same rows at the full hidden width, a batch of two with a row offset and a batch
stride into a larger buffer; 5 x 7 pixels per view, which the affine form refuses and the
engine runs in the GEMM form)."""
import numpy as np
import pytest
import torch

from projects.mmdet3d_plugin.runtime import options

pytestmark = pytest.mark.gpu

KEYS = ("center", "height", "dim", "rot", "vel", "cls_logits")
PC = [-54.0, -54.0, -5.0, 54.0, 54.0, 3.0]
D = 64
PAD = (128, 320, 3)
OFF, GAP = 7, 11            # the launch's rows start OFF rows in; batch stride M + GAP rows
FILL = 0x5A5A               # what the buffers hold before a launch


def _pair(x):
    hi = x.half()
    lo = (x - hi.float()).half()
    return torch.stack([hi, lo], dim=-2).contiguous().view(torch.uint16)


def _unpair(p):
    h = p.view(torch.float16)
    return h[..., 0, :].double() + h[..., 1, :].double()


class _Case:
    """Inputs, the float64 reference (computed once) and the launches of one shape."""

    def __init__(self, dev, V, h, w, Hd, batch, seed=0, spike=None):
        from projects.mmdet3d_plugin import native
        from projects.mmdet3d_plugin import synthetic as S
        self.dev, self.V, self.h, self.w, self.Hd, self.batch = dev, V, h, w, Hd, batch
        self.M = V * h * w
        self.rows = batch * (self.M + GAP) + OFF
        g = torch.Generator().manual_seed(seed)
        K = 3 * D
        self.W0 = torch.randn(Hd, K, generator=g) * (1.0 / K ** 0.5)
        self.b0 = torch.randn(Hd, generator=g) * 0.1
        self.W2 = torch.randn(256, Hd, generator=g) * (1.0 / Hd ** 0.5)
        self.b2 = torch.randn(256, generator=g) * 0.1
        self.x = torch.randn(batch * V, 256, h, w, generator=g)
        if spike is not None:
            self.x[0, 3, 0, 1] = spike
        metas = S.synthetic_metas(batch, yaws=S.NUS_YAWS[:V], pad_shape=PAD, seed=seed + 1)
        l2i = np.stack([np.asarray(m["lidar2img"], dtype=np.float64) for m in metas])
        self.i2l = torch.from_numpy(np.linalg.inv(l2i)).float()                   # [batch, V, 4, 4]
        self.packs = native.mlp2_pack(_pair(self.W0).to(dev), _pair(self.W2).to(dev))
        self.tab = native.mlp2_affine_tables(self.W0.to(dev), self.b0.to(dev), D=D, depth_max=PC[3], pc_range=PC)
        self.geo = dict(i2l=self.i2l.to(dev), h=h, w=w, D=D, pad_h=float(PAD[0]), pad_w=float(PAD[1]),
                        depth_max=PC[3], pc_range=PC)
        # the memory rows "(bs v) c h w -> bs (v h w) c" as their f16 pair
        self.mem = _pair(self.x.view(batch, V, 256, h * w).permute(0, 1, 3, 2).reshape(batch, self.M, 256))
        self.flag = torch.zeros(1, dtype=torch.int32, device=dev)

    def slices(self):
        return [slice(OFF + z * (self.M + GAP), OFF + z * (self.M + GAP) + self.M) for z in range(self.batch)]

    def reference(self):
        """(out, accumulated magnitude) [batch, M, 256] in float64."""
        h, w, V = self.h, self.w, self.V
        lo, hi = torch.tensor(PC[:3]).double(), torch.tensor(PC[3:]).double()
        u = (torch.arange(w).float() * PAD[1] / w).double()
        v = (torch.arange(h).float() * PAD[0] / h).double()
        d = (1 + torch.arange(D).float() * (PC[3] - 1) / D).double()
        vv, uu, dd = torch.meshgrid(v, u, d, indexing="ij")
        pix = torch.stack([uu * dd, vv * dd, dd, torch.ones_like(dd)], dim=-1)
        c3 = torch.einsum("hwdo, zbco -> zbhwdc", pix, self.i2l.double())[..., :3]
        cn = ((c3 - lo) / (hi - lo)).reshape(self.batch, self.M, 3 * D)
        hid = torch.relu(cn @ self.W0.double().T + self.b0.double())
        rv = _unpair(self.mem)
        out = hid @ self.W2.double().T + self.b2.double() + rv
        mag = hid.abs() @ self.W2.double().abs().T + self.b2.double().abs() + rv.abs()
        return out, mag

    def _bufs(self):
        mk = lambda: torch.full((self.rows, 2, 256), FILL, dtype=torch.uint16, device=self.dev)
        return mk(), mk()

    def run(self, form):
        """form: 'affine' / 'gemm' (fused camera-row epilogue) or 'affine_rows' (R = memory rows).
        Returns (C, C2) on the host."""
        from projects.mmdet3d_plugin import native
        dev, M = self.dev, self.M
        C, C2 = self._bufs()
        self.flag.zero_()
        kw = dict(batch=self.batch, c_offset=OFF * 256, c_bstride=(M + GAP) * 256)
        b2 = self.b2.to(dev)
        if form == "affine_rows":
            for z, sl in enumerate(self.slices()):
                C2[sl] = self.mem[z].to(dev)
            native.mlp2_affine(self.tab, self.packs[1], b2, C, M=M, Hd=self.Hd, geo=self.geo, R=C2,
                               r_offset=OFF * 256, r_bstride=(M + GAP) * 256, **kw)
        else:
            rx = dict(rx=self.x.to(dev), C2=C2, c2_offset=OFF * 256, c2_bstride=(M + GAP) * 256, range_flag=self.flag)
            if form == "affine":
                native.mlp2_affine(self.tab, self.packs[1], b2, C, M=M, Hd=self.Hd, geo=self.geo, **kw, **rx)
            else:
                native.mlp2(None, self.packs[0], self.b0.to(dev), self.packs[1], b2, C, M=M, K=3 * D, Hd=self.Hd,
                            geo=self.geo, **kw, **rx)
        torch.cuda.synchronize()
        return C.cpu(), C2.cpu()


@pytest.mark.parametrize("V,h,w,Hd,batch", [
    (2, 4, 8, 64, 1),        # one wave per view, two hidden blocks
    (3, 8, 20, 128, 1),      # 160 rows per view: two views in a workgroup, a partial last workgroup
    (3, 8, 20, 1024, 2),     # the full hidden width, two batch elements into a larger buffer
])
def test_affine_matches_float64_and_the_gemm_form(dev, V, h, w, Hd, batch):
    c = _Case(dev, V, h, w, Hd, batch)
    ref, mag = c.reference()
    Ca, C2a = c.run("affine")
    flag_a = int(c.flag.item())
    Cr, _ = c.run("affine_rows")
    Cg, C2g = c.run("gemm")
    got, gemm = _unpair(Ca), _unpair(Cg)
    outside = torch.ones(c.rows, dtype=torch.bool)
    for z, sl in enumerate(c.slices()):
        outside[sl] = False
        e_aff = ((got[sl] - ref[z]).abs() / mag[z]).max().item()
        e_gemm = ((gemm[sl] - ref[z]).abs() / mag[z]).max().item()
        e_two = ((got[sl] - gemm[sl]).abs() / mag[z]).max().item()
        print(f"V{V} {h}x{w} Hd{Hd} z{z}: |err| / magnitude vs float64: affine {e_aff:.3e}, gemm form {e_gemm:.3e}; "
              f"affine vs gemm form {e_two:.3e} (bounds {2 ** -19:.3e}, {2 ** -18:.3e})")
        assert e_aff <= 2 ** -19, (z, e_aff)
        assert e_two <= 2 * 2 ** -19, (z, e_two)
        # the memory rows: the pair split of the NCHW features, bit for bit
        assert torch.equal(C2a[sl], c.mem[z])
        assert torch.equal(C2g[sl], c.mem[z])
        # the R-rows epilogue and the NCHW epilogue: the same values
        assert torch.equal(Cr[sl], Ca[sl])
    # rows outside the launch's ranges are untouched
    assert (Ca[outside] == FILL).all() and (C2a[outside] == FILL).all() and (Cr[outside] == FILL).all()
    assert flag_a == 0


def test_range_flag(dev):
    c = _Case(dev, 2, 4, 8, 64, 1, spike=7e4)
    c.run("affine")
    assert int(c.flag.item()) == 1
    c = _Case(dev, 2, 4, 8, 64, 1)
    c.run("affine")
    assert int(c.flag.item()) == 0


def _small_head(dev, V=6, h=8, w=20, seed=9):
    from projects.mmdet3d_plugin import synthetic as S
    head, cfg, _ = S.build_synthetic_head("cmt_fusion_nus", seed=seed, num_query=96, num_layers=3,
                                          grid_size=[256, 256, 40], device=dev)
    x = S.synthetic_bev(1, 32, 32, seed=61).to(dev)
    xi = S.synthetic_img(V, h, w, seed=62).to(dev)
    metas = S.synthetic_metas(1, yaws=S.NUS_YAWS[:V], pad_shape=PAD, seed=63)
    return head, x, xi, metas


def _forward(head, x, xi, metas, **opts):
    from projects.mmdet3d_plugin import set_precision
    set_precision("ref")
    head.box_epilogue = False
    try:
        with torch.no_grad(), options(**opts):
            o = head([x], [xi], metas)[0][0]
        torch.cuda.synchronize()
        return {k: v.float().clone() for k, v in o.items()}
    finally:
        head.box_epilogue = True


def test_unsupported_view_size_takes_the_gemm_form(dev):
    """5 x 7 pixels per view: the entry point refuses (a wave's rows would span views) and the
    engine runs the coordinates + fc1 GEMM launch, bit for bit what rv_affine=False runs."""
    c = _Case(dev, 1, 5, 7, 64, 1)
    with pytest.raises(RuntimeError, match="1002"):
        c.run("affine")
    head, x, xi, metas = _small_head(dev, V=1, h=5, w=7)
    on = _forward(head, x, xi, metas, rv_affine=True)
    off = _forward(head, x, xi, metas, rv_affine=False)
    for k in KEYS:
        assert torch.isfinite(on[k]).all(), k
        assert torch.equal(on[k], off[k]), k


def test_head_affine_agrees_with_gemm_form(dev):
    """The small fusion head of test_ref_path_selections_agree, and its bound: both forms are
    fp32-accurate; a ~2^-21 difference flips the f16 rounding of a few K / V elements of the
    fp16 flash core, so the logits agree to ~1e-4.  Also with the layout pass and the R rows
    (rv_geo=False), which must stay bit-identical to the one-launch rows."""
    head, x, xi, metas = _small_head(dev)
    on = _forward(head, x, xi, metas, rv_affine=True)
    off = _forward(head, x, xi, metas, rv_affine=False)
    rows = _forward(head, x, xi, metas, rv_affine=True, rv_geo=False)
    for k in KEYS:
        assert torch.isfinite(on[k]).all() and torch.isfinite(off[k]).all(), k
        err = (on[k] - off[k]).abs().max().item()
        print(f"{k}: rv_affine on vs off {err:.3e} (bound 5e-4)")
        assert err <= 5e-4, (k, err)
        assert torch.equal(on[k], rows[k]), k


def test_tables_follow_the_weights(dev):
    """An in-place change of rv_embedding[0].weight rebuilds the tables: the forward after it
    equals a fresh head's with the same state, and differs from the forward before it."""
    head, x, xi, metas = _small_head(dev)
    before = _forward(head, x, xi, metas, rv_affine=True)
    with torch.no_grad():
        head.rv_embedding[0].weight.mul_(1.25)
    after = _forward(head, x, xi, metas, rv_affine=True)
    fresh, _, _, _ = _small_head(dev)
    fresh.load_state_dict(head.state_dict())
    want = _forward(fresh, x, xi, metas, rv_affine=True)
    assert any(not torch.equal(before[k], after[k]) for k in KEYS)
    for k in KEYS:
        assert torch.equal(after[k], want[k]), k
