"""cmt_mlp2_affine (csrc/mlp.hip) without a device: the weight-only tables of
native.mlp2_affine_tables against a float64 restatement of _rv_pe + rv_embedding[0]
(cmt_head.py:417-433, 297-301), and the entry point's argument checks, which run
before any HIP call."""
import ctypes

import numpy as np
import torch

PC = [-54.0, -54.0, -5.0, 54.0, 54.0, 3.0]
D = 64


def _cams(V, seed):
    from projects.mmdet3d_plugin import synthetic as S
    metas = S.synthetic_metas(1, yaws=S.NUS_YAWS[:V], pad_shape=(128, 320, 3), seed=seed)
    l2i = np.stack([np.asarray(m["lidar2img"], dtype=np.float64) for m in metas])
    return torch.from_numpy(np.linalg.inv(l2i)).float()[0]          # [V, 4, 4] fp32, as uploaded


def test_tables_restate_the_first_layer():
    """alpha u + beta v + gamma from the tables equals W0 . coords_n + b0 evaluated directly,
    both in float64 (rounding only: ~1e-13 of the accumulated magnitude)."""
    from projects.mmdet3d_plugin import native
    g = torch.Generator().manual_seed(3)
    Hd, h, w, V = 96, 8, 20, 3
    W0 = torch.randn(Hd, 3 * D, generator=g) / (3 * D) ** 0.5
    b0 = torch.randn(Hd, generator=g) * 0.1
    tab = native.mlp2_affine_tables(W0, b0, D=D, depth_max=PC[3], pc_range=PC)
    assert tab.dtype == torch.float64 and tab.shape == (Hd, 8) and (tab[:, 7] == 0).all()
    i2l = _cams(V, 5).double()
    lo, hi = torch.tensor(PC[:3]).double(), torch.tensor(PC[3:]).double()
    u = (torch.arange(w).float() * 320 / w).double()
    v = (torch.arange(h).float() * 128 / h).double()
    d = (1 + torch.arange(D).float() * (PC[3] - 1) / D).double()
    vv, uu, dd = torch.meshgrid(v, u, d, indexing="ij")
    pix = torch.stack([uu * dd, vv * dd, dd, torch.ones_like(dd)], dim=-1)          # [h, w, D, 4]
    c3 = torch.einsum("hwdo, bco -> bhwdc", pix, i2l)[..., :3]
    cn = ((c3 - lo) / (hi - lo)).reshape(V, h, w, 3 * D)
    pre = cn @ W0.double().T + b0.double()
    mag = cn.abs() @ W0.double().abs().T + b0.double().abs()
    T1, T0, bb = tab[:, 0:3], tab[:, 3:6], tab[:, 6]
    al = torch.einsum("jc, bc -> bj", T1, i2l[:, :3, 0])
    be = torch.einsum("jc, bc -> bj", T1, i2l[:, :3, 1])
    ga = torch.einsum("jc, bc -> bj", T1, i2l[:, :3, 2]) + torch.einsum("jc, bc -> bj", T0, i2l[:, :3, 3] - lo) + bb
    aff = (al[:, None, None, :] * u[None, None, :, None] + be[:, None, None, :] * v[None, :, None, None]
           + ga[:, None, None, :])
    assert ((aff - pre).abs() / mag).max().item() <= 1e-12


def _args(native, **kw):
    fake = 0x1000                       # never dereferenced: every case returns before the launch
    ga = native.Mlp2AffineArgs()
    m = ga.m
    m.M, m.Hd, m.N, m.batch = 64, 64, 256, 1
    m.geo_i2l, m.W2p, m.b2, m.C = fake, fake, fake, fake
    m.geo_h, m.geo_w = 4, 8
    m.ldc, m.c_dtype = 512, native.F16P
    ga.tab = fake
    for k, v in kw.items():
        if k == "tab":
            ga.tab = v
        else:
            setattr(m, k, v)
    return ga


def test_argument_checks_without_device():
    from projects.mmdet3d_plugin import native
    L = native.lib()
    assert L.cmt_mlp2_affine_args_size() == ctypes.sizeof(native.Mlp2AffineArgs)
    assert L.cmt_mlp2_affine(None, None) == 1001
    ga = _args(native, tab=None)                                     # null tables
    assert L.cmt_mlp2_affine(ctypes.byref(ga), None) == 1001 and b"null pointer" in L.cmt_last_error()
    ga = _args(native, Hd=48)                                        # Hd not a multiple of 32
    assert L.cmt_mlp2_affine(ctypes.byref(ga), None) == 1001 and b"multiple of 32" in L.cmt_last_error()
    ga = _args(native, M=70, geo_h=5, geo_w=7)                       # h w % 32 != 0: unsupported
    assert L.cmt_mlp2_affine(ctypes.byref(ga), None) == 1002 and b"one view" in L.cmt_last_error()
    ga = _args(native, Hd=2048)                                      # beyond the LDS tables
    assert L.cmt_mlp2_affine(ctypes.byref(ga), None) == 1002
    ga = _args(native, M=60)                                         # not whole views
    assert L.cmt_mlp2_affine(ctypes.byref(ga), None) == 1001
    ga = _args(native, rx=0x1000)                                    # rx without C2
    assert L.cmt_mlp2_affine(ctypes.byref(ga), None) == 1001
