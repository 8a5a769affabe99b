"""Host side of the image backbone's one-pass fp16 policy (no device): the library's new entries and their
argument checks, the fp16 packs against a float64 fold, the switch (native_img.set_img_precision and the
environment variable CMT_IMG_PRECISION), VoVNet's per-arithmetic pack cache and the wrappers' argument checks."""
import ctypes
import os
import subprocess
import sys

import pytest
import torch

import _vov_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "cmt-cooperative-perception_amd")
F16_ENTRIES = ("cmt_img_stem_f16", "cmt_img_conv3x3_f16", "cmt_img_concat1x1_f16", "cmt_img_ese_apply_f16",
               "cmt_img_maxpool_f16", "cmt_rows_to_nchw_f16")
# the argument structs the entries reuse
F16_STRUCTS = ("img_stem", "img_conv", "img_concat", "img_apply", "img_pool", "rows_to_nchw")


def _NI():
    from projects.mmdet3d_plugin import native_img
    return native_img


# ---- the library -----------------------------------------------------------------------------------------------

def test_library_exports_the_f16_entries():
    from projects.mmdet3d_plugin import native
    L = native.lib()
    assert L.cmt_abi_version() == 25 == native.ABI_VERSION          # additive: the version stays
    raw = ctypes.CDLL(L._name)
    for sym in F16_ENTRIES:
        assert hasattr(raw, sym), sym
    for key in F16_STRUCTS:
        assert getattr(L, f"cmt_{key}_args_size")() == ctypes.sizeof(native.STRUCTS[key]), key


def test_library_refuses_bad_arguments():
    """1001 and a message from the library itself, on a zeroed struct and on a host pointer that is never
    dereferenced: every check comes before any device work"""
    from projects.mmdet3d_plugin import native
    L = native.lib()
    buf = (ctypes.c_char * 80)()
    p = ctypes.c_void_p((ctypes.addressof(buf) + 15) & ~15)
    for cls, fn in zip((native.ImgStemArgs, native.ImgConvArgs, native.ImgConcatArgs, native.ImgApplyArgs,
                        native.ImgPoolArgs, native.RowsToNchwArgs), F16_ENTRIES):
        assert getattr(L, fn)(None, None) == 1001 and b"null argument struct" in L.cmt_last_error(), fn
        assert getattr(L, fn)(ctypes.byref(cls()), None) == 1001, fn
        assert b"non-null" in L.cmt_last_error() and fn.encode() in L.cmt_last_error(), fn
    c = native.ImgConvArgs()
    c.X, c.Wt, c.shift, c.Y = p, p, p, p
    c.B, c.H, c.W, c.Cin, c.Cout, c.stride, c.ldx, c.ldw, c.ldy = 1, 2, 2, 32, 288, 1, 32, 288, 288
    assert L.cmt_img_conv3x3_f16(ctypes.byref(c), None) == 1001 and b"at most 256" in L.cmt_last_error()
    c.Cout, c.Cin = 160, 48
    assert L.cmt_img_conv3x3_f16(ctypes.byref(c), None) == 1001 and b"Cin must be" in L.cmt_last_error()
    c.Cin, c.stride = 32, 3
    assert L.cmt_img_conv3x3_f16(ctypes.byref(c), None) == 1001 and b"stride" in L.cmt_last_error()
    c.stride, c.nb = 1, 2                                     # 160 / 32 = 5 column blocks
    assert L.cmt_img_conv3x3_f16(ctypes.byref(c), None) == 1001 and b"divisor" in L.cmt_last_error()
    c.nb = 0
    for field, bad in (("ldx", 24), ("ldx", 36), ("ldw", 280), ("ldw", 292), ("ldy", 152), ("ldy", 164)):
        good = getattr(c, field)
        setattr(c, field, bad)                                # below the row, or no multiple of 8
        assert L.cmt_img_conv3x3_f16(ctypes.byref(c), None) == 1001 and b"ldx >= Cin" in L.cmt_last_error(), (field, bad)
        setattr(c, field, good)
    c.X = ctypes.c_void_p(p.value + 2)
    assert L.cmt_img_conv3x3_f16(ctypes.byref(c), None) == 1001 and b"16-byte aligned" in L.cmt_last_error()
    s = native.ImgStemArgs()
    s.X, s.Wt, s.shift, s.Y = p, p, p, p
    s.B, s.H, s.W, s.Cin, s.Cout, s.x_bstride, s.ldy = 1, 2, 2, 4, 64, 16, 64
    assert L.cmt_img_stem_f16(ctypes.byref(s), None) == 1001 and b"1, 2 or 3" in L.cmt_last_error()
    s.Cin, s.x_bstride = 3, 11
    assert L.cmt_img_stem_f16(ctypes.byref(s), None) == 1001 and b"x_bstride" in L.cmt_last_error()
    s.x_bstride, s.ldy = 12, 56
    assert L.cmt_img_stem_f16(ctypes.byref(s), None) == 1001 and b"ldy >= Cout" in L.cmt_last_error()
    k = native.ImgConcatArgs()
    k.Wt, k.shift, k.Y, k.B, k.HW, k.Cout, k.nsrc = p, p, p, 1, 4, 128, 9
    assert L.cmt_img_concat1x1_f16(ctypes.byref(k), None) == 1001 and b"1 to 8 sources" in L.cmt_last_error()
    k.nsrc, k.C[0], k.X[0], k.ldx[0] = 1, 48, p.value, 48
    assert L.cmt_img_concat1x1_f16(ctypes.byref(k), None) == 1001 and b"multiple of 32" in L.cmt_last_error()
    k.C[0], k.ldx[0] = 32, 24
    assert L.cmt_img_concat1x1_f16(ctypes.byref(k), None) == 1001 and b"ldx >= C" in L.cmt_last_error()
    k.ldx[0], k.ldw, k.ldy, k.Cout = 32, 32, 128, 64
    assert L.cmt_img_concat1x1_f16(ctypes.byref(k), None) == 1001 and b"multiple of 128" in L.cmt_last_error()
    k.Cout, k.ldw = 128, 24
    assert L.cmt_img_concat1x1_f16(ctypes.byref(k), None) == 1001 and b"ldw >= K" in L.cmt_last_error()
    a = native.ImgApplyArgs()
    a.X, a.gate, a.Y, a.B, a.HW, a.C, a.ldx, a.ldy = p, p, p, 1, 4, 36, 40, 40
    assert L.cmt_img_ese_apply_f16(ctypes.byref(a), None) == 1001 and b"multiple of 8" in L.cmt_last_error()
    a.C, a.ldx = 32, 24
    assert L.cmt_img_ese_apply_f16(ctypes.byref(a), None) == 1001 and b"ldx, ldy >= C" in L.cmt_last_error()
    a.ldx, a.R, a.ldr = 32, p, 16
    assert L.cmt_img_ese_apply_f16(ctypes.byref(a), None) == 1001 and b"ldr >= C" in L.cmt_last_error()
    q = native.ImgPoolArgs()
    q.X, q.Y, q.B, q.H, q.W, q.C, q.ldx, q.ldy = p, p, 1, 1, 5, 128, 128, 128
    assert L.cmt_img_maxpool_f16(ctypes.byref(q), None) == 1001 and b"H, W >= 2" in L.cmt_last_error()
    q.H, q.ldy = 2, 120
    assert L.cmt_img_maxpool_f16(ctypes.byref(q), None) == 1001 and b"ldx, ldy >= C" in L.cmt_last_error()
    t = native.RowsToNchwArgs()
    t.X, t.Y, t.B, t.C, t.HW, t.ldx = p, p, 1, 36, 4, 40
    assert L.cmt_rows_to_nchw_f16(ctypes.byref(t), None) == 1001 and b"multiple of 8" in L.cmt_last_error()
    t.C, t.ldx = 32, 24
    assert L.cmt_rows_to_nchw_f16(ctypes.byref(t), None) == 1001 and b"ldx >= C" in L.cmt_last_error()


# ---- the packs -------------------------------------------------------------------------------------------------

def _fold64(w, bn, eps):
    """the float64 fold, restated: (W * scale per output channel, shift)"""
    g, b, mean, var = (t.double() for t in bn)
    scale = g / torch.sqrt(var + eps)
    return w.double() * scale[:, None, None, None], b - mean * scale


def _same_bits(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and torch.equal(a.view(torch.int16), b.view(torch.int16))


@pytest.mark.parametrize("cin", [1, 3])
def test_pack_stem_f16(cin):
    NI = _NI()
    g = torch.Generator().manual_seed(170 + cin)
    w = torch.randn(64, cin, 3, 3, generator=g) / (9 * cin) ** 0.5
    bn = R.random_bn(64, g)
    w16, shift = NI.pack_stem_f16(w, list(bn) + [R.BN_EPS])
    w64, s64 = _fold64(w, bn, R.BN_EPS)
    assert w16.dtype == torch.float16 and tuple(w16.shape) == (64, NI.STEM_K) and w16.is_contiguous()
    assert _same_bits(w16[:, :9 * cin].contiguous(), w64.permute(0, 2, 3, 1).reshape(64, -1).to(torch.float16))
    assert not w16[:, 9 * cin:].any(), "the K padding columns must be zero"
    assert shift.dtype == torch.float32 and torch.equal(shift, s64.float())
    with pytest.raises(ValueError, match="Cin <= 3"):
        NI.pack_stem_f16(torch.zeros(64, 4, 3, 3), list(bn) + [R.BN_EPS])


def test_pack_conv3x3_f16_and_concat_f16():
    NI = _NI()
    g = torch.Generator().manual_seed(173)
    w = torch.randn(96, 32, 3, 3, generator=g) / 288 ** 0.5
    bn = R.random_bn(96, g)
    w16, shift = NI.pack_conv3x3_f16(w, list(bn) + [R.BN_EPS])
    w64, s64 = _fold64(w, bn, R.BN_EPS)
    assert tuple(w16.shape) == (96, 288) and w16.is_contiguous()
    # tap-major: k = (ky*3 + kx) * Cin + c
    assert _same_bits(w16, w64.permute(0, 2, 3, 1).reshape(96, 288).to(torch.float16))
    assert w16[5, (1 * 3 + 2) * 32 + 7].item() == w64[5, 7, 1, 2].to(torch.float16).item()
    assert torch.equal(shift, s64.float())
    # the rounding is the one RNE rounding of the float64 value: within half an fp16 ulp, ties included
    err = (w16.double() - w64.permute(0, 2, 3, 1).reshape(96, 288)).abs()
    assert (err <= 2.0 ** -11 * w64.abs().max()).all() and err.max() > 0
    k = torch.randn(128, 160, 1, 1, generator=g) / 160 ** 0.5
    bnk = R.random_bn(128, g)
    k16, kshift = NI.pack_concat_f16(k, list(bnk) + [R.BN_EPS])
    k64, ks64 = _fold64(k, bnk, R.BN_EPS)
    assert _same_bits(k16, k64.reshape(128, 160).to(torch.float16)) and torch.equal(kshift, ks64.float())
    with pytest.raises(ValueError, match="running_var"):
        NI.pack_concat_f16(k, None)
    with pytest.raises(ValueError, match="3, 3"):
        NI.pack_conv3x3_f16(k, list(bnk) + [R.BN_EPS])


def test_packs_refuse_what_fp16_cannot_hold():
    NI = _NI()
    one = [torch.ones(32), torch.zeros(32), torch.zeros(32), torch.ones(32), 0.0]
    w = torch.zeros(32, 32, 3, 3)
    w[3, 4, 1, 1] = 65504.0
    w16, _ = NI.pack_conv3x3_f16(w, one)                      # the largest finite value is held
    assert w16[3, 4 * 32 + 4].item() == 65504.0
    w[3, 4, 1, 1] = 65505.0
    with pytest.raises(ValueError, match="65504"):
        NI.pack_conv3x3_f16(w, one)
    w[3, 4, 1, 1] = 1000.0
    big = [torch.full((32,), 100.0)] + one[1:]                # a fold that overflows: 1000 * 100
    with pytest.raises(ValueError, match="65504"):
        NI.pack_conv3x3_f16(w, big)
    with pytest.raises(ValueError, match="65504"):
        NI.pack_concat_f16(torch.full((128, 32, 1, 1), -7e4), [torch.ones(128), torch.zeros(128), torch.zeros(128),
                                                              torch.ones(128), 0.0])
    with pytest.raises(ValueError, match="65504"):
        NI.pack_stem_f16(torch.full((32, 3, 3, 3), 7e4), one)
    w[3, 4, 1, 1] = float("nan")
    with pytest.raises(ValueError, match="non-finite"):
        NI.pack_conv3x3_f16(w, one)
    w[3, 4, 1, 1] = 1.0
    var0 = one[:3] + [torch.zeros(32), 0.0]                   # 1 / sqrt(0): an infinite scale
    with pytest.raises(ValueError, match="non-finite"):
        NI.pack_conv3x3_f16(w, var0)


# ---- the switch ------------------------------------------------------------------------------------------------

def test_setter_validates_and_defaults_to_ref():
    NI = _NI()
    if not os.environ.get("CMT_IMG_PRECISION"):
        assert NI.img_precision() == "ref"
    old = NI.set_img_precision("fp16")
    try:
        assert NI.img_precision() == "fp16" and NI.set_img_precision("ref") == "fp16" and NI.img_precision() == "ref"
        for bad in ("bf16", "FP16", "", None, 16):
            with pytest.raises(ValueError, match="ref"):
                NI.set_img_precision(bad)
            assert NI.img_precision() == "ref"                # a refused value changes nothing
    finally:
        NI.set_img_precision(old)


def _child(env_value, code):
    env = {k: v for k, v in os.environ.items() if k != "CMT_IMG_PRECISION"}
    if env_value is not None:
        env["CMT_IMG_PRECISION"] = env_value
    env["PYTHONPATH"] = os.pathsep.join([PKG, ROOT] + ([env["PYTHONPATH"]] if env.get("PYTHONPATH") else []))
    return subprocess.run([sys.executable, "-c", code], env=env, capture_output=True, text=True, timeout=300)


def test_environment_variable_is_read_at_import():
    code = ("from projects.mmdet3d_plugin import native_img as NI, runtime\n"
            "print(NI.img_precision(), runtime.get_precision().name)")
    got = _child("fp16", code)
    assert got.returncode == 0, got.stderr
    first = got.stdout.split()
    got = _child(None, code)
    assert got.returncode == 0, got.stderr
    # the image setting is its own: the head's policy is what it is without the variable
    assert first[0] == "fp16" and got.stdout.split() == ["ref", first[1]]
    got = _child("half", code)
    assert got.returncode != 0 and "CMT_IMG_PRECISION" in got.stderr and "ValueError" in got.stderr


# ---- the module's packs ----------------------------------------------------------------------------------------

def test_module_keeps_packs_per_arithmetic():
    from projects.mmdet3d_plugin import build_backbone
    m = R.seed_by_key(build_backbone(dict(type="VoVNet", spec_name="V-19-eSE", out_features=("stage4", "stage5"))), 7)
    blk = m.stage3.OSA3_1
    p_ref, p16 = m.packed_layer("OSA3_1", blk, 1), m.packed_layer("OSA3_1", blk, 1, fp16=True)
    assert p_ref[0].dtype == torch.uint16 and tuple(p_ref[0].shape) == (160, 2, 9 * 160)
    assert p16[0].dtype == torch.float16 and tuple(p16[0].shape) == (160, 9 * 160)
    # the two do not evict each other
    assert m.packed_layer("OSA3_1", blk, 1)[0] is p_ref[0] and m.packed_layer("OSA3_1", blk, 1, fp16=True)[0] is p16[0]
    s16, c16 = m.packed_stem(0, fp16=True), m.packed_layer("OSA3_1", blk, "concat", fp16=True)
    assert tuple(s16[0].shape) == (64, 32) and tuple(m.packed_stem(2, fp16=True)[0].shape) == (128, 9 * 64)
    assert tuple(c16[0].shape) == (512, 256 + 3 * 160) and m.packed_stem(0)[0].dtype == torch.uint16
    # the fp16 weight is the float64 fold rounded once: the pair's hi half rounds the same value
    assert _same_bits(p16[0], p_ref[0].view(torch.float16)[:, 0].contiguous())
    with torch.no_grad():
        blk.layers[1][0].weight.mul_(1.5)
        m.stem[1].running_mean.add_(0.25)
    n_ref, n16 = m.packed_layer("OSA3_1", blk, 1), m.packed_layer("OSA3_1", blk, 1, fp16=True)
    assert not _same_bits(n16[0], p16[0]) and not torch.equal(n_ref[0].view(torch.int16), p_ref[0].view(torch.int16))
    assert _same_bits(n16[0], n_ref[0].view(torch.float16)[:, 0].contiguous())
    t16 = m.packed_stem(0, fp16=True)
    assert _same_bits(t16[0], s16[0]) and not torch.equal(t16[1], s16[1])      # the mean moves the shift only


# ---- the wrappers ----------------------------------------------------------------------------------------------

def _rows(n, c):
    return torch.zeros((n, c), dtype=torch.float16)


def test_wrappers_check_before_the_device():
    """every ValueError comes before the device check: all tensors here live on the CPU, and a call whose
    arguments are fine ends in the no-fallback RuntimeError instead"""
    NI = _NI()
    from projects.mmdet3d_plugin import native_fpn as NF
    sh = lambda c: torch.zeros(c)   # noqa: E731
    V = pytest.raises(ValueError)
    with V:
        NI.stem_f16(torch.zeros(1, 4, 8, 8), _rows(64, 32), sh(64), Cout=64)
    with V:
        NI.stem_f16(torch.zeros(1, 3, 8, 8), _rows(48, 32), sh(48), Cout=48)
    with V:
        NI.stem_f16(torch.zeros(1, 3, 8, 8).double(), _rows(64, 32), sh(64), Cout=64)
    with V:
        NI.stem_f16(torch.zeros(1, 3, 8, 8)[:, :, :, ::2], _rows(64, 32), sh(64), Cout=64)
    with V:
        NI.stem_f16(torch.zeros(1, 3, 8, 8), _rows(64, 27), sh(64), Cout=64)
    with V:
        NI.stem_f16(torch.zeros(1, 3, 8, 8), torch.zeros((64, 2, 32), dtype=torch.uint16), sh(64), Cout=64)   # pair rows
    ok = dict(B=1, H=4, W=4, Cin=32, Cout=64, stride=1)
    with V:
        NI.conv3x3_f16(_rows(16, 48), _rows(64, 9 * 48), sh(64), **dict(ok, Cin=48))
    with V:
        NI.conv3x3_f16(_rows(16, 32), _rows(80, 9 * 32), sh(80), **dict(ok, Cout=80))
    with V:
        NI.conv3x3_f16(_rows(16, 32), _rows(288, 9 * 32), sh(288), **dict(ok, Cout=288))
    with V:
        NI.conv3x3_f16(_rows(16, 32), _rows(64, 9 * 32), sh(64), **dict(ok, stride=3))
    with V:
        NI.conv3x3_f16(_rows(16, 32), _rows(96, 9 * 32), sh(96), nb=2, **dict(ok, Cout=96))
    with V:
        NI.conv3x3_f16(_rows(15, 32), _rows(64, 9 * 32), sh(64), **ok)          # short X
    with V:
        NI.conv3x3_f16(_rows(16, 32), _rows(64, 9 * 32), sh(64), out=_rows(15, 64), **ok)   # short out
    with V:
        NI.conv3x3_f16(_rows(16, 32).view(torch.int16), _rows(64, 9 * 32), sh(64), **ok)    # wrong dtype
    with V:
        NI.conv3x3_f16(_rows(16, 36)[:, :32], _rows(64, 9 * 32), sh(64), **ok)              # ld 36: no multiple of 8
    with V:
        NI.conv3x3_f16(_rows(16, 32), _rows(64, 9 * 32), sh(64), range_flag=torch.zeros(1), **ok)
    with V:
        NI.concat1x1_f16([_rows(4, 32)] * 9, _rows(128, 288), sh(128), B=1, HW=4, Cout=128)
    with V:
        NI.concat1x1_f16([], _rows(128, 32), sh(128), B=1, HW=4, Cout=128)
    with V:
        NI.concat1x1_f16([_rows(4, 48)], _rows(128, 48), sh(128), B=1, HW=4, Cout=128)
    with V:
        NI.concat1x1_f16([_rows(4, 32)], _rows(64, 32), sh(64), B=1, HW=4, Cout=64)
    with V:
        NI.concat1x1_f16([_rows(3, 32)], _rows(128, 32), sh(128), B=1, HW=4, Cout=128)
    with V:
        NI.concat1x1_f16([_rows(4, 32), _rows(4, 32)], _rows(128, 32), sh(128), B=1, HW=4, Cout=128)   # K of W
    with V:
        NI.concat1x1_f16([torch.zeros((4, 2, 32), dtype=torch.uint16)], _rows(128, 32), sh(128), B=1, HW=4, Cout=128)
    with V:
        NI.concat1x1_f16([_rows(4, 32)], _rows(128, 32), sh(128), B=1, HW=4, Cout=128, part=torch.zeros(1, 2, 128))
    with V:
        NI.ese_apply_f16(_rows(4, 36), torch.zeros(1, 36), B=1, HW=4, C=36)
    with V:
        NI.ese_apply_f16(_rows(4, 32), torch.zeros(2, 32), B=1, HW=4, C=32)
    with V:
        NI.ese_apply_f16(_rows(4, 32), torch.zeros(1, 32), B=1, HW=4, C=32, identity=_rows(3, 32))
    with V:
        NI.maxpool_f16(_rows(5, 128), B=1, H=1, W=5, C=128)
    with V:
        NI.maxpool_f16(_rows(9, 36), B=1, H=3, W=3, C=36)
    with V:
        NI.maxpool_f16(_rows(8, 128), B=1, H=3, W=3, C=128)
    with V:
        NI.maxpool_f16(_rows(9, 128).float(), B=1, H=3, W=3, C=128)
    with V:
        NF.rows_to_nchw_f16(_rows(9, 36), (1, 36, 3, 3))
    with V:
        NF.rows_to_nchw_f16(_rows(8, 32), (1, 32, 3, 3))
    with V:
        NF.rows_to_nchw_f16(_rows(9, 32), (1, 32, 3, 3), out=torch.zeros(1, 32, 3, 3).double())
    with V:
        NF.rows_to_nchw_f16(torch.zeros((9, 2, 32), dtype=torch.uint16), (1, 32, 3, 3))
    D = pytest.raises(RuntimeError, match="HIP device")
    wide = torch.zeros((4, 48), dtype=torch.float16)[:, 8:40]       # a column slice: ld 48 > C
    with D:
        NI.stem_f16(torch.zeros(1, 3, 8, 8), _rows(64, 32), sh(64), Cout=64)
    with D:
        NI.stem_f16(torch.zeros(3, 3, 8, 8)[::2], _rows(64, 32), sh(64), Cout=64)    # a batch stride of two images
    with D:
        NI.conv3x3_f16(_rows(16, 32), _rows(64, 9 * 32), sh(64), **ok)
    with D:
        NI.conv3x3_f16(_rows(16, 40)[:, :32], _rows(64, 9 * 32), sh(64), out=_rows(16, 72)[:, :64], **ok)
    with D:
        NI.concat1x1_f16([_rows(4, 32), wide], _rows(128, 64), sh(128), B=1, HW=4, Cout=128, part=True)
    with D:
        NI.ese_apply_f16(_rows(4, 32), torch.zeros(1, 32), B=1, HW=4, C=32, identity=_rows(4, 32))
    with D:
        NI.maxpool_f16(_rows(9, 128), B=1, H=3, W=3, C=128)
    with D:
        NF.rows_to_nchw_f16(_rows(9, 32), (1, 32, 3, 3))
