"""Host side of the native VoVNet (no device): the registry, the state_dict layout against the reference's
own keys (tests/golden/vovnet_keys.json), the unsupported-input errors, the float64 oracle
(tests/_vov_ref.py) against the reference's own output (tests/golden/vovnet_v39_ref.npz), the pool size
rule, the stem and aggregation packing through a float64 GEMM, the library's new symbols and structs, and
the wrappers' argument checks."""
import ctypes
import json
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import _vov_ref as R
from test_fpn_host import IMG_NAMES, REF_CONFIGS

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
CFG = dict(type="VoVNet", spec_name="V-99-eSE", norm_eval=True, frozen_stages=-1, input_ch=3,
           out_features=("stage4", "stage5"))
SPECS = ("V-19-eSE", "V-39-eSE", "V-57-eSE", "V-99-eSE")
ENTRIES = {"V-19-eSE": 122, "V-39-eSE": 246, "V-99-eSE": 626}


def _build(**change):
    from projects.mmdet3d_plugin import build_backbone
    return build_backbone(dict(CFG, **change))


def _keys():
    with open(os.path.join(GOLDEN, "vovnet_keys.json")) as f:
        return json.load(f)


# ---- registry, state dict, errors ----------------------------------------------------------------------------

def test_registered_and_exported():
    import projects.mmdet3d_plugin as plugin
    from projects.mmdet3d_plugin.models import backbones
    from projects.mmdet3d_plugin.registry import BACKBONES
    assert BACKBONES.get("VoVNet") is backbones.VoVNet and "VoVNet" in backbones.__all__
    m = plugin.build_backbone(CFG)
    assert type(m).__name__ == "VoVNet" and m.spec_name == "V-99-eSE"
    assert (m.frozen_stages, m.norm_eval, m.pretrained, m.init_cfg) == (-1, True, None, None)
    assert m.init_weights() is None
    assert m._out_feature_channels == dict(stem=128, stage2=256, stage3=512, stage4=768, stage5=1024)
    assert m._out_feature_strides == dict(stem=4, stage2=4, stage3=8, stage4=16, stage5=32)


@pytest.mark.parametrize("name", IMG_NAMES)
def test_reference_img_backbone_builds(name):
    if not os.path.isdir(REF_CONFIGS):
        pytest.skip("reference checkout not present")
    from projects.mmdet3d_plugin import build_backbone
    from projects.mmdet3d_plugin.config import load_config
    model = load_config(os.path.join(REF_CONFIGS, name))["model"]
    parts = [m for m in (model, model.get("vehicle_model"), model.get("infrastructure_model"))
             if isinstance(m, dict) and "img_backbone" in m]
    assert parts
    for part in parts:
        cfg = part["img_backbone"]
        if cfg["type"] != "VoVNet":
            assert "r50" in name and cfg["type"] == "ResNet"   # the one ResNet-50 config: not part of this package
            continue
        m = build_backbone(cfg)
        assert type(m).__name__ == "VoVNet" and m._out_features == ("stage4", "stage5")
        assert len(m.state_dict()) == ENTRIES[cfg["spec_name"]]


@pytest.mark.parametrize("spec", SPECS)
def test_state_dict_is_the_references(spec):
    m = _build(spec_name=spec)
    sd = m.state_dict()
    assert [[k, list(v.shape)] for k, v in sd.items()] == _keys()[spec]
    if spec in ENTRIES:
        assert len(sd) == ENTRIES[spec]
    if spec == "V-99-eSE":
        assert sum(v.numel() for v in sd.values()) == 69_577_763
        for k, shape in (("stem.stem_1/conv.weight", (64, 3, 3, 3)), ("stem.stem_1/norm.num_batches_tracked", ()),
                         ("stage3.OSA3_2.layers.4.OSA3_2_4/conv.weight", (160, 160, 3, 3)),
                         ("stage2.OSA2_1.concat.OSA2_1_concat/conv.weight", (256, 768, 1, 1)),
                         ("stage5.OSA5_3.ese.fc.weight", (1024, 1024, 1, 1)), ("stage5.OSA5_3.ese.fc.bias", (1024,))):
            assert tuple(sd[k].shape) == shape, k
    assert not any("Pooling" in k for k in sd)
    # strict round trip through a differently seeded copy
    other = R.seed_by_key(_build(spec_name=spec), 5)
    assert other.load_state_dict(R.seed_by_key(m, 6).state_dict(), strict=True).missing_keys == []
    assert all(torch.equal(a, b) for a, b in zip(other.state_dict().values(), m.state_dict().values()))


def test_seeding_is_by_key():
    a, b = R.seed_by_key(_build(spec_name="V-19-eSE"), 3), R.seed_by_key(_build(spec_name="V-39-eSE"), 3)
    k = "stage2.OSA2_1.layers.1.OSA2_1_1/conv.weight"
    assert torch.equal(a.state_dict()[k], b.state_dict()[k])
    assert not torch.equal(a.state_dict()[k], R.seed_by_key(_build(spec_name="V-19-eSE"), 4).state_dict()[k])


def test_unbuilt_forms_raise():
    for spec, word in (("V-19-slim-dw-eSE", "depthwise"), ("V-19-dw-eSE", "depthwise"), ("V-19-slim-eSE", "multiple of 32")):
        with pytest.raises(NotImplementedError, match=word):
            _build(spec_name=spec)
    for ch in (0, 4, 16):
        with pytest.raises(NotImplementedError, match="input_ch"):
            _build(input_ch=ch)
    for feats in (None, (), ("stage6",), ("stage4", "res5")):
        with pytest.raises(ValueError, match="out_features"):
            _build(out_features=feats)
    with pytest.raises((KeyError, ValueError), match="V-99-eSE"):
        _build(spec_name="V-100")
    assert _build(input_ch=1).stem[0].weight.shape == (64, 1, 3, 3)


def test_inference_only_and_input_checks():
    m = _build(spec_name="V-19-eSE")
    m.train()
    with torch.enable_grad(), pytest.raises(NotImplementedError, match="inference only"):
        m(torch.zeros(1, 3, 32, 32))
    m.eval()
    with pytest.raises(ValueError, match="image"):
        m(torch.zeros(1, 4, 32, 32))
    with pytest.raises(ValueError, match="H, W >= 2"):
        m(torch.zeros(1, 3, 32, 9))   # 9 -> 5 -> 3 -> 1 (stage3's map): stage4's pool has nothing to take
    with pytest.raises(RuntimeError, match="HIP device"):
        m(torch.zeros(1, 3, 64, 64))   # the checks pass, the CPU tensor does not: no fallback


# ---- the oracle against the reference ------------------------------------------------------------------------

def test_oracle_equals_the_reference():
    """the float64 oracle on the by-key seeded V-39-eSE against the reference's own class: pins the ceil-mode
    pool (10 x 14 clips, 5 x 7 is exact), the gate in every block, the identity add and the hsigmoid"""
    g = np.load(os.path.join(GOLDEN, "vovnet_v39_ref.npz"))
    m = R.seed_by_key(_build(spec_name="V-39-eSE"), int(g["seed"]))
    x = R.seeded_image(int(g["image_seed"]), tuple(int(s) for s in g["shape"]))
    assert tuple(x.shape) == (2, 3, 37, 53)
    out = R.vovnet_ref(m.state_dict(), "V-39-eSE", x, ("stage4", "stage5"))
    assert list(out) == ["stage4", "stage5"]
    for k, shape in (("stage4", (2, 768, 2, 3)), ("stage5", (2, 1024, 1, 1))):
        ref = torch.from_numpy(g[k])
        assert tuple(out[k].shape) == tuple(ref.shape) == shape
        assert (out[k] - ref).abs().max().item() <= 1e-12 * ref.abs().max().item()
        assert ref.abs().max().item() > 1.0
    every = R.vovnet_ref(m.state_dict(), "V-39-eSE", x)
    assert list(every) == list(R.NAMES)
    assert [tuple(v.shape[1:]) for v in every.values()] == [(128, 10, 14), (256, 10, 14), (512, 5, 7), (768, 2, 3),
                                                             (1024, 1, 1)]


def test_pool_sizes_are_torchs():
    from projects.mmdet3d_plugin import native_img as NI
    for H in range(2, 41):
        for W in range(2, 41):
            want = F.max_pool2d(torch.zeros(1, 1, H, W), 3, 2, ceil_mode=True).shape[2:]
            assert NI.pool_hw(H, W) == tuple(want), (H, W)
    for hw in ((1, 5), (5, 1), (0, 3)):
        with pytest.raises(ValueError, match="H, W >= 2"):
            NI.pool_hw(*hw)
        if min(hw) == 1:
            with pytest.raises(RuntimeError):
                F.max_pool2d(torch.zeros(1, 1, *hw), 3, 2, ceil_mode=True)


# ---- packing against the oracle ------------------------------------------------------------------------------

def _stem_im2col(x):
    """float64 NCHW -> tap-major rows [B*Ho*Wo, 9 C] of the stride-2 / pad-1 window, written with explicit
    shifts (R.im2col3x3)"""
    return R.im2col3x3(x, 2)


@pytest.mark.parametrize("cin", [1, 3])
def test_stem_packing_matches_the_oracle(cin):
    from projects.mmdet3d_plugin import native_bev as NB
    from projects.mmdet3d_plugin import native_img as NI
    g = torch.Generator().manual_seed(70 + cin)
    B, Cout, H, W = 2, 64, 6, 9
    x = torch.randn(B, cin, H, W, generator=g)
    w = torch.randn(Cout, cin, 3, 3, generator=g) / (9 * cin) ** 0.5
    bn = R.random_bn(Cout, g)
    wp, shift = NI.pack_stem(w, list(bn) + [R.BN_EPS])
    assert wp.dtype == torch.uint16 and tuple(wp.shape) == (Cout, 2, NI.STEM_K) == (Cout, 2, 32)
    assert shift.dtype == torch.float32 and tuple(shift.shape) == (Cout,)
    assert not wp[:, :, 9 * cin:].any(), "the K padding columns must be zero"
    cols, Ho, Wo = _stem_im2col(x)
    wk = NB.unpack_pair(wp)
    got = R.nchw_of(cols @ wk[:, :9 * cin].T + shift.double(), B, Ho, Wo)
    want = R.conv_bn_relu(x, w, bn, R.BN_EPS, stride=2, relu=False)
    bound = 2.0 ** -21 * wk.abs().max().item() * cols.abs().sum(1).max().item() + 2.0 ** -24 * want.abs().max().item()
    assert (got - want).abs().max().item() <= bound
    assert want.abs().max().item() > 1.0
    with pytest.raises(ValueError, match="Cin <= 3"):
        NI.pack_stem(torch.zeros(64, 4, 3, 3), list(bn) + [R.BN_EPS])


def test_concat_packing_matches_the_oracle():
    from projects.mmdet3d_plugin import native_bev as NB
    from projects.mmdet3d_plugin import native_img as NI
    g = torch.Generator().manual_seed(73)
    B, Cs, Cout, H, W = 2, (64, 32, 32), 128, 3, 5
    xs = [torch.randn(B, c, H, W, generator=g) for c in Cs]
    w = torch.randn(Cout, sum(Cs), 1, 1, generator=g) / sum(Cs) ** 0.5
    bn = R.random_bn(Cout, g)
    wp, shift = NI.pack_concat(w, list(bn) + [R.BN_EPS])
    assert tuple(wp.shape) == (Cout, 2, sum(Cs))
    wk = NB.unpack_pair(wp)
    acc, off = shift.double()[None, :].repeat(B * H * W, 1), 0
    for x, c in zip(xs, Cs):    # the concatenation, source by source at its channel offset
        acc = acc + R.rows_of(x).double() @ wk[:, off:off + c].T
        off += c
    want = R.bn_relu(F.conv2d(torch.cat(xs, 1).double(), w.double()), bn, R.BN_EPS, relu=False)
    rows_abs = torch.cat([R.rows_of(x) for x in xs], 1).double().abs().sum(1).max().item()
    bound = 2.0 ** -21 * wk.abs().max().item() * rows_abs + 2.0 ** -24 * want.abs().max().item()
    assert (R.nchw_of(acc, B, H, W) - want).abs().max().item() <= bound
    with pytest.raises(ValueError, match="running_var"):
        NI.pack_concat(w, None)


def test_packs_follow_in_place_updates():
    m = R.seed_by_key(_build(spec_name="V-19-eSE"), 7)
    blk = m.stage3.OSA3_1
    s0, l0, c0, f0 = m.packed_stem(0), m.packed_layer("OSA3_1", blk, 1), m.packed_layer("OSA3_1", blk, "concat"), \
        m.packed_fc("OSA3_1", blk)
    assert m.packed_stem(0)[0] is s0[0] and m.packed_fc("OSA3_1", blk)[0] is f0[0]
    assert tuple(s0[0].shape) == (64, 2, 32) and tuple(l0[0].shape) == (160, 2, 9 * 160)
    assert tuple(c0[0].shape) == (512, 2, 256 + 3 * 160) and tuple(f0[0].shape) == (512, 512)
    with torch.no_grad():
        m.stem[0].weight.mul_(2.0)
        blk.layers[1][1].running_var.add_(1.0)
        blk.concat[1].bias.add_(1.0)
        blk.ese.fc.bias.add_(1.0)
    assert not torch.equal(m.packed_stem(0)[0].view(torch.int16), s0[0].view(torch.int16))
    l1 = m.packed_layer("OSA3_1", blk, 1)
    assert not torch.equal(l1[0].view(torch.int16), l0[0].view(torch.int16)) and not torch.equal(l1[1], l0[1])
    c1 = m.packed_layer("OSA3_1", blk, "concat")
    assert torch.equal(c1[0].view(torch.int16), c0[0].view(torch.int16)) and not torch.equal(c1[1], c0[1])
    f1 = m.packed_fc("OSA3_1", blk)
    assert torch.equal(f1[1], blk.ese.fc.bias) and torch.equal(f1[0], blk.ese.fc.weight.view(512, 512))
    blk.ese.fc.bias = torch.nn.Parameter(torch.zeros(512))   # a replaced tensor is followed too
    assert not m.packed_fc("OSA3_1", blk)[1].any()


# ---- the library and the wrappers ------------------------------------------------------------------------------

IMG_STRUCTS = ("img_stem", "img_conv", "img_concat", "img_gate", "img_apply", "img_pool")
IMG_ENTRIES = ("cmt_img_stem", "cmt_img_conv3x3", "cmt_img_concat1x1", "cmt_img_ese_gate", "cmt_img_ese_apply",
               "cmt_img_maxpool")


def test_library_exports_the_new_entries():
    from projects.mmdet3d_plugin import native
    from projects.mmdet3d_plugin import native_img as NI
    L = native.lib()
    assert L.cmt_abi_version() == 25 == native.ABI_VERSION
    raw = ctypes.CDLL(L._name)
    for key in IMG_STRUCTS:
        assert getattr(L, f"cmt_{key}_args_size")() == ctypes.sizeof(native.STRUCTS[key]), key
        assert hasattr(raw, f"cmt_{key}_args_size")
    for sym in IMG_ENTRIES + ("cmt_img_concat_tile_rows",):
        assert hasattr(raw, sym), sym
    assert L.cmt_img_concat_tile_rows() == NI.CONCAT_TM and native.IMG_MAX_SRC == NI.MAX_SRC == 8
    # bad arguments are refused by the library itself too (no device is touched before the checks)
    buf = (ctypes.c_char * 80)()
    p = ctypes.c_void_p((ctypes.addressof(buf) + 15) & ~15)   # a 16-byte aligned host address: never dereferenced
    for cls, fn in zip((native.ImgStemArgs, native.ImgConvArgs, native.ImgConcatArgs, native.ImgGateArgs,
                        native.ImgApplyArgs, native.ImgPoolArgs), IMG_ENTRIES):
        assert getattr(L, fn)(ctypes.byref(cls()), None) == 1001, fn
        assert b"non-null" in L.cmt_last_error(), fn
    c = native.ImgConvArgs()
    c.X, c.Wt, c.shift, c.Y = p, p, p, p
    c.B, c.H, c.W, c.Cin, c.Cout, c.stride, c.ldx, c.ldw, c.ldy = 1, 2, 2, 32, 288, 1, 64, 576, 576
    assert L.cmt_img_conv3x3(ctypes.byref(c), None) == 1001 and b"at most 256" in L.cmt_last_error()
    c.Cout, c.Cin = 160, 48
    assert L.cmt_img_conv3x3(ctypes.byref(c), None) == 1001 and b"Cin must be" in L.cmt_last_error()
    c.Cin, c.stride = 32, 3
    assert L.cmt_img_conv3x3(ctypes.byref(c), None) == 1001 and b"stride" in L.cmt_last_error()
    c.stride, c.nb = 1, 2                                     # 160 / 32 = 5 column blocks
    assert L.cmt_img_conv3x3(ctypes.byref(c), None) == 1001 and b"divisor" in L.cmt_last_error()
    s = native.ImgStemArgs()
    s.X, s.Wt, s.shift, s.Y = p, p, p, p
    s.B, s.H, s.W, s.Cin, s.Cout, s.x_bstride, s.ldy = 1, 2, 2, 4, 64, 16, 128
    assert L.cmt_img_stem(ctypes.byref(s), None) == 1001 and b"1, 2 or 3" in L.cmt_last_error()
    k = native.ImgConcatArgs()
    k.Wt, k.shift, k.Y, k.B, k.HW, k.Cout, k.nsrc = p, p, p, 1, 4, 128, 9
    assert L.cmt_img_concat1x1(ctypes.byref(k), None) == 1001 and b"1 to 8 sources" in L.cmt_last_error()
    k.nsrc, k.C[0], k.X[0], k.ldx[0] = 1, 48, p.value, 96
    assert L.cmt_img_concat1x1(ctypes.byref(k), None) == 1001 and b"multiple of 32" in L.cmt_last_error()
    q = native.ImgPoolArgs()
    q.X, q.Y, q.B, q.H, q.W, q.C, q.ldx, q.ldy = p, p, 1, 1, 5, 128, 256, 256
    assert L.cmt_img_maxpool(ctypes.byref(q), None) == 1001 and b"H, W >= 2" in L.cmt_last_error()


def _rows(n, c):
    return torch.zeros((n, 2, c), dtype=torch.uint16)


def test_wrappers_check_before_the_device():
    """every ValueError comes before the device check: all tensors here live on the CPU, and a call whose
    arguments are fine ends in the no-fallback RuntimeError instead"""
    from projects.mmdet3d_plugin import native_img as NI
    sh = lambda c: torch.zeros(c)   # noqa: E731
    V = pytest.raises(ValueError)
    # stem
    with V:
        NI.stem(torch.zeros(1, 4, 8, 8), _rows(64, 32), sh(64), Cout=64)
    with V:
        NI.stem(torch.zeros(1, 3, 8, 8), _rows(48, 32), sh(48), Cout=48)
    with V:
        NI.stem(torch.zeros(1, 3, 8, 8).double(), _rows(64, 32), sh(64), Cout=64)
    with V:
        NI.stem(torch.zeros(1, 3, 8, 8)[:, :, :, ::2], _rows(64, 32), sh(64), Cout=64)
    with V:
        NI.stem(torch.zeros(1, 3, 8, 8), _rows(64, 27), sh(64), Cout=64)
    # conv
    ok = dict(B=1, H=4, W=4, Cin=32, Cout=64, stride=1)
    with V:
        NI.conv3x3(_rows(16, 48), _rows(64, 9 * 48), sh(64), **dict(ok, Cin=48))
    with V:
        NI.conv3x3(_rows(16, 32), _rows(80, 9 * 32), sh(80), **dict(ok, Cout=80))
    with V:
        NI.conv3x3(_rows(16, 32), _rows(288, 9 * 32), sh(288), **dict(ok, Cout=288))
    with V:
        NI.conv3x3(_rows(16, 32), _rows(64, 9 * 32), sh(64), **dict(ok, stride=3))
    with V:
        NI.conv3x3(_rows(16, 32), _rows(96, 9 * 32), sh(96), nb=2, **dict(ok, Cout=96))
    gok = dict(B=1, H=4, W=4, Cin=64, Cout=128)
    with V:
        NI.conv3x3_gemm(_rows(16, 32), _rows(128, 9 * 32), sh(128), **dict(gok, Cin=32))   # the gemm path: % 64
    with V:
        NI.conv3x3_gemm(_rows(16, 64), _rows(96, 9 * 64), sh(96), **dict(gok, Cout=96))
    with V:
        NI.conv3x3_gemm(_rows(15, 64), _rows(128, 9 * 64), sh(128), **gok)
    with V:
        NI.conv3x3(_rows(15, 32), _rows(64, 9 * 32), sh(64), **ok)          # short X
    with V:
        NI.conv3x3(_rows(16, 32), _rows(64, 9 * 32), sh(64), out=_rows(15, 64), **ok)   # short out
    with V:
        NI.conv3x3(_rows(16, 32).view(torch.int16), _rows(64, 9 * 32), sh(64), **ok)    # wrong dtype
    with V:
        NI.conv3x3(_rows(16, 64)[:, :, :32], _rows(64, 9 * 32), sh(64), **ok)           # non-contiguous
    with V:
        NI.conv3x3(_rows(16, 32), _rows(64, 9 * 32), sh(64), range_flag=torch.zeros(1), **ok)
    # concat
    with V:
        NI.concat1x1([_rows(4, 32)] * 9, _rows(128, 288), sh(128), B=1, HW=4, Cout=128)
    with V:
        NI.concat1x1([], _rows(128, 32), sh(128), B=1, HW=4, Cout=128)
    with V:
        NI.concat1x1([_rows(4, 48)], _rows(128, 48), sh(128), B=1, HW=4, Cout=128)
    with V:
        NI.concat1x1([_rows(4, 32)], _rows(64, 32), sh(64), B=1, HW=4, Cout=64)
    with V:
        NI.concat1x1([_rows(3, 32)], _rows(128, 32), sh(128), B=1, HW=4, Cout=128)
    with V:
        NI.concat1x1([_rows(4, 32), _rows(4, 32)], _rows(128, 32), sh(128), B=1, HW=4, Cout=128)   # K of W
    with V:
        NI.concat1x1([_rows(4, 64)[:, :, :32]], _rows(128, 32), sh(128), B=1, HW=4, Cout=128)      # lo not at C
    with V:
        NI.concat1x1([_rows(4, 32)], _rows(128, 32), sh(128), B=1, HW=4, Cout=128, part=torch.zeros(1, 2, 128))
    wide = torch.zeros((4, 80), dtype=torch.uint16)[:, 8:72].view(4, 2, 32)   # a column slice: ld 80 > 2 C
    # gate
    with V:
        NI.ese_gate(torch.zeros(1, 2, 30), torch.zeros(30, 30), sh(30), HW=4)
    with V:
        NI.ese_gate(torch.zeros(1, 2, 32), torch.zeros(32, 16), sh(32), HW=4)
    with V:
        NI.ese_gate(torch.zeros(1, 2, 32), torch.zeros(32, 32), sh(32), HW=0)
    with V:
        NI.ese_gate(torch.zeros(1, 2, 32).half(), torch.zeros(32, 32), sh(32), HW=4)
    # apply
    with V:
        NI.ese_apply(_rows(4, 36), torch.zeros(1, 36), B=1, HW=4, C=36)
    with V:
        NI.ese_apply(_rows(4, 32), torch.zeros(2, 32), B=1, HW=4, C=32)
    with V:
        NI.ese_apply(_rows(4, 32), torch.zeros(1, 32), B=1, HW=4, C=32, identity=_rows(3, 32))
    # pool
    with V:
        NI.maxpool(_rows(5, 128), B=1, H=1, W=5, C=128)
    with V:
        NI.maxpool(_rows(9, 36), B=1, H=3, W=3, C=36)
    with V:
        NI.maxpool(_rows(8, 128), B=1, H=3, W=3, C=128)
    # the same calls with good arguments reach the device check
    D = pytest.raises(RuntimeError, match="HIP device")
    with D:
        NI.stem(torch.zeros(1, 3, 8, 8), _rows(64, 32), sh(64), Cout=64)
    with D:
        NI.conv3x3(_rows(16, 32), _rows(64, 9 * 32), sh(64), **ok)
    with D:
        NI.conv3x3_gemm(_rows(16, 64), _rows(128, 9 * 64), sh(128), **gok)
    with D:
        NI.concat1x1([_rows(4, 32), wide], _rows(128, 64), sh(128), B=1, HW=4, Cout=128, part=True)
    with D:
        NI.ese_gate(torch.zeros(1, 2, 32), torch.zeros(32, 32, 1, 1), sh(32), HW=4)
    with D:
        NI.ese_apply(_rows(4, 32), torch.zeros(1, 32), B=1, HW=4, C=32, identity=_rows(4, 32))
    with D:
        NI.maxpool(_rows(9, 128), B=1, H=3, W=3, C=128)
