"""Host side of the native CPFPN (no device): the registry, the state_dict layout, the unsupported-input
errors, the library's new symbols and structs, the wrappers' argument checks, the nearest-index rule, and
the 1 x 1 weight packing against the float64 oracle (tests/_fpn_ref.py) through a float64 GEMM."""
import ctypes
import os

import pytest
import torch
import torch.nn.functional as F

import _fpn_ref as R

REF_CONFIGS = "/root/reference/projects/configs"
# the reference's camera and fusion config files by name (the LiDAR configs have no img_neck)
IMG_NAMES = sorted(f"{d}/{n}.py" for d, n in [
    ("CMTCoop_TUMTraf/camera/coop", "cmt_camera_vov_1600x640_cbgs_a9coop_pretrained"),
    ("CMTCoop_TUMTraf/camera/infra", "cmt_camera_vov_1600x640_cbgs_a9coop_infrastructure_pretrained"),
    ("CMTCoop_TUMTraf/camera/vehicle", "cmt_camera_vov_1600x640_cbgs_a9coop_vehicle_pretrained"),
    ("CMTCoop_TUMTraf/fusion/coop", "cmt_voxel0075_vov_1600x640_cbgs_a9coop_pretrained"),
    ("CMTCoop_TUMTraf/fusion/infra", "cmt_voxel0075_vov_1600x640_cbgs_a9coop_infrastructure_pretrained"),
    ("CMTCoop_TUMTraf/fusion/vehicle", "cmt_voxel0075_vov_1600x640_cbgs_a9coop_vehicle_pretrained"),
    ("CMT_Nuscenes/camera", "cmt_camera_vov_1600x640_cbgs"),
    ("CMT_Nuscenes/fusion", "cmt_voxel0075_vov_1600x640_cbgs"),
    ("CMT_Nuscenes/fusion", "cmt_voxel0100_r50_800x320_cbgs"),
])

NECK_CFG = dict(type="CPFPN", in_channels=[768, 1024], out_channels=256, num_outs=2)
BN = dict(type="BN", eps=1e-3, momentum=0.01)
BN_KEYS = ("weight", "bias", "running_mean", "running_var", "num_batches_tracked")


def _build(**change):
    from projects.mmdet3d_plugin import build_neck
    return build_neck(dict(NECK_CFG, **change))


def _bias_keys(levels=2):
    keys = []
    for i in range(levels):
        keys += [f"lateral_convs.{i}.conv.weight", f"lateral_convs.{i}.conv.bias"]
    return keys + ["fpn_convs.0.conv.weight", "fpn_convs.0.conv.bias"]


def _bn_keys(levels=2, lateral_norm=True):
    keys = []
    for i in range(levels):
        if lateral_norm:
            keys += [f"lateral_convs.{i}.conv.weight"] + [f"lateral_convs.{i}.bn.{k}" for k in BN_KEYS]
        else:
            keys += [f"lateral_convs.{i}.conv.weight", f"lateral_convs.{i}.conv.bias"]
    return keys + ["fpn_convs.0.conv.weight"] + [f"fpn_convs.0.bn.{k}" for k in BN_KEYS]


def test_cpfpn_is_registered_and_exported():
    import projects.mmdet3d_plugin as P
    from projects.mmdet3d_plugin.models.necks import CPFPN
    assert "CPFPN" in P.NECKS and "SECONDFPN" in P.NECKS
    assert type(_build()) is CPFPN


def test_state_dict_keys_are_the_conv_module_layout():
    n = _build()
    assert sorted(n.state_dict().keys()) == sorted(_bias_keys())
    sd = n.state_dict()
    assert tuple(sd["lateral_convs.0.conv.weight"].shape) == (256, 768, 1, 1)
    assert tuple(sd["lateral_convs.1.conv.weight"].shape) == (256, 1024, 1, 1)
    assert tuple(sd["fpn_convs.0.conv.weight"].shape) == (256, 256, 3, 3) and n.fpn_convs[0].conv.padding == (1, 1)
    assert len(n.fpn_convs) == 1
    assert all(not sd[k].any() for k in sd if k.endswith("conv.bias")), "biases start at zero"
    assert sum(p.numel() for p in n.parameters()) == 768 * 256 + 1024 * 256 + 9 * 256 * 256 + 3 * 256
    b = _build(norm_cfg=BN, act_cfg=dict(type="ReLU"))
    assert sorted(b.state_dict().keys()) == sorted(_bn_keys())
    assert b.fpn_convs[0].bn.eps == 1e-3 and b.fpn_convs[0].bn.momentum == 0.01
    assert b.lateral_convs[0].conv.bias is None and b.fpn_convs[0].conv.bias is None
    nol = _build(norm_cfg=BN, no_norm_on_lateral=True)
    assert sorted(nol.state_dict().keys()) == sorted(_bn_keys(lateral_norm=False))
    # end_level cuts the levels used; the inputs are still one per entry of in_channels
    one = _build(in_channels=[768, 1024], end_level=1, num_outs=1)
    assert sorted(one.state_dict().keys()) == sorted(_bias_keys(1))
    three = _build(in_channels=[32, 48, 64], out_channels=128, num_outs=4)
    assert sorted(three.state_dict().keys()) == sorted(_bias_keys(3))


@pytest.mark.parametrize("form", ["bias", "bn"])
def test_conv_module_shaped_state_dict_loads_strictly(form):
    g = torch.Generator().manual_seed(5)
    n = _build() if form == "bias" else _build(norm_cfg=BN)
    sd = {}
    for prefix, shape in (("lateral_convs.0", (256, 768, 1, 1)), ("lateral_convs.1", (256, 1024, 1, 1)),
                          ("fpn_convs.0", (256, 256, 3, 3))):
        sd[f"{prefix}.conv.weight"] = torch.randn(shape, generator=g)
        if form == "bias":
            sd[f"{prefix}.conv.bias"] = torch.randn(256, generator=g)
        else:
            for k in BN_KEYS[:4]:
                sd[f"{prefix}.bn.{k}"] = torch.rand(256, generator=g) + 0.5
            sd[f"{prefix}.bn.num_batches_tracked"] = torch.tensor(7)
    res = n.load_state_dict(sd, strict=True)
    assert res.missing_keys == [] and res.unexpected_keys == []
    assert torch.equal(n.fpn_convs[0].conv.weight, sd["fpn_convs.0.conv.weight"])
    back = n.state_dict()
    assert sorted(back.keys()) == sorted(sd.keys()) and all(torch.equal(back[k], sd[k]) for k in sd)
    with pytest.raises(RuntimeError):
        n.load_state_dict(dict(sd, **{"fpn_convs.1.conv.weight": torch.zeros(1)}), strict=True)


def test_defaults_are_the_references():
    from projects.mmdet3d_plugin.models.necks import CPFPN
    n = CPFPN([768, 1024], 256, 2)
    assert (n.start_level, n.end_level, n.backbone_end_level, n.num_ins, n.num_outs) == (0, -1, 2, 2, 2)
    assert not n.add_extra_convs and not n.relu_before_extra_convs and not n.no_norm_on_lateral
    assert n.upsample_cfg == dict(mode="nearest")
    assert not hasattr(n.lateral_convs[0], "bn") and not hasattr(n.lateral_convs[0], "activate")


@pytest.mark.parametrize("change,match", [
    (dict(add_extra_convs=True), "add_extra_convs"),
    (dict(add_extra_convs="on_output"), "add_extra_convs"),
    (dict(start_level=1, num_outs=1), "start_level"),
    (dict(upsample_cfg=dict(mode="nearest", scale_factor=2)), "scale_factor"),
    (dict(upsample_cfg=dict(mode="bilinear")), "nearest"),
    (dict(norm_cfg=dict(type="GN", num_groups=32)), "BN"),
    (dict(act_cfg=dict(type="GELU")), "ReLU"),
    (dict(conv_cfg=dict(type="DCNv2")), "conv_cfg"),
    (dict(in_channels=[768, 1000]), "% 16"),
    (dict(out_channels=192), "% 128"),
])
def test_limits_raise_at_construction(change, match):
    with pytest.raises(NotImplementedError, match=match):
        _build(**change)


def test_level_arithmetic_is_checked():
    with pytest.raises(ValueError, match="num_outs"):
        _build(num_outs=1)
    with pytest.raises(ValueError, match="num_outs"):
        _build(end_level=1, num_outs=2)
    with pytest.raises(ValueError, match="end_level"):
        _build(end_level=3, num_outs=3)


def test_forward_errors_come_before_the_device_check():
    n = _build(in_channels=[32, 48], out_channels=128).eval()
    with pytest.raises(NotImplementedError, match="width 181"):
        n([torch.zeros(1, 32, 4, 181), torch.zeros(1, 48, 2, 91)])
    with pytest.raises(ValueError, match="larger than the finer"):
        n([torch.zeros(1, 32, 4, 6), torch.zeros(1, 48, 5, 3)])
    with pytest.raises(ValueError, match="larger than the finer"):
        n([torch.zeros(1, 32, 4, 6), torch.zeros(1, 48, 2, 7)])
    with pytest.raises(ValueError, match="2 maps"):
        n([torch.zeros(1, 32, 4, 6)])
    with pytest.raises(ValueError, match="48"):
        n([torch.zeros(1, 32, 4, 6), torch.zeros(1, 32, 2, 3)])
    with pytest.raises(ValueError, match="one batch size"):
        n([torch.zeros(1, 32, 4, 6), torch.zeros(2, 48, 2, 3)])
    with pytest.raises(RuntimeError, match="HIP device"):
        n([torch.zeros(1, 32, 4, 6), torch.zeros(1, 48, 2, 3)])
    n.train()
    with pytest.raises(NotImplementedError, match="inference only"):
        n([torch.zeros(1, 32, 4, 6), torch.zeros(1, 48, 2, 3)])
    n.check_input_range()   # no forward yet: nothing to report


def test_wrapper_checks_raise_value_errors_on_the_host():
    from projects.mmdet3d_plugin import native_fpn as NF
    u16 = torch.uint16
    x = torch.zeros(2, 32, 5, 7)
    Wp, sh = torch.zeros(128, 2, 32, dtype=u16), torch.zeros(128)
    top = torch.zeros(2 * 3 * 4, 2, 128, dtype=u16)
    with pytest.raises(RuntimeError, match="HIP device"):
        NF.lateral(x, Wp, sh, Cout=128)
    with pytest.raises(RuntimeError, match="HIP device"):
        NF.lateral(x, Wp, sh, Cout=128, top=top, top_hw=(3, 4))
    with pytest.raises(ValueError, match="x must be"):
        NF.lateral(x.double(), Wp, sh, Cout=128)
    with pytest.raises(ValueError, match="x must be"):
        NF.lateral(x.permute(0, 1, 3, 2), Wp, sh, Cout=128)
    with pytest.raises(ValueError, match="Cin % 16"):
        NF.lateral(torch.zeros(2, 24, 5, 7), torch.zeros(128, 2, 24, dtype=u16), sh, Cout=128)
    with pytest.raises(ValueError, match="Cout % 128"):
        NF.lateral(x, torch.zeros(64, 2, 32, dtype=u16), torch.zeros(64), Cout=64)
    with pytest.raises(ValueError, match="Wp must"):
        NF.lateral(x, Wp[:, :, :16], sh, Cout=128)
    with pytest.raises(ValueError, match="Wp must"):
        NF.lateral(x, torch.zeros(256, 2, 32, dtype=u16), sh, Cout=128)
    with pytest.raises(ValueError, match="shift"):
        NF.lateral(x, Wp, sh.double(), Cout=128)
    with pytest.raises(ValueError, match="range_flag"):
        NF.lateral(x, Wp, sh, Cout=128, range_flag=torch.zeros(1))
    with pytest.raises(ValueError, match="go together"):
        NF.lateral(x, Wp, sh, Cout=128, top=top)
    for hw in ((6, 4), (3, 8), (0, 4)):
        with pytest.raises(ValueError, match="coarser map"):
            NF.lateral(x, Wp, sh, Cout=128, top=top, top_hw=hw)
    with pytest.raises(ValueError, match="top must be"):
        NF.lateral(x, Wp, sh, Cout=128, top=top[:23], top_hw=(3, 4))
    with pytest.raises(ValueError, match="out must be"):
        NF.lateral(x, Wp, sh, Cout=128, out=torch.zeros(69, 2, 128, dtype=u16))   # 2 * 5 * 7 = 70 rows needed
    rows = torch.zeros(70, 2, 128, dtype=u16)
    with pytest.raises(RuntimeError, match="HIP device"):
        NF.rows_to_nchw(rows, (2, 128, 5, 7))
    with pytest.raises(ValueError, match="rows must be"):
        NF.rows_to_nchw(rows, (2, 128, 5, 8))
    with pytest.raises(ValueError, match="rows must be"):
        NF.rows_to_nchw(rows.view(torch.int16).float(), (2, 128, 5, 7))
    with pytest.raises(ValueError, match="C % 8"):
        NF.rows_to_nchw(torch.zeros(70, 2, 12, dtype=u16), (2, 12, 5, 7))
    with pytest.raises(ValueError, match="out must be"):
        NF.rows_to_nchw(rows, (2, 128, 5, 7), out=torch.zeros(2, 128, 7, 5))
    with pytest.raises(ValueError, match="1, 1"):
        NF.pack_conv1x1(torch.zeros(128, 32, 3, 3), None)
    with pytest.raises(ValueError, match="bias"):
        NF.pack_conv1x1(torch.zeros(128, 32, 1, 1), torch.zeros(64))


# every (in, out) the GPU tests and the reference geometry use, the two the issue names (2 -> 82, 3 -> 123: the
# integer rule in * dst // out differs there), and the whole range in <= 64, out < 130
NEAREST_NAMED = [(2, 82), (3, 123), (3, 6), (5, 10), (3, 5), (7, 13), (4, 7), (5, 9), (1, 5), (1, 7), (5, 5), (7, 7),
                 (1, 2), (20, 40), (50, 100)]


def test_nearest_index_is_torchs():
    from projects.mmdet3d_plugin import native_fpn as NF
    pairs = NEAREST_NAMED + [(i, o) for i in range(1, 65) for o in range(i, 130)]
    integer_rule_differs = 0
    for i, o in pairs:
        src = torch.arange(i, dtype=torch.float32).view(1, 1, i, 1)
        want = F.interpolate(src, size=(o, 1), mode="nearest").view(-1).to(torch.int64)
        got = NF.nearest_index(o, i)
        assert torch.equal(got, want), (i, o)
        integer_rule_differs += int(not torch.equal(torch.arange(o) * i // o, want))
    assert integer_rule_differs > 0, "the integer rule is the same everywhere: the named pairs test nothing"
    for i, o in ((2, 82), (3, 123)):
        src = torch.arange(i, dtype=torch.float32).view(1, 1, 1, i)
        want = F.interpolate(src, size=(1, o), mode="nearest").view(-1).to(torch.int64)
        assert not torch.equal(torch.arange(o) * i // o, want), (i, o)


def test_library_exports_the_new_entries():
    from projects.mmdet3d_plugin import native
    L = native.lib()
    assert L.cmt_abi_version() == 25 == native.ABI_VERSION
    for key, cls in (("fpn_lateral", native.FpnLateralArgs), ("rows_to_nchw", native.RowsToNchwArgs)):
        assert native.STRUCTS[key] is cls
        assert getattr(L, f"cmt_{key}_args_size")() == ctypes.sizeof(cls), key
    raw = ctypes.CDLL(L._name)
    for sym in ("cmt_fpn_lateral", "cmt_rows_to_nchw", "cmt_fpn_lateral_args_size", "cmt_rows_to_nchw_args_size"):
        assert hasattr(raw, sym), sym
    # bad arguments are refused by the library itself too (no device is touched before the checks)
    a = native.FpnLateralArgs()
    assert L.cmt_fpn_lateral(ctypes.byref(a), None) == 1001
    assert b"non-null" in L.cmt_last_error()
    buf = (ctypes.c_char * 80)()
    p = ctypes.c_void_p((ctypes.addressof(buf) + 15) & ~15)   # a 16-byte aligned host address: never dereferenced
    a.X, a.Wt, a.shift, a.L = p, p, p, p
    a.B, a.H, a.W, a.Cin, a.Cout, a.x_bstride, a.ldw, a.ldl = 1, 2, 2, 24, 128, 96, 48, 256
    assert L.cmt_fpn_lateral(ctypes.byref(a), None) == 1001 and b"multiple of 16" in L.cmt_last_error()
    a.Cin, a.x_bstride, a.ldw, a.Cout = 32, 128, 64, 64
    assert L.cmt_fpn_lateral(ctypes.byref(a), None) == 1001 and b"multiple of 128" in L.cmt_last_error()
    a.Cout, a.T, a.ldt, a.Htop, a.Wtop = 128, p, 256, 3, 1
    assert L.cmt_fpn_lateral(ctypes.byref(a), None) == 1001 and b"Htop" in L.cmt_last_error()
    r = native.RowsToNchwArgs()
    assert L.cmt_rows_to_nchw(ctypes.byref(r), None) == 1001
    r.X, r.Y, r.B, r.C, r.HW, r.ldx = p, p, 1, 12, 4, 24
    assert L.cmt_rows_to_nchw(ctypes.byref(r), None) == 1001 and b"multiple of 8" in L.cmt_last_error()


# ---- packing against the oracle ------------------------------------------------------------------------------

@pytest.mark.parametrize("form", ["bias", "bn", "none"])
def test_conv1x1_packing_matches_the_oracle(form):
    """pack_conv1x1 unpacks to the float64 folded weight within the f16-pair rounding of W' alone: per output
    2^-21 max|W'| sum|x| (cmt_hip.h CMT_F16P), plus the fp32 rounding of the shift"""
    from projects.mmdet3d_plugin import native_bev as NB
    from projects.mmdet3d_plugin import native_fpn as NF
    g = torch.Generator().manual_seed(61)
    B, Cin, Cout, H, W, eps = 2, 48, 128, 5, 7, 1e-3
    x = torch.randn(B, Cin, H, W, generator=g)
    w = torch.randn(Cout, Cin, 1, 1, generator=g) / Cin ** 0.5
    bias = 0.5 * torch.randn(Cout, generator=g) if form == "bias" else None
    bn = R.random_bn(Cout, g) if form == "bn" else None
    wp, shift = NF.pack_conv1x1(w, list(bn) + [eps] if bn is not None else bias)
    assert wp.dtype == torch.uint16 and tuple(wp.shape) == (Cout, 2, Cin)
    assert shift.dtype == torch.float32 and tuple(shift.shape) == (Cout,)
    rows = R.rows_of(x).double()
    got = R.nchw_of(rows @ NB.unpack_pair(wp).T + shift.double(), B, H, W)
    want = R.conv_norm_act(x, w, bias, bn, eps, relu=False)
    bound = 2.0 ** -21 * NB.unpack_pair(wp).abs().max().item() * rows.abs().sum(1).max().item() + \
        2.0 ** -24 * want.abs().max().item()
    assert (got - want).abs().max().item() <= bound
    assert want.abs().max().item() > 1.0
    if form == "bias":
        assert torch.equal(shift, bias)
    if form == "none":
        assert not shift.any()


def test_conv3x3_bias_packing_is_the_identity_norm():
    from projects.mmdet3d_plugin import native_bev as NB
    from projects.mmdet3d_plugin import native_fpn as NF
    g = torch.Generator().manual_seed(62)
    w = torch.randn(128, 128, 3, 3, generator=g) / (9 * 128) ** 0.5
    bias = torch.randn(128, generator=g)
    wp, shift = NF.pack_conv3x3_bias(w, bias)
    assert torch.equal(shift, bias)
    assert torch.equal(wp.view(torch.int16), NB.split_pair(w.double().permute(0, 2, 3, 1).reshape(128, -1)).view(torch.int16))
    bn = list(R.random_bn(128, g)) + [1e-3]
    wb, sb = NF.pack_conv3x3_bias(w, bn)
    wr, sr = NB.pack_conv3x3(w, bn)
    assert torch.equal(wb.view(torch.int16), wr.view(torch.int16)) and torch.equal(sb, sr)


def test_packs_follow_in_place_updates():
    """PackCache: keyed on every tensor a pack is made from"""
    n = R.seed_neck(_build(in_channels=[32, 48], out_channels=128), 7)
    w0, s0 = n.packed("lateral", 1)
    assert n.packed("lateral", 1)[0] is w0
    with torch.no_grad():
        n.lateral_convs[1].conv.weight.mul_(2.0)
    w1, s1 = n.packed("lateral", 1)
    assert w1 is not w0 and not torch.equal(w1.view(torch.int16), w0.view(torch.int16)) and torch.equal(s0, s1)
    with torch.no_grad():
        n.lateral_convs[1].conv.bias.add_(1.0)
    w2, s2 = n.packed("lateral", 1)
    assert not torch.equal(s2, s1) and torch.equal(s2, n.lateral_convs[1].conv.bias)
    f0 = n.packed("fpn")
    assert tuple(f0[0].shape) == (128, 2, 9 * 128)
    with torch.no_grad():
        n.fpn_convs[0].conv.bias.add_(1.0)
    assert not torch.equal(n.packed("fpn")[1], f0[1])
    b = R.seed_neck(_build(in_channels=[32, 48], out_channels=128, norm_cfg=BN), 8)
    p0 = b.packed("lateral", 0)
    with torch.no_grad():
        b.lateral_convs[0].bn.running_var.add_(1.0)
    p1 = b.packed("lateral", 0)
    assert not torch.equal(p1[0].view(torch.int16), p0[0].view(torch.int16)) and not torch.equal(p1[1], p0[1])


def test_oracle_is_the_restated_forward():
    """the oracle itself: three levels against an explicit loop over torch ops on one output element each"""
    n = R.seed_neck(_build(in_channels=[32, 48, 64], out_channels=128, num_outs=4), 9).eval()
    g = torch.Generator().manual_seed(10)
    xs = [torch.randn(2, 32, 6, 10, generator=g), torch.randn(2, 48, 3, 5, generator=g),
          torch.randn(2, 64, 2, 3, generator=g)]
    outs = R.cpfpn_ref(n, xs)
    assert [tuple(o.shape) for o in outs] == [(2, 128, 6, 10), (2, 128, 3, 5), (2, 128, 2, 3), (2, 128, 1, 2)]
    assert torch.equal(outs[3], outs[2][:, :, ::2, ::2])
    lat2 = F.conv2d(xs[2].double(), n.lateral_convs[2].conv.weight.double(), n.lateral_convs[2].conv.bias.double())
    assert torch.allclose(outs[2], lat2, rtol=0, atol=1e-12)
    lat1 = F.conv2d(xs[1].double(), n.lateral_convs[1].conv.weight.double(), n.lateral_convs[1].conv.bias.double())
    iy, ix = torch.tensor([0, 0, 1]), torch.tensor([0, 0, 1, 1, 2])   # 2 -> 3 rows, 3 -> 5 columns
    assert torch.allclose(outs[1], lat1 + lat2[:, :, iy][:, :, :, ix], rtol=0, atol=1e-12)


@pytest.mark.parametrize("name", IMG_NAMES)
def test_reference_img_neck_builds(name):
    if not os.path.isdir(REF_CONFIGS):
        pytest.skip("reference checkout not present")
    from projects.mmdet3d_plugin import build_neck
    from projects.mmdet3d_plugin.config import load_config
    model = load_config(os.path.join(REF_CONFIGS, name))["model"]
    # the cooperative configs hold one headless model per agent
    parts = [m for m in (model, model.get("vehicle_model"), model.get("infrastructure_model"))
             if isinstance(m, dict) and "img_neck" in m]
    assert parts
    for part in parts:
        n = build_neck(part["img_neck"])
        assert type(n).__name__ == "CPFPN" == part["img_neck"]["type"]
        assert sorted(n.state_dict().keys()) == sorted(_bias_keys())
        assert n.out_channels == 256 and n.num_outs == 2 and len(n.fpn_convs) == 1
