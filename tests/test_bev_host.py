"""Host side of the native SECOND / SECONDFPN (no device): registries, state_dict layout, the
unsupported-input errors, the library's new symbols and structs, and the weight packing checked
against the float64 oracle (tests/_bev_ref.py) through a float64 GEMM, which isolates the index maths
(tap-major im2col, the (dy, dx, n) pixel shuffle, the BN fold) from the kernels."""
import ctypes
import os

import pytest
import torch

import _bev_ref as R

REF_CONFIGS = "/root/reference/projects/configs"
# the reference's LiDAR and fusion config files by name (the camera configs have no pts_backbone)
LIDAR_NAMES = sorted(f"{d}/{n}.py" for d, n in [
    ("CMTCoop_TUMTraf/fusion/coop", "cmt_voxel0075_vov_1600x640_cbgs_a9coop_pretrained"),
    ("CMTCoop_TUMTraf/fusion/infra", "cmt_voxel0075_vov_1600x640_cbgs_a9coop_infrastructure_pretrained"),
    ("CMTCoop_TUMTraf/fusion/vehicle", "cmt_voxel0075_vov_1600x640_cbgs_a9coop_vehicle_pretrained"),
    ("CMTCoop_TUMTraf/lidar/coop", "cmt_lidar_voxel0075_cbgs_a9coop_pretrained"),
    ("CMTCoop_TUMTraf/lidar/infra", "cmt_lidar_voxel0075_cbgs_a9coop_infrastructure_pretrained"),
    ("CMTCoop_TUMTraf/lidar/vehicle", "cmt_lidar_voxel0075_cbgs_a9coop_vehicle_pretrained"),
    ("CMT_Nuscenes/fusion", "cmt_voxel0075_vov_1600x640_cbgs"),
    ("CMT_Nuscenes/fusion", "cmt_voxel0100_r50_800x320_cbgs"),
    ("CMT_Nuscenes/lidar", "cmt_lidar_voxel0075_cbgs"),
])

BN = dict(type="BN", eps=1e-3, momentum=0.01)
BACKBONE_CFG = dict(type="SECOND", in_channels=256, out_channels=[128, 256], layer_nums=[5, 5], layer_strides=[1, 2],
                    norm_cfg=BN, conv_cfg=dict(type="Conv2d", bias=False))
NECK_CFG = dict(type="SECONDFPN", in_channels=[128, 256], out_channels=[256, 256], upsample_strides=[1, 2],
                norm_cfg=BN, upsample_cfg=dict(type="deconv", bias=False), use_conv_for_no_stride=True)
BN_KEYS = ("weight", "bias", "running_mean", "running_var", "num_batches_tracked")


def _build():
    from projects.mmdet3d_plugin import build_backbone, build_neck
    return build_backbone(BACKBONE_CFG), build_neck(NECK_CFG)


def _backbone_keys():
    keys = []
    for i in range(2):
        for j in range(6):
            keys.append(f"blocks.{i}.{3 * j}.weight")
            keys += [f"blocks.{i}.{3 * j + 1}.{k}" for k in BN_KEYS]
    return keys


def _neck_keys():
    keys = []
    for i in range(2):
        keys.append(f"deblocks.{i}.0.weight")
        keys += [f"deblocks.{i}.1.{k}" for k in BN_KEYS]
    return keys


def test_registries_are_exported():
    import projects.mmdet3d_plugin as P
    from projects.mmdet3d_plugin import registry
    assert "SECOND" in P.BACKBONES and "SECONDFPN" in P.NECKS
    assert P.build_backbone is registry.build_backbone and P.build_neck is registry.build_neck
    for name in ("BACKBONES", "NECKS", "build_backbone", "build_neck"):
        assert name in registry.__all__


def test_config_builds_with_the_reference_layout():
    b, n = _build()
    assert type(b).__name__ == "SECOND" and type(n).__name__ == "SECONDFPN"
    assert list(b.state_dict().keys()) == _backbone_keys()
    assert list(n.state_dict().keys()) == _neck_keys()
    assert _backbone_keys()[0] == "blocks.0.0.weight" and _backbone_keys()[1] == "blocks.0.1.weight"
    # parameters from the config values: bias-free convs + the BN affine pairs
    want_b = 256 * 128 * 9 + 5 * 128 * 128 * 9 + 6 * 2 * 128 + 128 * 256 * 9 + 5 * 256 * 256 * 9 + 6 * 2 * 256
    want_n = 128 * 256 + 2 * 256 + 256 * 256 * 4 + 2 * 256
    assert sum(p.numel() for p in b.parameters()) == want_b
    assert sum(p.numel() for p in n.parameters()) == want_n
    sd = b.state_dict()
    assert tuple(sd["blocks.0.0.weight"].shape) == (128, 256, 3, 3)
    assert tuple(sd["blocks.1.0.weight"].shape) == (256, 128, 3, 3) and b.blocks[1][0].stride == (2, 2)
    assert b.blocks[0][1].eps == 1e-3 and b.blocks[0][1].momentum == 0.01


def test_mmdet3d_shaped_state_dict_loads_strictly():
    b, n = _build()
    g = torch.Generator().manual_seed(3)
    sd_b = {}
    chans = [(256, 128), (128, 256)]
    for i, (cin, cout) in enumerate(chans):
        for j in range(6):
            sd_b[f"blocks.{i}.{3 * j}.weight"] = torch.randn(cout, cin if j == 0 else cout, 3, 3, generator=g)
            for k in BN_KEYS[:4]:
                sd_b[f"blocks.{i}.{3 * j + 1}.{k}"] = torch.rand(cout, generator=g) + 0.5
            sd_b[f"blocks.{i}.{3 * j + 1}.num_batches_tracked"] = torch.tensor(7)
    assert b.load_state_dict(sd_b, strict=True).missing_keys == []
    assert torch.equal(b.blocks[1][3].weight, sd_b["blocks.1.3.weight"])
    # the 1 x 1 Conv2d of use_conv_for_no_stride is (Cout, Cin, 1, 1), the deconv (Cin, Cout, k, k)
    sd_n = {"deblocks.0.0.weight": torch.randn(256, 128, 1, 1, generator=g),
            "deblocks.1.0.weight": torch.randn(256, 256, 2, 2, generator=g)}
    for i in range(2):
        for k in BN_KEYS[:4]:
            sd_n[f"deblocks.{i}.1.{k}"] = torch.rand(256, generator=g) + 0.5
        sd_n[f"deblocks.{i}.1.num_batches_tracked"] = torch.tensor(7)
    assert n.load_state_dict(sd_n, strict=True).missing_keys == []
    from projects.mmdet3d_plugin import build_neck
    deconv1 = build_neck(dict(NECK_CFG, in_channels=[64, 256], use_conv_for_no_stride=False))
    assert tuple(deconv1.state_dict()["deblocks.0.0.weight"].shape) == (64, 256, 1, 1)   # (Cin, Cout, 1, 1)


def test_defaults_are_mmdet3ds():
    from projects.mmdet3d_plugin.models.backbones import SECOND
    from projects.mmdet3d_plugin.models.necks import SECONDFPN
    b, n = SECOND(), SECONDFPN()
    assert (b.in_channels, b.out_channels, b.layer_nums, b.layer_strides) == (128, [128, 128, 256], [3, 5, 5], [2, 2, 2])
    assert (n.in_channels, n.out_channels, n.upsample_strides) == ([128, 128, 256], [256, 256, 256], [1, 2, 4])
    assert not n.use_conv_for_no_stride and isinstance(n.deblocks[0][0], torch.nn.ConvTranspose2d)
    assert [len(blk) for blk in b.blocks] == [12, 18, 18]


@pytest.mark.parametrize("change,match", [
    (dict(out_channels=[96, 256]), "multiples of 128"),
    (dict(in_channels=24), "multiple of 16"),
    (dict(in_channels=48, layer_strides=[2, 2]), "multiple of 32"),
    (dict(conv_cfg=dict(type="Conv2d", bias=True)), "biased"),
    (dict(norm_cfg=dict(type="GN", num_groups=8)), "BN"),
    (dict(layer_strides=[1, 3]), "strides 1 and 2"),
])
def test_backbone_limits_raise_at_construction(change, match):
    from projects.mmdet3d_plugin import build_backbone
    with pytest.raises(NotImplementedError, match=match):
        build_backbone(dict(BACKBONE_CFG, **change))


@pytest.mark.parametrize("change,match", [
    (dict(out_channels=[256, 64]), "% 128"),
    (dict(in_channels=[128, 40]), "% 32"),
    (dict(upsample_cfg=dict(type="deconv", bias=True)), "biased"),
    (dict(conv_cfg=dict(type="Conv2d", bias=True)), "biased"),
    (dict(norm_cfg=dict(type="LN")), "BN"),
    (dict(upsample_strides=[1, 3]), "1, 2 and 4"),
    (dict(upsample_strides=[0.5, 1]), "1, 2 and 4"),
])
def test_neck_limits_raise_at_construction(change, match):
    from projects.mmdet3d_plugin import build_neck
    with pytest.raises(NotImplementedError, match=match):
        build_neck(dict(NECK_CFG, **change))


def test_forward_errors_come_before_the_device_check():
    """widths above 180, unequal deblock outputs, training with grad: raised on CPU tensors, i.e. before any
    device work (a CPU tensor that passes the checks gets the 'no CPU fallback' RuntimeError)"""
    from projects.mmdet3d_plugin import native_bev as NB
    b, n = _build()
    b.eval(), n.eval()
    with pytest.raises(NotImplementedError, match="width 181"):
        b(torch.zeros(1, 256, 4, 181))
    with pytest.raises(ValueError, match="256"):
        b(torch.zeros(1, 128, 4, 4))
    with pytest.raises(ValueError, match="differ in size"):
        n([torch.zeros(1, 128, 8, 8), torch.zeros(1, 256, 5, 4)])
    with pytest.raises(ValueError, match="2 maps"):
        n([torch.zeros(1, 128, 8, 8)])
    with pytest.raises(RuntimeError, match="HIP device"):
        b(torch.zeros(1, 256, 4, 4))
    rows = NB.RowMap(torch.zeros(64, 2, 128, dtype=torch.uint16), (1, 128, 8, 8))
    assert rows.shape == (1, 128, 8, 8) and tuple(rows.nchw().shape) == (1, 128, 8, 8)
    with pytest.raises(RuntimeError, match="HIP device"):
        n([rows, torch.zeros(1, 256, 4, 4)])
    b.train(), n.train()
    with pytest.raises(NotImplementedError, match="inference only"):
        b(torch.zeros(1, 256, 4, 4))
    with pytest.raises(NotImplementedError, match="inference only"):
        n([torch.zeros(1, 128, 8, 8), torch.zeros(1, 256, 4, 4)])
    b.check_input_range(), n.check_input_range()   # no forward yet: nothing to report


def test_wrapper_checks_raise_value_errors_on_the_host():
    from projects.mmdet3d_plugin import native_bev as NB
    u16, f32 = torch.uint16, torch.float32
    X = torch.zeros(2 * 5 * 7, 2, 32, dtype=u16)
    Wc, sh = torch.zeros(128, 2, 288, dtype=u16), torch.zeros(128)
    ok = dict(B=2, H=5, W=7, Cin=32, Cout=128, stride=2)
    with pytest.raises(RuntimeError, match="HIP device"):
        NB.conv3x3(X, Wc, sh, **ok)
    for bad in (dict(stride=3), dict(Cin=16), dict(Cout=64), dict(W=181), dict(B=3), dict(H=0)):
        with pytest.raises(ValueError):
            NB.conv3x3(X, Wc, sh, **dict(ok, **bad))
    with pytest.raises(ValueError, match="X must be"):
        NB.conv3x3(X.view(torch.int16).float(), Wc, sh, **ok)
    with pytest.raises(ValueError, match="Wp must be"):
        NB.conv3x3(X, Wc[:, :, :287], sh, **ok)
    with pytest.raises(ValueError, match="shift"):
        NB.conv3x3(X, Wc, sh.double(), **ok)
    with pytest.raises(ValueError, match="out must be"):
        NB.conv3x3(X, Wc, sh, out=torch.zeros(23, 2, 128, dtype=u16), **ok)   # 2 * 3 * 4 = 24 rows needed
    with pytest.raises(ValueError, match="range_flag"):
        NB.conv3x3(X, Wc, sh, range_flag=torch.zeros(1), **ok)
    Wd = torch.zeros(4 * 128, 2, 32, dtype=u16)
    out = torch.zeros(2, 256, 10, 14)
    okd = dict(B=2, H=5, W=7, Cin=32, Cout=128, k=2, c0=128)
    with pytest.raises(RuntimeError, match="HIP device"):
        NB.deblock(X, Wd, sh, out, **okd)
    for bad in (dict(k=3), dict(c0=129), dict(c0=-1), dict(Cin=48), dict(Cout=192)):
        with pytest.raises(ValueError):
            NB.deblock(X, Wd, sh, out, **dict(okd, **bad))
    with pytest.raises(ValueError, match="out must be"):
        NB.deblock(X, Wd, sh, out[:, :, :, :13], **okd)
    with pytest.raises(ValueError, match="out must be"):
        NB.deblock(X, Wd, sh, out.permute(0, 1, 3, 2), **okd)
    with pytest.raises(ValueError, match="Wp must be"):
        NB.deblock(X, Wd[:128], sh, out, **okd)
    with pytest.raises(ValueError):
        NB.conv3x3_nchw_gemm(torch.zeros(1, 24, 4, 4), torch.zeros(128, 2, 216, dtype=u16), sh, Cout=128)
    with pytest.raises(ValueError):
        NB.to_rows(torch.zeros(1, 32, 4, 4, dtype=torch.float64))


def test_library_exports_the_new_entries():
    from projects.mmdet3d_plugin import native
    L = native.lib()
    assert L.cmt_abi_version() == 25 == native.ABI_VERSION
    for key, cls in (("bev_conv", native.BevConvArgs), ("bev_deblock", native.BevDeblockArgs)):
        assert native.STRUCTS[key] is cls
        assert getattr(L, f"cmt_{key}_args_size")() == ctypes.sizeof(cls), key
    assert L.cmt_gemm_args_size() == ctypes.sizeof(native.GemmArgs)
    raw = ctypes.CDLL(L._name)
    for sym in ("cmt_bev_conv3x3", "cmt_bev_deblock", "cmt_bev_conv_args_size", "cmt_bev_deblock_args_size"):
        assert hasattr(raw, sym), sym
    # bad arguments are refused by the library itself too (no device is touched before the checks)
    a = native.BevConvArgs()
    assert L.cmt_bev_conv3x3(ctypes.byref(a), None) == 1001
    assert b"null" in L.cmt_last_error() or b"non-null" in L.cmt_last_error()
    d = native.BevDeblockArgs()
    assert L.cmt_bev_deblock(ctypes.byref(d), None) == 1001


# ---- packing against the oracle ------------------------------------------------------------------------------

def _weight_bound(wp, x_rows_abs_sum):
    """the f16-pair rounding of W' only: 2^-21 max|W'| sum|x| per output (cmt_hip.h CMT_F16P)"""
    from projects.mmdet3d_plugin import native_bev as NB
    return 2.0 ** -21 * NB.unpack_pair(wp).abs().max().item() * x_rows_abs_sum


@pytest.mark.parametrize("stride", [1, 2])
@pytest.mark.parametrize("hw", [(7, 9), (8, 10), (1, 5)])
def test_conv_packing_matches_the_oracle(stride, hw):
    from projects.mmdet3d_plugin import native_bev as NB
    g = torch.Generator().manual_seed(21 + stride)
    B, Cin, Cout, eps = 2, 32, 128, 1e-3
    x = torch.randn(B, Cin, *hw, generator=g)
    w = torch.randn(Cout, Cin, 3, 3, generator=g) / (9 * Cin) ** 0.5
    bn = R.random_bn(Cout, g)
    wp, shift = NB.pack_conv3x3(w, list(bn) + [eps])
    assert wp.dtype == torch.uint16 and tuple(wp.shape) == (Cout, 2, 9 * Cin) and shift.dtype == torch.float32
    cols, Ho, Wo = R.im2col3x3(x, stride)
    assert (Ho, Wo) == NB.out_hw(*hw, stride)
    got = torch.relu(cols @ NB.unpack_pair(wp).T + shift.double())
    want = R.rows_of(R.conv_bn_relu(x, w, bn, eps, stride))
    bound = _weight_bound(wp, cols.abs().sum(1).max().item()) + 2.0 ** -24 * want.abs().max().item()  # + fp32 shift
    assert (got - want).abs().max().item() <= bound
    assert want.abs().max().item() > 1.0


@pytest.mark.parametrize("k,transposed", [(1, True), (1, False), (2, True), (4, True)])
def test_deblock_packing_matches_the_oracle(k, transposed):
    from projects.mmdet3d_plugin import native_bev as NB
    g = torch.Generator().manual_seed(31 + k)
    B, Cin, Cout, H, W, eps = 2, 32, 128, 5, 7, 1e-3
    x = torch.randn(B, Cin, H, W, generator=g)
    w = torch.randn((Cin, Cout, k, k) if transposed else (Cout, Cin, 1, 1), generator=g) / Cin ** 0.5
    bn = R.random_bn(Cout, g)
    wp, shift = NB.pack_deblock(w, list(bn) + [eps], k, transposed=transposed)
    assert tuple(wp.shape) == (k * k * Cout, 2, Cin)
    rows = R.rows_of(x).double()
    y = rows @ NB.unpack_pair(wp).T + shift.double().repeat(k * k)
    got = torch.relu(R.pixel_shuffle_rows(y, B, H, W, k, Cout))
    want = R.deblock_bn_relu(x, w, bn, eps, k, transposed=transposed)
    assert got.shape == want.shape == (B, Cout, k * H, k * W)
    bound = _weight_bound(wp, rows.abs().sum(1).max().item()) + 2.0 ** -24 * want.abs().max().item()
    assert (got - want).abs().max().item() <= bound
    with pytest.raises(ValueError):
        NB.pack_deblock(w, list(bn) + [eps], 2 if k != 2 else 4, transposed=transposed)


def test_packs_follow_in_place_updates():
    """PackCache: keyed on the conv weight and the four BN tensors"""
    b, n = _build()
    R.seed_module(b, 5), R.seed_module(n, 6)
    w0, s0 = b.packed(1, 0)
    assert b.packed(1, 0)[0] is w0
    with torch.no_grad():
        b.blocks[1][0].weight.mul_(2.0)
    w1, s1 = b.packed(1, 0)
    assert w1 is not w0 and not torch.equal(w1.view(torch.int16), w0.view(torch.int16)) and torch.equal(s0, s1)
    with torch.no_grad():
        b.blocks[1][1].running_var.add_(1.0)
    w2, s2 = b.packed(1, 0)
    assert w2 is not w1 and not torch.equal(s2, s1)
    d0 = n.packed(1)
    with torch.no_grad():
        n.deblocks[1][1].running_mean.add_(1.0)
    assert n.packed(1)[1] is not d0[1] and not torch.equal(n.packed(1)[1], d0[1])


@pytest.mark.parametrize("name", LIDAR_NAMES)
def test_reference_backbone_and_neck_build(name):
    if not os.path.isdir(REF_CONFIGS):
        pytest.skip("reference checkout not present")
    from projects.mmdet3d_plugin import build_backbone, build_neck
    from projects.mmdet3d_plugin.config import load_config
    model = load_config(os.path.join(REF_CONFIGS, name))["model"]
    # the cooperative configs hold one headless model per agent
    parts = [m for m in (model, model.get("vehicle_model"), model.get("infrastructure_model"))
             if isinstance(m, dict) and "pts_backbone" in m]
    assert parts
    for part in parts:
        b, n = build_backbone(part["pts_backbone"]), build_neck(part["pts_neck"])
        assert list(b.state_dict().keys()) == _backbone_keys()
        assert list(n.state_dict().keys()) == _neck_keys()
        assert sum(n.out_channels) == 512 and b.out_channels == n.in_channels and b.in_channels == 256
