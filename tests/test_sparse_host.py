"""The sparse-convolution C entry points and the SparseEncoder module without a device: exported
symbols and struct sizes, argument errors reported before any HIP call, the registry, the
state_dict's keys / shapes / both conv-weight layouts, and the refusals (host tensors,
block_type='conv_module')."""
import ctypes
import os

import pytest
import torch

from _sparse_ref import REF_ENCODER_CFG

REF_CONFIG = "/root/reference/projects/configs/CMT_Nuscenes/lidar/cmt_lidar_voxel0075_cbgs.py"
SYMBOLS = ("cmt_sparse_index", "cmt_sparse_index_bytes", "cmt_sparse_rulebook_subm", "cmt_sparse_rulebook_down",
           "cmt_sparse_conv", "cmt_sparse_pack_bytes", "cmt_sparse_to_dense")
STRUCTS = {"sparse_index": "SparseIndexArgs", "sparse_rulebook": "SparseRulebookArgs",
           "sparse_conv": "SparseConvArgs", "sparse_dense": "SparseDenseArgs"}


def _ptr():
    buf = ctypes.create_string_buffer(64)
    return buf, ctypes.addressof(buf)


def test_sparse_symbols_and_struct_sizes():
    from projects.mmdet3d_plugin import native
    L = native.lib()
    for s in SYMBOLS:
        assert hasattr(L, s), s
    for key, cls in STRUCTS.items():
        st = getattr(native, cls)
        assert native.STRUCTS[key] is st
        assert getattr(L, f"cmt_{key}_args_size")() == ctypes.sizeof(st), key
    assert L.cmt_abi_version() == native.ABI_VERSION == 25          # the new symbols are additive


def test_sparse_sizes():
    from projects.mmdet3d_plugin import native
    L = native.lib()
    # one bit per site + one running count per 32 sites + the rank table
    b = L.cmt_sparse_index_bytes(1, 41, 1440, 1440, 120000)
    sites = 41 * 1440 * 1440
    assert sites // 8 + sites // 8 + 4 * 120000 <= b <= sites // 4 + 4 * 120000 + (1 << 20)
    assert L.cmt_sparse_index_bytes(26, 41, 1440, 1440, 10) == 0       # >= 2^31 sites
    assert L.cmt_sparse_index_bytes(0, 41, 1440, 1440, 10) == 0
    assert L.cmt_sparse_pack_bytes(27, 5, 16) == 27 * 1 * 1 * 2 * 64 * 8 * 2      # Cin 5 -> 16, Cout 16 -> 32
    assert L.cmt_sparse_pack_bytes(27, 128, 128) == 27 * 8 * 4 * 2 * 64 * 8 * 2
    assert L.cmt_sparse_pack_bytes(3, 128, 128) == 3 * 8 * 4 * 2 * 64 * 8 * 2


def _index_args(native, grid=(2, 9, 16, 24)):
    buf, p = _ptr()
    a = native.SparseIndexArgs()
    a.B, a.D, a.H, a.W = grid
    a.n_cap, a.coors, a.count, a.index, a.index_bytes = 8, p, p, p, 0
    a._keep = buf
    return a


def _rulebook_args(native, grid=(2, 9, 16, 24), kernel=(3, 3, 3), stride=(2, 2, 2), padding=(1, 1, 1), K=27):
    buf, p = _ptr()
    a = native.SparseRulebookArgs()
    a.B, a.D, a.H, a.W = grid
    for i in range(3):
        a.kernel3[i], a.stride3[i], a.padding3[i] = kernel[i], stride[i], padding[i]
    a.K, a.n_cap, a.cap = K, 8, 8
    a.coors, a.count, a.index, a.index_bytes = p, p, p, 0
    a.out_index, a.out_index_bytes, a.out_coors, a.out_count, a.nbr = p, 0, p, p, p
    a._keep = buf
    return a


def _conv_args(native, Cin=16, Cout=16, K=27):
    buf, p = _ptr()
    L = native.lib()
    a = native.SparseConvArgs()
    a.cap, a.n_in_cap, a.Cin, a.Cout, a.K, a.relu = 8, 8, Cin, Cout, K, 1
    a.X, a.ldx, a.nbr, a.count = p, Cin, p, p
    a.Wp, a.wp_bytes = p, L.cmt_sparse_pack_bytes(K, Cin, min(Cout, 128))
    a.scale, a.shift, a.Y, a.ldy = p, p, p, Cout
    a._keep = buf
    return a


def test_sparse_argument_errors_before_any_launch():
    """Every refusal below is CMT_EINVAL (1001) with a message, on a machine with no device."""
    from projects.mmdet3d_plugin import native
    L = native.lib()
    err = L.cmt_last_error
    # a grid of >= 2^31 sites
    for fn, a in ((L.cmt_sparse_index, _index_args(native, (26, 41, 1440, 1440))),
                  (L.cmt_sparse_rulebook_subm, _rulebook_args(native, (26, 41, 1440, 1440), stride=(1, 1, 1))),
                  (L.cmt_sparse_rulebook_down, _rulebook_args(native, (26, 41, 1440, 1440)))):
        assert fn(ctypes.byref(a), None) == 1001
        assert b"2^31" in err()
    # Cout > 128
    a = _conv_args(native, Cout=129)
    assert L.cmt_sparse_conv(ctypes.byref(a), None) == 1001 and b"Cout" in err()
    a = _conv_args(native)
    a.wp_bytes -= 2
    assert L.cmt_sparse_conv(ctypes.byref(a), None) == 1001 and b"wp_bytes" in err()
    # K not matching kernel3
    for fn, kw in ((L.cmt_sparse_rulebook_subm, dict(stride=(1, 1, 1), K=9)), (L.cmt_sparse_rulebook_down, dict(K=3)),
                   (L.cmt_sparse_rulebook_down, dict(kernel=(3, 1, 1), stride=(2, 1, 1), padding=(0, 0, 0), K=27))):
        a = _rulebook_args(native, **kw)
        assert fn(ctypes.byref(a), None) == 1001
        assert b"kernel3" in err()
    # a submanifold rulebook is stride 1, padding k // 2
    a = _rulebook_args(native)
    assert L.cmt_sparse_rulebook_subm(ctypes.byref(a), None) == 1001 and b"stride3" in err()
    # null pointers
    for fn, mk, fields in ((L.cmt_sparse_index, _index_args, ("coors", "count", "index")),
                           (L.cmt_sparse_rulebook_down, _rulebook_args,
                            ("coors", "count", "index", "out_index", "out_coors", "out_count", "nbr")),
                           (L.cmt_sparse_conv, _conv_args, ("X", "nbr", "count", "Wp", "scale", "shift", "Y"))):
        assert fn(None, None) == 1001
        for f in fields:
            a = mk(native)
            setattr(a, f, None)
            assert fn(ctypes.byref(a), None) == 1001, f
            assert b"non-null" in err(), f
    d = native.SparseDenseArgs()
    assert L.cmt_sparse_to_dense(ctypes.byref(d), None) == 1001 and b"non-null" in err()
    assert L.cmt_sparse_to_dense(None, None) == 1001


def test_sparse_encoder_is_registered():
    import projects.mmdet3d_plugin as plugin
    from projects.mmdet3d_plugin.models.middle_encoders import SparseEncoder
    from projects.mmdet3d_plugin.registry import MIDDLE_ENCODERS, MODELS, build_middle_encoder
    assert "SparseEncoder" in MIDDLE_ENCODERS and MIDDLE_ENCODERS.get("SparseEncoder") is SparseEncoder
    assert MIDDLE_ENCODERS.parent is MODELS
    assert plugin.MIDDLE_ENCODERS is MIDDLE_ENCODERS and plugin.build_middle_encoder is build_middle_encoder


def _expected_keys(cfg):
    bn = ("weight", "bias", "running_mean", "running_var", "num_batches_tracked")
    keys = {"conv_input.0.weight", "conv_out.0.weight"}
    keys |= {f"conv_input.1.{b}" for b in bn} | {f"conv_out.1.{b}" for b in bn}
    chans = cfg["encoder_channels"]
    for i, blocks in enumerate(chans):
        for j in range(len(blocks)):
            p = f"encoder_layers.encoder_layer{i + 1}.{j}."
            if i != len(chans) - 1 and j == len(blocks) - 1:
                keys |= {p + "0.weight"} | {p + f"1.{b}" for b in bn}
            else:
                keys |= {p + "conv1.weight", p + "conv2.weight"} | {p + f"bn{n}.{b}" for n in (1, 2) for b in bn}
    return keys


def _check_built(enc, cfg):
    conv = (5 * 16 * 27 + 4 * 16 * 16 * 27 + 16 * 32 * 27 + 4 * 32 * 32 * 27 + 32 * 64 * 27 + 4 * 64 * 64 * 27
            + 64 * 128 * 27 + 4 * 128 * 128 * 27 + 128 * 128 * 3)
    bn_channels = 16 + 4 * 16 + 32 + 4 * 32 + 64 + 4 * 64 + 128 + 4 * 128 + 128
    assert sum(p.numel() for p in enc.parameters()) == conv + 2 * bn_channels
    sd = enc.state_dict()
    assert set(sd) == _expected_keys(cfg)
    assert tuple(sd["conv_input.0.weight"].shape) == (16, 3, 3, 3, 5)                       # (Cout, kD, kH, kW, Cin)
    assert tuple(sd["encoder_layers.encoder_layer1.2.0.weight"].shape) == (32, 3, 3, 3, 16)
    assert tuple(sd["encoder_layers.encoder_layer4.1.conv2.weight"].shape) == (128, 3, 3, 3, 128)
    assert tuple(sd["conv_out.0.weight"].shape) == (128, 3, 1, 1, 128)
    assert enc.conv_input[1].eps == 1e-3 and enc.conv_input[1].momentum == 0.01
    assert enc.encoder_layers.encoder_layer3[2][0].padding == (0, 1, 1)
    assert enc.output_shape() == (256, 180, 180)                                            # D: 41 -> 21 -> 11 -> 5 -> 2


def test_reference_config_middle_encoder_builds():
    if not os.path.isfile(REF_CONFIG):
        pytest.skip("reference checkout not present")
    from projects.mmdet3d_plugin import build_middle_encoder
    from projects.mmdet3d_plugin.config import load_config
    cfg = load_config(REF_CONFIG)["model"]["pts_middle_encoder"]
    assert cfg["type"] == "SparseEncoder"
    _check_built(build_middle_encoder(cfg), cfg)


def test_written_out_config_middle_encoder_builds():
    from projects.mmdet3d_plugin import build_middle_encoder
    _check_built(build_middle_encoder(REF_ENCODER_CFG), REF_ENCODER_CFG)


def _small(**kw):
    from projects.mmdet3d_plugin import build_middle_encoder
    cfg = dict(REF_ENCODER_CFG, sparse_shape=[41, 32, 32])
    cfg.update(kw)
    return build_middle_encoder(cfg)


def test_both_weight_layouts_load_to_equal_tensors():
    torch.manual_seed(3)
    src = _small()
    sd = src.state_dict()
    a, b = _small(), _small()
    a.load_state_dict(sd, strict=True)
    b.load_state_dict({k: (v.permute(1, 2, 3, 4, 0).contiguous() if v.dim() == 5 else v) for k, v in sd.items()},
                      strict=True)
    for k, v in sd.items():
        assert torch.equal(a.state_dict()[k], v), k
        assert torch.equal(b.state_dict()[k], v), k
        assert a.state_dict()[k].shape == b.state_dict()[k].shape == v.shape


def test_converted_agent_checkpoint_loads_strict():
    from projects.mmdet3d_plugin.checkpoint import convert_agent_checkpoint
    torch.manual_seed(4)
    src = _small()
    det = {"pts_middle_encoder." + k: v for k, v in src.state_dict().items()}
    det["pts_bbox_head.task_heads.0.x"] = torch.zeros(1)
    out = convert_agent_checkpoint(det, "vehicle")
    pre = "vehicle_model.pts_middle_encoder."
    sub = {k[len(pre):]: v for k, v in out.items() if k.startswith(pre)}
    assert tuple(sub["conv_input.0.weight"].shape) == (3, 3, 3, 5, 16)     # the converter's permuted layout
    dst = _small()
    res = dst.load_state_dict(sub, strict=True)
    assert not res.missing_keys and not res.unexpected_keys
    for k, v in src.state_dict().items():
        assert torch.equal(dst.state_dict()[k], v), k


def test_host_tensors_are_refused():
    enc = _small().eval()
    with pytest.raises(RuntimeError, match="HIP device"):
        enc(torch.zeros(4, 5), torch.zeros(4, 4, dtype=torch.int32), 1)
    from projects.mmdet3d_plugin import native_sparse as S
    with pytest.raises(RuntimeError, match="HIP device"):
        S.build_index(torch.zeros(4, 4, dtype=torch.int32), torch.zeros(1, dtype=torch.int32), (1, 4, 4, 4))
    with pytest.raises(RuntimeError, match="HIP device"):
        S.conv(torch.zeros(4, 16), torch.zeros(4, 27, dtype=torch.int32), torch.zeros(1, dtype=torch.int32),
               S.pack_weight(torch.zeros(16, 3, 3, 3, 16)), torch.zeros(16), torch.zeros(16), Cin=16, Cout=16)


def test_unbuilt_options_raise():
    from projects.mmdet3d_plugin import build_middle_encoder
    with pytest.raises(NotImplementedError):
        build_middle_encoder(dict(REF_ENCODER_CFG, block_type="conv_module"))
    with pytest.raises(NotImplementedError):
        build_middle_encoder(dict(type="SparseEncoder", in_channels=5, sparse_shape=[41, 32, 32]))   # the default
    with pytest.raises(NotImplementedError):
        build_middle_encoder(dict(REF_ENCODER_CFG, order=("conv", "act", "norm")))
    enc = _small().train()
    with pytest.raises(NotImplementedError):
        enc(torch.zeros(4, 5), torch.zeros(4, 4, dtype=torch.int32), 1)


def test_pack_weight_index_map():
    """pack_weight against the documented element map (cmt_hip.h), with hi + lo reproducing the weight to
    bf16-pair precision and zeros in the padding."""
    from projects.mmdet3d_plugin import native_sparse as S
    g = torch.Generator().manual_seed(5)
    w = torch.randn(40, 3, 1, 1, 5, generator=g)
    img = S.pack_weight(w)
    assert tuple(img.shape) == (3, 1, 2, 2, 64, 8) and img.dtype == torch.bfloat16
    assert img.numel() * 2 == 3 * 1 * 2 * 2 * 64 * 8 * 2
    f = img.float()
    for (k, nb, lane, j) in ((0, 0, 0, 0), (2, 1, 7, 4), (1, 0, 37, 3), (1, 1, 63, 7), (2, 1, 8, 0)):
        cin, cout = 8 * (lane >> 5) + j, 32 * nb + (lane & 31)
        want = w[cout, k, 0, 0, cin].item() if cin < 5 and cout < 40 else 0.0
        hi, lo = f[k, 0, nb, 0, lane, j].item(), f[k, 0, nb, 1, lane, j].item()
        assert hi == torch.tensor(want).bfloat16().item()
        assert abs(hi + lo - want) <= 2.0 ** -16 * abs(want)


# ---- the restatement's own helpers (tests/_sparse_ref.py), used by tests/test_gpu_sparse_edges.py ------------

def test_vectorised_restatement_matches_the_dictionary_one():
    """nbr_table against nbr_subm / nbr_down and down_coors against the dense mask, on the (2, 9, 16, 24)
    active set and every strided form; the figures the GPU tests rely on as preconditions."""
    import _sparse_ref as R
    shape, B = (9, 16, 24), 2
    grid = (B,) + shape
    coors = R.active_set(shape, B)[:300]
    assert coors.shape[0] == 300
    for kernel in (3, (1, 3, 3), (3, 1, 3), 1):
        assert torch.equal(R.nbr_table(coors, grid, kernel), R.nbr_subm(coors, kernel)), kernel
    _, mask = R.densify(torch.zeros(300, 1), coors, grid)
    outputs = {"k3s2p1": 503, "k3s2p011": 434, "k311s211p0": 349, "k3s2p0": 362, "k2s2p0": 195, "k3s3p0": 145,
               "k3s1p1": 3717, "k133s122p011": 442, "k3s2p2": 621, "k1s2p0": 45}
    outside = {"k3s2p0": 51, "k2s2p0": 39, "k3s3p0": 29, "k1s2p0": 255}
    forms = {**R.DOWN_FORMS, **R.MORE_FORMS}
    assert set(forms) == set(outputs)
    for name, (k, s, p) in forms.items():
        want = R.mask_coors(R.down_mask(mask, k, s, p))
        got = R.down_coors(coors, shape, k, s, p)
        assert got.dtype == torch.int32 and torch.equal(got, want), name
        assert want.shape[0] == outputs[name], name
        assert torch.equal(R.nbr_table(coors, grid, k, want, s, p), R.nbr_down(coors, want, k, s, p)), name
        assert R.rows_in_no_window(coors, want, k, s, p) == outside.get(name, 0), name
    # rows 200..299 are neighbours of earlier rows: dropping them changes 111 entries of the first 200 rows
    assert (R.nbr_subm(coors)[:200] != R.nbr_subm(coors[:200])).sum().item() == 111


def test_restatement_duplicates_resolve_to_the_lowest_row():
    import _sparse_ref as R
    grid = (2, 9, 16, 24)
    base = R.active_set(grid[1:], 2)[:300]
    pick = torch.arange(7, 300, 15)[:20]
    ref = R.nbr_subm(base)
    got = R.nbr_table(torch.cat([base, base[pick]]), grid)
    assert torch.equal(got[:300], ref) and torch.equal(got[300:], ref[pick])


def test_conv_rows_x3_is_the_three_pass_arithmetic():
    import _sparse_ref as R
    g = torch.Generator().manual_seed(8)
    x, w = torch.randn(50, 20, generator=g), torch.randn(33, 9, 1, 1, 20, generator=g)
    nbr = torch.randint(-1, 50, (40, 9), generator=g).to(torch.int32)
    want, got = R.conv_rows(x, nbr, w, relu=False), R.conv_rows_x3(x, nbr, w, relu=False)
    err = (got - want).abs().max().item()
    assert 0 < err <= 2.0 ** -15 * (9 * 20) ** 0.5 * 4               # not exact, well inside the kernels' bound
    # operands that are bf16 already have no lo part: the emulation is exact on them
    xb, wb = x.bfloat16().float(), w.bfloat16().float()
    assert torch.equal(R.conv_rows_x3(xb, nbr, wb, relu=False), R.conv_rows(xb, nbr, wb, relu=False))
    # the epilogue is conv_rows'
    sc, sh, res = 0.5 + torch.rand(33, generator=g), torch.randn(33, generator=g), torch.randn(40, 33, generator=g)
    full = R.conv_rows_x3(x, nbr, w, sc, sh, res)
    assert torch.equal(full, torch.relu(got * sc.double() + sh.double() + res.double()))


# ---- the wrappers refuse operands the kernels would index out of bounds, before the device check -------------

def _conv_call(**over):
    from projects.mmdet3d_plugin import native_sparse as S
    kw = dict(X=torch.zeros(4, 16), nbr=torch.zeros(6, 27, dtype=torch.int32), count=torch.zeros(1, dtype=torch.int32),
              Wp=S.pack_weight(torch.zeros(24, 3, 3, 3, 16)), scale=torch.zeros(24), shift=torch.zeros(24), R=None,
              out=None)
    kw.update(over)
    return S.conv(kw["X"], kw["nbr"], kw["count"], kw["Wp"], kw["scale"], kw["shift"], Cin=16, Cout=24, R=kw["R"],
                  out=kw["out"])


@pytest.mark.parametrize("name", ["out", "R"])
def test_conv_refuses_a_malformed_out_or_residual(name):
    for bad in (torch.zeros(6, 24, dtype=torch.float64), torch.zeros(6, 24, dtype=torch.bfloat16),
                torch.zeros(5, 24), torch.zeros(6, 23), torch.zeros(6, 48)[:, ::2], torch.zeros(24, 6).t(),
                torch.zeros(6 * 24)):
        with pytest.raises(ValueError, match=name):
            _conv_call(**{name: bad})
    for good in (torch.zeros(6, 24), torch.zeros(9, 40)[:, 3:27], torch.zeros(6, 24)[:, :24]):
        with pytest.raises(RuntimeError, match="HIP device"):          # well-formed: only the device is missing
            _conv_call(**{name: good})


@pytest.mark.parametrize("name", ["scale", "shift"])
def test_conv_refuses_a_malformed_scale_or_shift(name):
    for bad in (torch.zeros(23), torch.zeros(24, dtype=torch.float64), torch.zeros(48)[::2], torch.zeros(0)):
        with pytest.raises(ValueError, match=name):
            _conv_call(**{name: bad})
    with pytest.raises(RuntimeError, match="HIP device"):
        _conv_call(**{name: torch.zeros(32)})


def test_conv_refuses_a_malformed_rulebook_or_input():
    with pytest.raises(ValueError, match="nbr"):
        _conv_call(nbr=torch.zeros(6 * 27, dtype=torch.int32))
    with pytest.raises(ValueError, match="nbr"):
        _conv_call(nbr=torch.zeros(6, 2, 27, dtype=torch.int32))
    with pytest.raises(ValueError, match="nbr"):
        _conv_call(nbr=torch.zeros(6, 27, dtype=torch.int64))
    with pytest.raises(ValueError, match="no rows"):
        _conv_call(X=torch.zeros(0, 16))
    with pytest.raises(ValueError, match="X must"):
        _conv_call(X=torch.zeros(4, 15))
    with pytest.raises(RuntimeError, match="HIP device"):
        _conv_call()


def test_to_dense_refuses_a_malformed_input():
    from projects.mmdet3d_plugin import native_sparse as S
    coors, count = torch.zeros(6, 4, dtype=torch.int32), torch.zeros(1, dtype=torch.int32)
    for bad in (torch.zeros(6, 8, dtype=torch.float64), torch.zeros(6, 8, dtype=torch.float16), torch.zeros(5, 8),
                torch.zeros(6, 7), torch.zeros(6, 16)[:, ::2], torch.zeros(8, 6).t(), torch.zeros(48)):
        with pytest.raises(ValueError, match="X must"):
            S.to_dense(bad, coors, count, (1, 4, 4, 4), 8)
    with pytest.raises(ValueError, match="coors"):
        S.to_dense(torch.zeros(6, 8), coors.long(), count, (1, 4, 4, 4), 8)
    for good in (torch.zeros(6, 8), torch.zeros(9, 12)[:, 2:10]):
        with pytest.raises(RuntimeError, match="HIP device"):
            S.to_dense(good, coors, count, (1, 4, 4, 4), 8)
