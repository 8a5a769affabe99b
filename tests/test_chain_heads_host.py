"""Host-side pieces of the task heads' first conv inside chain B2 (cmt_chain_args.Wh): the padded
head pack and native.chain's argument rules.  No device needed."""
import pytest
import torch

from projects.mmdet3d_plugin import native
from projects.mmdet3d_plugin.models.utils.packing import to_dtype

SPLIT = torch.uint16


def _unpack(pack, G):
    """Fragment-major pack -> row-major [256 G, 256] by the index formula of cmt_hip.h
    (cmt_chain_args.Wn): W[256g + 64w + 32nt + r][32kc + 16ks + 8h + e] at
    ((((((g*4 + w)*8 + kc)*2 + ks)*2 + nt)*2 + h)*32 + r)*8 + e."""
    n = torch.arange(256 * G).view(-1, 1)
    k = torch.arange(256).view(1, -1)
    g, w, nt, r = n // 256, n // 64 % 4, n // 32 % 2, n % 32
    kc, ks, h, e = k // 32, k // 16 % 2, k // 8 % 2, k % 8
    at = ((((((g * 4 + w) * 8 + kc) * 2 + ks) * 2 + nt) * 2 + h) * 32 + r) * 8 + e
    return pack[at]


@pytest.mark.parametrize("cols", [384, 64, 512])
def test_head_pack_round_trips(cols):
    """pack_chain_heads = pack_chain_pair of the weight zero-padded to whole 256-row blocks: hi pack,
    then lo pack, each the padded row count x 256 long; unpacked, the original rows and zeros."""
    g = torch.Generator().manual_seed(cols)
    Wp = to_dtype(torch.randn(cols, 256, generator=g) / 16, SPLIT)          # [cols, 2, 256]
    pack = native.pack_chain_heads(Wp)
    G = -(-cols // 256)
    assert pack.dtype == SPLIT and pack.shape == (2 * G * 256 * 256,)
    halves = pack.view(torch.int16).view(2, -1)
    src = Wp.view(torch.int16)
    for half in range(2):
        W = _unpack(halves[half], G)
        assert torch.equal(W[:cols], src[:, half])
        assert (W[cols:] == 0).all()
    if cols % 256 == 0:
        assert torch.equal(pack.view(torch.int16), native.pack_chain_pair(Wp).view(torch.int16))


def test_head_pack_refuses_other_shapes():
    with pytest.raises(RuntimeError, match="pack_chain_heads"):
        native.pack_chain_heads(torch.zeros(100, 2, 256, dtype=SPLIT))      # not a multiple of 64
    with pytest.raises(RuntimeError, match="pack_chain_heads"):
        native.pack_chain_heads(torch.zeros(128, 2, 128, dtype=SPLIT))
    with pytest.raises(RuntimeError, match="pack_chain_heads"):
        native.pack_chain_heads(torch.zeros(128, 256, dtype=torch.float16))


def _call(kind=2, flags=native.LN_NAN_TO_NUM, head_cols=384, pack_cols=None, H1="ok", rows=40):
    Wh = native.pack_chain_heads(torch.zeros(pack_cols or 384, 2, 256, dtype=SPLIT))
    H1 = torch.zeros(rows, head_cols) if H1 == "ok" else H1
    prm = torch.zeros(native.CHAIN_PRM[kind])
    Y = torch.zeros(rows, 256)
    native.chain(kind, None, None, prm, None, None, Y, rows=rows, Nq=rows, eps=1e-5, OUT=torch.zeros(rows, 256),
                 out_flags=flags, WS=torch.zeros(native.chain_ws_numel(rows)), Wh=Wh, H1=H1, head_cols=head_cols)


def test_chain_refuses_bad_head_arguments():
    """The rules of cmt_chain_x3 mirrored in native.chain, raised before any device work (the tensors
    here live on the host; a well-formed call gets as far as the no-CPU-fallback check)."""
    with pytest.raises(RuntimeError, match="LN_MAX_INTO"):
        _call(flags=native.LN_NAN_TO_NUM | native.LN_MAX_INTO)
    for kind in (0, 1):
        with pytest.raises(RuntimeError, match="kind 2"):
            _call(kind=kind)
    for cols in (100, 0, 1088):
        with pytest.raises(RuntimeError, match="multiple of 64"):
            _call(head_cols=cols)
    with pytest.raises(RuntimeError, match="pack_chain_heads"):
        _call(head_cols=768)                                    # a 512-row pack under 768 columns
    with pytest.raises(RuntimeError, match="H1"):
        _call(H1=None)
    with pytest.raises(RuntimeError, match="H1"):
        _call(H1=torch.zeros(40, 384, dtype=torch.float64))
    with pytest.raises(RuntimeError, match="go with Wh"):
        native.chain(2, None, None, torch.zeros(3840), None, None, torch.zeros(40, 256), rows=40, Nq=40, eps=1e-5,
                     OUT=torch.zeros(40, 256), WS=torch.zeros(native.chain_ws_numel(40)), head_cols=384)
    with pytest.raises(RuntimeError, match="HIP device"):
        _call()


def test_option_defaults_on_and_overrides():
    from projects.mmdet3d_plugin.runtime import OPTIONS, options
    import os
    assert OPTIONS.chain_heads == (os.environ.get("CMT_CHAIN_HEADS", "1") != "0")
    with options(chain_heads=False):
        assert OPTIONS.chain_heads is False
