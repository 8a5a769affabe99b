"""cmt_img_resize_prepare on the GPU against the numpy contract of tests/_resize_ref.py: 8-bit fixed-point bilinear
resize, window, normalise, pad and HWC -> CHW in one launch.

Windows are (x0, y0, w, h) in pixels of the resized image, the kernel's own form; ``prepare_images`` takes
(x0, y0, x1, y1).  Every case pre-fills the destination with NaN, keeps sentinels before and after it and asserts
that the sentinels are intact, that no NaN is left and that the result equals the reference bit for bit (integer
resampling and two float32 operations: there is no tolerance to choose).
"""
import importlib.util
import json
import os

import numpy as np
import pytest
import torch

import _resize_ref as R
from conftest import PKG
from projects.mmdet3d_plugin import native_img as NI

pytestmark = pytest.mark.gpu

BGR = dict(mean=[103.530, 116.280, 123.675], std=[57.375, 57.120, 58.395])
RGB = dict(mean=[123.675, 116.28, 103.53], std=[58.395, 57.12, 57.375])
TAIL = 64
HEAD = 4      # sentinels in front of the destination, a multiple of 4 so that ``offset`` alone sets the alignment
SENTINEL = -12345.5


def _run_and_check(dev, src, dims, win=None, *, consts=BGR, to_rgb=False, size_divisor=32, size=None, offset=0):
    """``dims`` = (Wr, Hr); ``win`` None: the whole resized image.  Returns the result as numpy."""
    Wr, Hr = dims
    x0, y0, w, h = win if win is not None else (0, 0, Wr, Hr)
    n = src.shape[0]
    if size is not None:
        Hp, Wp = size
    else:
        Hp, Wp = -(-h // size_divisor) * size_divisor, -(-w // size_divisor) * size_divisor
    numel = n * 3 * Hp * Wp
    lead = HEAD + offset
    buf = torch.full((lead + numel + TAIL,), float("nan"), dtype=torch.float32, device=dev)
    buf[lead + numel:] = SENTINEL
    buf[:lead] = SENTINEL
    out = buf[lead:lead + numel].view(n, 3, Hp, Wp)
    frames = torch.from_numpy(src).to(dev)
    got = NI.prepare_images(frames, crop=None if win is None else (x0, y0, x0 + w, y0 + h), mean=consts["mean"],
                            std=consts["std"], to_rgb=to_rgb, size_divisor=size_divisor, size=size, out=out,
                            resize_dims=dims)
    assert got.data_ptr() == out.data_ptr() and tuple(got.shape) == (n, 3, Hp, Wp)
    torch.cuda.synchronize()
    host = buf.cpu().numpy()
    assert np.all(host[lead + numel:] == SENTINEL), "sentinel tail overwritten"
    assert np.all(host[:lead] == SENTINEL), "elements before the destination overwritten"
    res = host[lead:lead + numel].reshape(n, 3, Hp, Wp)
    ref = R.reference(src, dims, (x0, y0, w, h), Hp, Wp, consts["mean"], consts["std"], to_rgb)
    assert not np.isnan(res).any(), "a destination element was not written"
    bad = res.view(np.uint32) != ref.view(np.uint32)
    print(f"imgresize {src.shape} -> {(Hr, Wr)} win {(x0, y0, w, h)} -> {(Hp, Wp)} rgb={to_rgb}: "
          f"{int(bad.sum())} of {bad.size} elements differ, max abs diff {np.abs(res - ref).max():.3e}")
    assert not bad.any(), f"not bit-equal to the contract at {np.argwhere(bad)[:4].tolist()}"
    return res


def _frames(n, H, W, seed):
    return np.random.default_rng(seed).integers(0, 256, (n, H, W, 3), dtype=np.uint8)


def _all_bytes():
    src = np.empty((2, 16, 16, 3), np.uint8)
    for n in range(2):
        for c in range(3):
            src[n, :, :, c] = np.roll(np.arange(256, dtype=np.uint8), 37 * c + 101 * n).reshape(16, 16)
    return src


@pytest.mark.parametrize("win", [(3, 2, 7, 5), (-2, -1, 12, 9), None], ids=["inside", "partly_outside", "whole"])
def test_identity_equals_prepare_images(dev, win):
    """resize_dims equal to the source size: the resize reproduces the source, so the call equals cmt_img_prepare"""
    src = _frames(2, 9, 14, 1)
    res = _run_and_check(dev, src, (14, 9), win, size_divisor=4)
    crop = None if win is None else (win[0], win[1], win[0] + win[2], win[1] + win[3])
    plain = NI.prepare_images(torch.from_numpy(src).to(dev), crop=crop, size_divisor=4)
    assert np.array_equal(plain.cpu().numpy().view(np.uint32), res.view(np.uint32))


def test_all_bytes_upscaled(dev):
    """the 16 x 16 frame with every byte value in every channel, to 23 x 29"""
    _run_and_check(dev, _all_bytes(), (29, 23), size_divisor=1)


def test_tumtraf_ratios(dev):
    """48 x 72 -> 36 x 60 is the TUMTraf frame's 1.3333 and 1.2, window rows 10..36, divisor 32"""
    res = _run_and_check(dev, _frames(2, 48, 72, 2), (60, 36), (0, 10, 60, 26))
    assert res.shape == (2, 3, 32, 64) and np.all(res[:, :, 26:] == 0) and np.all(res[:, :, :, 60:] == 0)


def test_exact_half(dev):
    src = _frames(2, 36, 64, 3)
    res = _run_and_check(dev, src, (32, 18), size_divisor=1)
    s = src.astype(np.int64)
    mean4 = ((s[:, 0::2, 0::2] + s[:, 0::2, 1::2] + s[:, 1::2, 0::2] + s[:, 1::2, 1::2] + 2) >> 2).astype(np.uint8)
    want = R.normalise_pad(mean4, 18, 32, BGR["mean"], BGR["std"], False)
    assert np.array_equal(res.view(np.uint32), want.view(np.uint32))


def test_downscale_3p7(dev):
    _run_and_check(dev, _frames(2, 37, 74, 4), (20, 10), size_divisor=4)


def test_upscale_2p5_border_clamps(dev):
    """9 x 14 -> 22 x 35: the first and last two resized columns and rows lie beyond the outer pixel centres"""
    _run_and_check(dev, _frames(2, 9, 14, 5), (35, 22), size_divisor=1)


@pytest.mark.parametrize("to_rgb", [False, True])
@pytest.mark.parametrize("consts", [BGR, RGB], ids=["bgr_constants", "rgb_constants"])
def test_window_leaves_the_resized_image(dev, to_rgb, consts):
    """6 x 7 -> 8 x 10, window (-2, -1, 14, 11): the resized image is missing on all four sides"""
    res = _run_and_check(dev, _frames(2, 6, 7, 6), (10, 8), (-2, -1, 14, 11), consts=consts, to_rgb=to_rgb)
    mean32, std32 = np.asarray(consts["mean"], np.float32), np.asarray(consts["std"], np.float32)
    outside = (np.float32(0) - mean32) * (1.0 / std32.astype(np.float64)).astype(np.float32)
    assert np.array_equal(res[0, :, 0, 0], outside) and np.array_equal(res[1, :, 10, 13], outside)


def test_window_misses_the_resized_image(dev):
    _run_and_check(dev, _frames(1, 6, 7, 7), (10, 8), (40, 30, 5, 3), size_divisor=4)
    _run_and_check(dev, _frames(1, 6, 7, 7), (10, 8), (-40, -30, 5, 3), size_divisor=4)


@pytest.mark.parametrize("w", [37, 1])
def test_width_tails(dev, w):
    _run_and_check(dev, _frames(2, 5, 41, 8 + w), (47, 7), (2, 1, w, 3))


@pytest.mark.parametrize("size,offset", [((7, 11), 0), ((6, 10), 0), ((8, 12), 1), ((5, 9), 3)])
def test_odd_destination(dev, size, offset):
    """Wp no multiple of 4, or a destination that is not 16-byte aligned: the scalar store path"""
    _run_and_check(dev, _frames(2, 9, 14, 9), (11, 8), (3, 2, 7, 5), size=size, offset=offset)


@pytest.mark.parametrize("hs,ws,dims", [(7, 1, (5, 9)), (1, 9, (13, 4)), (6, 11, (1, 8)), (1, 1, (6, 5))],
                         ids=["Ws1", "Hs1", "Wr1", "one_pixel"])
def test_degenerate_sources(dev, hs, ws, dims):
    for seed in (10, 11):
        _run_and_check(dev, _frames(2, hs, ws, seed), dims, size_divisor=1)
        _run_and_check(dev, _frames(2, hs, ws, seed), dims, size_divisor=4)


def test_more_than_one_block_odd_row_bytes(dev):
    """N = 3, 3 * Ws = 1497: tap pairs at every byte phase, 3 * 64 * 104 groups in several workgroups"""
    _run_and_check(dev, _frames(3, 70, 499, 12), (413, 61), (0, 0, 413, 61))


def test_full_size_tumtraf_frame(dev):
    """[1, 1200, 1920, 3] resized to 1600 x 900, rows 260..900 -> [1, 3, 640, 1600], the plan of the TUMTraf configs"""
    resize, dims, crop = NI.resize_crop_plan((900, 1600), (640, 1600))
    assert (resize, dims, crop) == (1.0, (1600, 900), (0, 260, 1600, 900))
    res = _run_and_check(dev, _frames(1, 1200, 1920, 13), dims, (crop[0], crop[1], crop[2] - crop[0], crop[3] - crop[1]))
    assert res.shape == (1, 3, 640, 1600)


def test_cli_detector_ida_size(dev, tmp_path):
    """tools/test.py --detector --ida-size in this process: 150 x 384 frames are resized to 320 x 188, rows 60..188.
    32 queries of the 7 TUMTraf classes are 224 candidates, fewer than the coder's default max_num = 300 (which the
    decode kernel rejects, as torch.topk would), hence the bbox_coder.max_num option."""
    assert NI.resize_crop_plan((188, 320), (128, 320)) == (1.0, (320, 188), (0, 60, 320, 188))
    spec = importlib.util.spec_from_file_location("cmt_test_cli_ida", os.path.join(PKG, "tools", "test.py"))
    cli = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(cli)
    out = tmp_path / "f.json"
    rc = cli.main(["cmtcoop_fusion_tumtraf", "--synthetic", "--detector", "--num-query", "32", "--num-layers", "1",
                   "--grid", "32", "32", "--frame-size", "150", "384", "--ida-size", "188", "320", "--points", "1000",
                   "--cfg-options", "bbox_coder.max_num=200", "--out", str(out)])
    assert rc == 0
    data = json.loads(out.read_text())
    assert data["config"] == "cmtcoop_fusion_tumtraf" and len(data["frames"]) == 1
    fr = data["frames"][0]
    n = len(fr["scores_3d"])
    assert n > 0 and len(fr["boxes_3d"]) == n == len(fr["labels_3d"]) and len(fr["boxes_3d"][0]) == 9
    assert np.isfinite(np.asarray(fr["boxes_3d"])).all() and np.isfinite(np.asarray(fr["scores_3d"])).all()
