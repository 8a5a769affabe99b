"""cmt_img_prepare on the GPU against a numpy restatement: crop, normalise, pad and HWC -> CHW in one pass.

The windows below are (x0, y0, w, h) in source pixels, the kernel's own form; ``prepare_images`` takes the
reference's (x0, y0, x1, y1).  Every case pre-fills the destination with NaN, keeps a sentinel tail behind it
and asserts

  1. the sentinel tail is untouched;
  2. the result equals, bit for bit, the float32 two-step form ``(x.astype(f32) - mean32) * inv32`` with
     ``inv32 = float32(1 / float64(float32(std)))``, zeros in the pad and ``(0 - mean32) * inv32`` where the
     window leaves the source;
  3. it is within 1e-6 absolute of the float64 ``(x - mean32) / std32``.  Two fp32 roundings and the
     reciprocal's rounding are at most about 3 ulp, one ulp is 2.4e-7 at the largest |value| 2.64; over all
     256 x 3 inputs of the configs' constants the two-step form is within 1.74e-7.
"""
import numpy as np
import pytest
import torch

from projects.mmdet3d_plugin import native_img as NI

pytestmark = pytest.mark.gpu

BGR = dict(mean=[103.530, 116.280, 123.675], std=[57.375, 57.120, 58.395])
RGB = dict(mean=[123.675, 116.28, 103.53], std=[58.395, 57.12, 57.375])
TAIL = 64
SENTINEL = -12345.5


def _reference(src, win, Hp, Wp, mean, std, to_rgb):
    """(float32 two-step form, float64 form) of the contract, in numpy"""
    x0, y0, w, h = win
    n, Hs, Ws, _ = src.shape
    crop = np.zeros((n, h, w, 3), np.uint8)   # the reference pastes the crop into zeros
    ys, xs = np.arange(y0, y0 + h), np.arange(x0, x0 + w)
    yi, xi = (ys >= 0) & (ys < Hs), (xs >= 0) & (xs < Ws)
    crop[:, np.ix_(yi, xi)[0], np.ix_(yi, xi)[1]] = src[:, ys[yi]][:, :, xs[xi]]
    if to_rgb:
        crop = crop[..., ::-1]
    mean32, std32 = np.asarray(mean, np.float32), np.asarray(std, np.float32)
    inv32 = (1.0 / std32.astype(np.float64)).astype(np.float32)
    f32 = (crop.astype(np.float32) - mean32) * inv32
    f64 = (crop.astype(np.float64) - mean32.astype(np.float64)) / std32.astype(np.float64)
    assert f32.dtype == np.float32
    out32 = np.zeros((n, 3, Hp, Wp), np.float32)
    out64 = np.zeros((n, 3, Hp, Wp), np.float64)
    out32[:, :, :h, :w] = f32.transpose(0, 3, 1, 2)
    out64[:, :, :h, :w] = f64.transpose(0, 3, 1, 2)
    return out32, out64


def _run_and_check(dev, src, win, *, consts=BGR, to_rgb=False, size_divisor=32, size=None, offset=0):
    x0, y0, w, h = win
    n = src.shape[0]
    if size is not None:
        Hp, Wp = size
    else:
        Hp, Wp = -(-h // size_divisor) * size_divisor, -(-w // size_divisor) * size_divisor
    numel = n * 3 * Hp * Wp
    buf = torch.full((offset + numel + TAIL,), float("nan"), dtype=torch.float32, device=dev)
    buf[offset + numel:] = SENTINEL
    if offset:
        buf[:offset] = SENTINEL
    out = buf[offset:offset + numel].view(n, 3, Hp, Wp)
    frames = torch.from_numpy(src).to(dev)
    got = NI.prepare_images(frames, crop=(x0, y0, x0 + w, y0 + h), mean=consts["mean"], std=consts["std"],
                            to_rgb=to_rgb, size_divisor=size_divisor, size=size, out=out)
    assert got.data_ptr() == out.data_ptr() and tuple(got.shape) == (n, 3, Hp, Wp)
    torch.cuda.synchronize()
    host = buf.cpu().numpy()
    assert np.all(host[offset + numel:] == SENTINEL), "sentinel tail overwritten"
    assert np.all(host[:offset] == SENTINEL), "elements before the destination overwritten"
    res = host[offset:offset + numel].reshape(n, 3, Hp, Wp)
    ref32, ref64 = _reference(src, win, Hp, Wp, consts["mean"], consts["std"], to_rgb)
    assert not np.isnan(res).any(), "a destination element was not written"
    assert np.array_equal(res.view(np.uint32), ref32.view(np.uint32)), \
        f"not bit-equal to the float32 form: max abs diff {np.abs(res - ref32).max():.3e}"
    err = np.abs(res.astype(np.float64) - ref64).max()
    print(f"imgprep {src.shape} win {win} -> {(Hp, Wp)} rgb={to_rgb}: max abs err vs float64 {err:.3e} (bound 1e-6)")
    assert err <= 1e-6
    return res


def _frames(n, H, W, seed):
    return np.random.default_rng(seed).integers(0, 256, (n, H, W, 3), dtype=np.uint8)


def test_all_bytes(dev):
    """a 16 x 16 frame holds every byte value in every channel (another order per channel and image)"""
    src = np.empty((2, 16, 16, 3), np.uint8)
    for n in range(2):
        for c in range(3):
            src[n, :, :, c] = np.roll(np.arange(256, dtype=np.uint8), 37 * c + 101 * n).reshape(16, 16)
    for k in range(3):
        assert np.array_equal(np.sort(src[0, :, :, k].ravel()), np.arange(256))
    _run_and_check(dev, src, (0, 0, 16, 16), size_divisor=1)


def test_small_window(dev):
    """9 x 14 source, window (3, 2, 7, 5), divisor 4 -> 8 x 8: row start at byte 9, one pad column, 3 pad rows"""
    res = _run_and_check(dev, _frames(2, 9, 14, 1), (3, 2, 7, 5), size_divisor=4)
    assert res.shape == (2, 3, 8, 8)
    assert np.all(res[:, :, 5:, :] == 0) and np.all(res[:, :, :, 7:] == 0)


@pytest.mark.parametrize("w", [37, 1])
def test_width_tails(dev, w):
    _run_and_check(dev, _frames(2, 5, 41, 2 + w), (2, 1, w, 3))


@pytest.mark.parametrize("to_rgb", [False, True])
def test_outside_the_source(dev, to_rgb):
    """window (-2, -1, 12, 9) on a 6 x 7 source: the source is missing on all four sides"""
    consts = RGB if to_rgb else BGR
    res = _run_and_check(dev, _frames(2, 6, 7, 3), (-2, -1, 12, 9), consts=consts, to_rgb=to_rgb)
    mean32, std32 = np.asarray(consts["mean"], np.float32), np.asarray(consts["std"], np.float32)
    outside = (np.float32(0) - mean32) * (1.0 / std32.astype(np.float64)).astype(np.float32)
    assert np.array_equal(res[0, :, 0, 0], outside) and np.array_equal(res[1, :, 8, 11], outside)


@pytest.mark.parametrize("to_rgb", [False, True])
@pytest.mark.parametrize("consts", [BGR, RGB], ids=["bgr_constants", "rgb_constants"])
def test_colour_order(dev, to_rgb, consts):
    _run_and_check(dev, _frames(2, 9, 14, 4), (3, 2, 7, 5), consts=consts, to_rgb=to_rgb, size_divisor=4)


@pytest.mark.parametrize("size,offset", [((7, 11), 0), ((6, 10), 0), ((8, 12), 1), ((5, 9), 3)])
def test_odd_destination(dev, size, offset):
    """Wp no multiple of 4, or a destination that is not 16-byte aligned: the scalar store path"""
    _run_and_check(dev, _frames(2, 9, 14, 5), (3, 2, 7, 5), size=size, offset=offset)


def test_more_than_one_block_unaligned_rows(dev):
    """3 * Ws = 1497 and 3 * x0 = 15: source row starts at every byte phase, several workgroups, grid stride"""
    _run_and_check(dev, _frames(2, 70, 499, 6), (5, 3, 488, 64))


def test_full_size(dev):
    """the configs' frame: [6, 900, 1600, 3] -> [6, 3, 640, 1600], rows 260..900"""
    resize, crop = NI.test_crop((900, 1600), (640, 1600))
    assert resize == 1.0 and crop == (0, 260, 1600, 900)
    src = _frames(6, 900, 1600, 7)
    res = _run_and_check(dev, src, (crop[0], crop[1], crop[2] - crop[0], crop[3] - crop[1]))
    assert res.shape == (6, 3, 640, 1600)


def test_defaults_cover_the_whole_frame(dev):
    src = _frames(2, 32, 64, 8)
    got = NI.prepare_images(torch.from_numpy(src).to(dev))
    ref32, _ = _reference(src, (0, 0, 64, 32), 32, 64, BGR["mean"], BGR["std"], False)
    assert got.dtype == torch.float32 and np.array_equal(got.cpu().numpy().view(np.uint32), ref32.view(np.uint32))
