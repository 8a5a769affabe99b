"""cmt_img_augment, cmt_grid_mask and cmt_img_paste on the GPU against the numpy contracts of tests/_imgaug_ref.py.

Everything is integer resampling, exact weights and at most three float32 operations (or float64 products with a
truncation), so every comparison is bit for bit: there is no tolerance to choose.  Destinations lie between
sentinel guard regions that must stay intact, and are pre-filled so that an element that was not written shows.
"""
import numpy as np
import pytest
import torch

import _imgaug_ref as A
from projects.mmdet3d_plugin import native_img as NI
from projects.mmdet3d_plugin import native_imgaug as NIA
from projects.mmdet3d_plugin.models.utils.grid_mask import GridMask

pytestmark = pytest.mark.gpu

BGR = dict(mean=[103.530, 116.280, 123.675], std=[57.375, 57.120, 58.395])
TAIL = 64
HEAD = 4      # sentinels in front of the destination, a multiple of 4 so that ``offset`` alone sets the alignment
SENTINEL = -12345.5


def _frames(n, H, W, seed):
    return np.random.default_rng(seed).integers(0, 256, (n, H, W, 3), dtype=np.uint8)


def _guarded(dev, shape, offset=0):
    numel = int(np.prod(shape))
    lead = HEAD + offset
    buf = torch.full((lead + numel + TAIL,), float("nan"), dtype=torch.float32, device=dev)
    buf[lead + numel:] = SENTINEL
    buf[:lead] = SENTINEL
    return buf, buf[lead:lead + numel].view(*shape), lead, numel


def _check_guards(buf, lead, numel, shape):
    host = buf.cpu().numpy()
    assert np.all(host[lead + numel:] == SENTINEL), "sentinel tail overwritten"
    assert np.all(host[:lead] == SENTINEL), "elements before the destination overwritten"
    return host[lead:lead + numel].reshape(shape)


def _bit_equal(res, ref, what):
    bad = res.view(np.uint32) != ref.view(np.uint32)
    print(f"{what}: {int(bad.sum())} of {bad.size} elements differ")
    assert not bad.any(), f"{what}: not bit-equal to the contract at {np.argwhere(bad)[:4].tolist()}"


def _run_augment(dev, src, plans, *, size_divisor=32, size=None, offset=0, grid=None, zero=False, to_rgb=False):
    n = len(src)
    w, h = plans[0]["crop"][2] - plans[0]["crop"][0], plans[0]["crop"][3] - plans[0]["crop"][1]
    Hp, Wp = size if size is not None else (-(-h // size_divisor) * size_divisor, -(-w // size_divisor) * size_divisor)
    buf, out, lead, numel = _guarded(dev, (n, 3, Hp, Wp), offset)
    got = NIA.augment_images(torch.from_numpy(src).to(dev), plans, mean=BGR["mean"], std=BGR["std"], to_rgb=to_rgb,
                             size_divisor=size_divisor, size=size, grid_mask=grid, zero=zero, out=out)
    assert got.data_ptr() == out.data_ptr() and tuple(got.shape) == (n, 3, Hp, Wp)
    torch.cuda.synchronize()
    res = _check_guards(buf, lead, numel, (n, 3, Hp, Wp))
    assert not np.isnan(res).any(), "a destination element was not written"
    zeros = [bool(zero)] * n if isinstance(zero, bool) else list(zero)
    images = [dict(Hr=p["resize_dims"][1], Wr=p["resize_dims"][0], x0=p["crop"][0], y0=p["crop"][1], flip=p["flip"],
                   zero=z, iM=NIA.warp_inverse(w, h, p["rotate"])) for p, z in zip(plans, zeros)]
    ref = A.augment(src, images, w, h, Hp, Wp, BGR["mean"], BGR["std"], to_rgb, grid=grid)
    _bit_equal(res, ref, f"img_augment {src.shape} -> {(Hp, Wp)} offset {offset} grid {grid}")
    return res


def _plans(rotate=0.0, flip=False, w=40, h=16):
    """three frames of 23 x 37: one upscaled, one downscaled, one kept, each with its own window; the second frame
    has the opposite flip and the opposite angle"""
    specs = [((50, 31), (4, 9)), ((20, 13), (-11, -2)), ((37, 23), (-1, 5))]
    return [dict(resize_dims=d, crop=(x0, y0, x0 + w, y0 + h), flip=flip != (i == 1), rotate=-rotate if i == 1 else rotate)
            for i, (d, (x0, y0)) in enumerate(specs)]


SRC = _frames(3, 23, 37, 21)


@pytest.mark.parametrize("flip", [False, True])
@pytest.mark.parametrize("rotate", [0.0, 5.4, -90.0])
def test_img_augment_resize_crop_flip_rotate(dev, rotate, flip):
    """final_dim (16, 40) padded to 32 x 64, the vector-store path"""
    res = _run_augment(dev, SRC, _plans(rotate, flip))
    assert res.shape == (3, 3, 32, 64) and (res[:, :, 16:] == 0).all() and (res[:, :, :, 40:] == 0).all()


@pytest.mark.parametrize("size,offset", [((17, 41), 0), ((32, 64), 1)], ids=["odd_size", "offset_view"])
@pytest.mark.parametrize("rotate", [0.0, 5.4])
def test_img_augment_scalar_store_path(dev, size, offset, rotate):
    _run_augment(dev, SRC, _plans(rotate, True), size=size, offset=offset, to_rgb=True)


@pytest.mark.parametrize("mode", [0, 1])
@pytest.mark.parametrize("d,l,st_h,st_w", [(2, 1, 1, 0), (7, 4, 6, 3)])
def test_img_augment_grid_mask_and_modal_mask(dev, d, l, st_h, st_w, mode):
    """the mask covers the pad too; the second frame is zeroed (ModalMask3D)"""
    grid = dict(d=d, l=l, st_h=st_h, st_w=st_w, use_h=True, use_w=True, mode=mode)
    res = _run_augment(dev, SRC, _plans(5.4, False), grid=grid, zero=[False, True, False])
    m = A.grid_mask(32, 64, **grid)
    assert (res[:, :, m == 0] == 0).all() and np.signbit(res[:, :, m == 0]).any()
    black = (np.float32(0) - np.asarray(BGR["mean"], np.float32)) * (1.0 / np.asarray(BGR["std"], np.float32).astype(np.float64)).astype(np.float32)
    inside = np.zeros((32, 64), bool)
    inside[:16, :40] = True
    assert np.array_equal(res[1][:, inside & (m == 1)], np.repeat(black[:, None], (inside & (m == 1)).sum(), axis=1))
    _run_augment(dev, SRC, _plans(0.0, True), size=(17, 41), grid=dict(grid, use_h=False), zero=True)


def test_img_augment_source_one_pixel_wide(dev):
    src = _frames(2, 9, 1, 22)
    plans = [dict(resize_dims=(5, 12), crop=(-1, 1, 7, 7), flip=True, rotate=12.0),
             dict(resize_dims=(1, 9), crop=(-3, 0, 5, 6), flip=False, rotate=0.0)]
    _run_augment(dev, src, plans, size_divisor=4)
    _run_augment(dev, src, plans, size=(7, 9))


def test_img_augment_equals_prepare_images_without_augmentation(dev):
    """rotate = 0, no flip, no mask: the bytes of cmt_img_resize_prepare"""
    plan = dict(resize_dims=(30, 17), crop=(3, -2, 23, 10), flip=False, rotate=0.0)
    res = _run_augment(dev, SRC, [plan] * 3, size_divisor=8)
    plain = NI.prepare_images(torch.from_numpy(SRC).to(dev), crop=plan["crop"], mean=BGR["mean"], std=BGR["std"],
                              size_divisor=8, resize_dims=plan["resize_dims"])
    assert np.array_equal(plain.cpu().numpy().view(np.uint32), res.view(np.uint32))


def test_img_augment_more_than_one_block_per_image(dev):
    """64 x 132 outputs are 2112 groups per image: several workgroups and a grid-stride tail"""
    src = _frames(2, 40, 57, 23)
    plans = [dict(resize_dims=(140, 80), crop=(3, 7, 133, 69), flip=True, rotate=-3.3),
             dict(resize_dims=(120, 70), crop=(-5, 2, 125, 64), flip=False, rotate=2.1)]
    _run_augment(dev, src, plans, size=(64, 132))


# ---- cmt_grid_mask -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape,offset", [((2, 3, 19, 30), 0), ((2, 3, 20, 32), 0), ((2, 3, 20, 32), 1)],
                         ids=["scalar", "vector", "offset_view"])
def test_grid_mask_in_place(dev, shape, offset):
    x = np.random.default_rng(31).standard_normal(shape).astype(np.float32)
    for grid in (dict(d=7, l=4, st_h=6, st_w=3, use_h=True, use_w=True, mode=1),
                 dict(d=2, l=1, st_h=0, st_w=1, use_h=False, use_w=True, mode=0)):
        buf, view, lead, numel = _guarded(dev, shape, offset)
        view.copy_(torch.from_numpy(x).to(dev))
        assert NIA.grid_mask_(view, grid).data_ptr() == view.data_ptr()
        torch.cuda.synchronize()
        res = _check_guards(buf, lead, numel, shape)
        want = x * A.grid_mask(shape[2], shape[3], **grid)[None, None]
        _bit_equal(res, want, f"grid_mask {shape} offset {offset} {grid}")


def test_grid_mask_module(dev):
    """training: the draws of the reference in its order; eval and rand() > prob return the input untouched"""
    gm = GridMask(True, True, rotate=1, offset=False, ratio=0.5, mode=1, prob=0.7)
    x = np.random.default_rng(32).standard_normal((2, 3, 19, 30)).astype(np.float32)
    seed = next(s for s in range(100) if np.random.RandomState(s).rand() <= 0.7)
    rs = np.random.RandomState(seed)
    rs.rand()
    d = rs.randint(2, 19)
    grid = dict(d=d, l=min(max(int(d * 0.5 + 0.5), 1), d - 1), st_h=rs.randint(d), st_w=rs.randint(d), use_h=True,
                use_w=True, mode=1)
    rs.randint(1)
    t = torch.from_numpy(x).to(dev)
    gm.train()
    np.random.seed(seed)
    out = gm(t)
    assert out.data_ptr() == t.data_ptr() and gm.l == grid["l"]
    assert np.random.rand() == rs.rand()   # the same number of draws consumed
    _bit_equal(out.cpu().numpy(), x * A.grid_mask(19, 30, **grid)[None, None], f"GridMask module {grid}")
    fresh = torch.from_numpy(x).to(dev)
    gm.eval()
    assert gm(fresh) is fresh
    gm.train()
    skip = next(s for s in range(100) if np.random.RandomState(s).rand() > 0.7)
    np.random.seed(skip)
    assert gm(fresh) is fresh
    assert np.array_equal(fresh.cpu().numpy(), x)


# ---- cmt_img_paste -----------------------------------------------------------------------------------------------
GUARD = 96


def _run_paste(dev, frames, plan, patches, m):
    flat = torch.full((GUARD + frames.size + GUARD,), 0xA5, dtype=torch.uint8, device=dev)
    view = flat[GUARD:GUARD + frames.size].view(*frames.shape)
    view.copy_(torch.from_numpy(frames).to(dev))
    got = NIA.paste_images(view, plan, patches, mixup_rate=m)
    assert got.data_ptr() == view.data_ptr()
    torch.cuda.synchronize()
    host = flat.cpu().numpy()
    assert (host[:GUARD] == 0xA5).all() and (host[GUARD + frames.size:] == 0xA5).all(), "guard bytes overwritten"
    res = host[GUARD:GUARD + frames.size].reshape(frames.shape)
    ref = A.paste(frames, plan, patches, m)
    bad = (res != ref).any(axis=-1)
    print(f"img_paste {frames.shape} m={m}: {int(bad.sum())} of {bad.size} pixels differ")
    assert not bad.any(), f"not equal to the contract at {np.argwhere(bad)[:4].tolist()}"
    return res


def _patches(seed):
    rng = np.random.default_rng(seed)
    return [rng.integers(0, 256, (7, 5, 3), dtype=np.uint8), rng.integers(0, 256, (1, 1, 3), dtype=np.uint8),
            np.zeros((0, 0, 3), np.uint8), rng.integers(0, 256, (31, 50, 3), dtype=np.uint8),
            rng.integers(0, 256, (2, 1, 3), dtype=np.uint8)]


@pytest.mark.parametrize("m", [-1, 0.5, 0.3])
def test_img_paste(dev, m):
    """[2, 29, 45, 3]: overlapping raw and sampled rectangles in list order, rectangles on every frame edge, a 1 x 1
    patch, an empty patch, an empty rectangle; the second camera has an empty list and stays untouched"""
    frames = _frames(2, 29, 45, 41)
    plan = [np.array([[0, 0, 12, 9, 0],        # the top-left corner, upscaled patch
                      [5, 4, 30, 20, -1],      # a raw box over it
                      [8, 6, 21, 29, 3],       # down to the bottom edge, downscaled patch, over the raw box
                      [33, 0, 45, 29, 1],      # the right edge, top to bottom, from a 1 x 1 patch
                      [0, 20, 9, 29, 2],       # an empty patch: skipped
                      [40, 25, 45, 29, -1],    # the bottom-right corner, raw, over a sampled box
                      [17, 10, 17, 15, 0],     # an empty rectangle
                      [0, 11, 3, 18, 4],       # the left edge, from a patch one pixel wide
                      [10, 2, 11, 3, 3]], np.int32),
            np.zeros((0, 5), np.int32)]
    res = _run_paste(dev, frames, plan, _patches(42), m)
    assert np.array_equal(res[1], frames[1])
    untouched = np.ones((29, 45), bool)
    for x0, y0, x1, y1, crop in plan[0].tolist():
        if crop != 2:
            untouched[y0:y1, x0:x1] = False
    assert untouched.sum() > 100 and np.array_equal(res[0][untouched], frames[0][untouched])
    assert not np.array_equal(res[0], frames[0])


def test_img_paste_both_cameras_and_the_rectangle_limit(dev):
    """two lists with different bounding rectangles; 256 rectangles pass, 257 are refused before any launch"""
    frames = _frames(2, 29, 45, 43)
    rng = np.random.default_rng(44)
    many = []
    for i in range(256):
        x0, y0 = int(rng.integers(0, 40)), int(rng.integers(3, 25))
        many.append([x0, y0, x0 + int(rng.integers(1, 6)), y0 + int(rng.integers(1, 5)), int(rng.integers(-1, 2))])
    plan = [np.array(many, np.int32), np.array([[30, 20, 44, 28, 3], [2, 2, 4, 4, -1]], np.int32)]
    res = _run_paste(dev, frames, plan, _patches(45), 0.3)
    assert np.array_equal(res[0][:3], frames[0][:3]) and np.array_equal(res[1][:2], frames[1][:2])
    over = [np.array(many + [[0, 0, 2, 2, -1]], np.int32), plan[1]]
    view = torch.from_numpy(frames).to(dev)
    with pytest.raises(ValueError, match="257"):
        NIA.paste_images(view, over, _patches(45), mixup_rate=0.3)
    torch.cuda.synchronize()
    assert np.array_equal(view.cpu().numpy(), frames)
