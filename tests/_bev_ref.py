"""Float64 restatement of the dense BEV backbone / neck on torch's CPU ops (conv2d, conv_transpose2d,
batch_norm in eval mode, relu), the oracle of tests/test_bev_host.py and tests/test_gpu_bev.py, and the
seeded operands they share."""
import torch
import torch.nn.functional as F

SPLIT = torch.uint16


def pair(x):
    """fp32 [..., C] -> [..., 2, C] uint16: hi = f16(x), lo = f16(x - hi)"""
    hi = x.float().half()
    lo = (x.float() - hi.float()).half()
    return torch.stack([hi, lo], -2).contiguous().view(SPLIT)


def unpair(p):
    """[..., 2, C] uint16 -> float64 [..., C]"""
    v = p.cpu().view(torch.float16).double()
    return v[..., 0, :] + v[..., 1, :]


def pair_rounded(x):
    """the value the pair format carries for fp32 x, as float64"""
    return unpair(pair(x))


def rows_of(x):
    """NCHW -> NHWC rows [B*H*W, C]"""
    return x.permute(0, 2, 3, 1).reshape(-1, x.shape[1]).contiguous()


def nchw_of(rows, B, H, W):
    return rows.reshape(B, H, W, -1).permute(0, 3, 1, 2).contiguous()


def random_bn(C, g):
    """(gamma, beta, running_mean, running_var) with var in [0.5, 2]"""
    return (0.5 + torch.rand(C, generator=g), 0.5 * torch.randn(C, generator=g), 0.5 * torch.randn(C, generator=g),
            0.5 + 1.5 * torch.rand(C, generator=g))


def bn_relu(y, bn, eps, relu=True):
    gamma, beta, mean, var = (t.double() for t in bn)
    y = F.batch_norm(y, mean, var, gamma, beta, False, 0.0, eps)
    return torch.relu(y) if relu else y


def conv_bn_relu(x, w, bn, eps, stride=1, relu=True):
    """conv3x3 / pad 1 -> BN (eval) -> ReLU, float64 NCHW"""
    return bn_relu(F.conv2d(x.double(), w.double(), None, stride, 1), bn, eps, relu)


def deblock_bn_relu(x, w, bn, eps, k, transposed=True, relu=True):
    """ConvTranspose2d(k, stride k) (weight (Cin, Cout, k, k)) or the 1 x 1 Conv2d (weight (Cout, Cin, 1, 1))"""
    if transposed:
        y = F.conv_transpose2d(x.double(), w.double(), None, k)
    else:
        y = F.conv2d(x.double(), w.double())
    return bn_relu(y, bn, eps, relu)


def im2col3x3(x, stride):
    """float64 NCHW -> tap-major rows [B*Ho*Wo, 9 C] with K = (ky*3 + kx) * C + c: independent of F.unfold's
    channel-major order, written with explicit shifts"""
    B, C, H, W = x.shape
    Ho, Wo = (H - 1) // stride + 1, (W - 1) // stride + 1
    xp = F.pad(x.double(), (1, 1, 1, 1))
    taps = []
    for ky in range(3):
        for kx in range(3):
            t = xp[:, :, ky:ky + stride * (Ho - 1) + 1:stride, kx:kx + stride * (Wo - 1) + 1:stride]
            taps.append(t.permute(0, 2, 3, 1).reshape(B * Ho * Wo, C))
    return torch.cat(taps, 1), Ho, Wo


def pixel_shuffle_rows(y, B, H, W, k, Cout):
    """GEMM output rows [B*H*W, (dy, dx, n)] -> NCHW [B, Cout, k H, k W]"""
    y = y.reshape(B, H, W, k, k, Cout).permute(0, 5, 1, 3, 2, 4)
    return y.reshape(B, Cout, k * H, k * W)


def bn_of(m):
    return [m.weight.detach(), m.bias.detach(), m.running_mean.detach(), m.running_var.detach()]


def seed_module(mod, seed):
    """seeded conv weights (N(0, 1) / sqrt(fan_in)) and random BN statistics, in place"""
    g = torch.Generator().manual_seed(seed)
    with torch.no_grad():
        for m in mod.modules():
            if isinstance(m, (torch.nn.Conv2d, torch.nn.ConvTranspose2d)):
                fan = m.in_channels * (9 if m.kernel_size == (3, 3) else 1)
                m.weight.copy_(torch.randn(m.weight.shape, generator=g) / fan ** 0.5)
            elif isinstance(m, torch.nn.BatchNorm2d):
                for t, v in zip((m.weight, m.bias, m.running_mean, m.running_var), random_bn(m.num_features, g)):
                    t.copy_(v)
    return mod


def second_ref(mod, x):
    """SECOND on the oracle: a list of float64 NCHW maps, one per stage"""
    outs = []
    x = x.double()
    for blk in mod.blocks:
        for j in range(0, len(blk), 3):
            x = conv_bn_relu(x, blk[j].weight.detach().cpu(), [t.cpu() for t in bn_of(blk[j + 1])], blk[j + 1].eps,
                             blk[j].stride[0])
        outs.append(x)
    return outs


def fpn_ref(mod, xs):
    """SECONDFPN on the oracle: float64 [B, sum(out), H, W]"""
    ys = []
    for blk, x, k in zip(mod.deblocks, xs, mod.upsample_strides):
        ys.append(deblock_bn_relu(x, blk[0].weight.detach().cpu(), [t.cpu() for t in bn_of(blk[1])], blk[1].eps, k,
                                  transposed=isinstance(blk[0], torch.nn.ConvTranspose2d)))
    return torch.cat(ys, 1)
