"""Float64 restatement of the camera neck (CPFPN) on torch's CPU ops (conv2d, interpolate(mode='nearest',
size=...), batch_norm in eval mode, relu), the oracle of tests/test_fpn_host.py and tests/test_gpu_fpn.py.
The pair helpers and the seeded operands are those of tests/_bev_ref.py."""
import torch
import torch.nn.functional as F

from _bev_ref import bn_of, nchw_of, pair, random_bn, rows_of, seed_module, unpair  # noqa: F401


def conv_norm_act(x, w, bias, bn, eps, relu):
    """conv (1 x 1, or 3 x 3 / pad 1) -> BN in eval mode (``bn`` = (gamma, beta, mean, var) or None) -> ReLU,
    float64 NCHW"""
    y = F.conv2d(x.double(), w.double(), None if bias is None else bias.double(), 1, w.shape[-1] // 2)
    if bn is not None:
        gamma, beta, mean, var = (t.double() for t in bn)
        y = F.batch_norm(y, mean, var, gamma, beta, False, 0.0, eps)
    return torch.relu(y) if relu else y


def lateral_ref(x, w, bias, bn, eps, relu, top=None):
    """act(norm(conv1x1(x))) + the coarser float64 NCHW map ``top`` nearest-upsampled to x's size"""
    y = conv_norm_act(x, w, bias, bn, eps, relu)
    if top is not None:
        y = y + F.interpolate(top.double(), size=tuple(y.shape[2:]), mode="nearest")
    return y


def _parts(m):
    """(weight, bias, bn, eps, relu) of a conv module (conv, optional bn, optional activation), on the CPU"""
    bn = getattr(m, "bn", None)
    return (m.conv.weight.detach().cpu(), None if m.conv.bias is None else m.conv.bias.detach().cpu(),
            None if bn is None else [t.cpu() for t in bn_of(bn)], None if bn is None else bn.eps,
            hasattr(m, "activate"))


def cpfpn_ref(mod, xs):
    """CPFPN on the oracle: a list of ``num_outs`` float64 NCHW maps"""
    n = len(mod.lateral_convs)
    lat = [conv_norm_act(x.cpu(), *_parts(m)) for x, m in zip(xs[:n], mod.lateral_convs)]
    for i in range(n - 1, 0, -1):
        lat[i - 1] = lat[i - 1] + F.interpolate(lat[i], size=tuple(lat[i - 1].shape[2:]), mode="nearest")
    outs = [conv_norm_act(lat[0], *_parts(mod.fpn_convs[0]))] + lat[1:]
    while len(outs) < mod.num_outs:
        outs.append(F.max_pool2d(outs[-1], 1, stride=2))
    return outs


def seed_neck(mod, seed):
    """seed_module plus N(0, 0.5) conv biases, in place"""
    seed_module(mod, seed)
    g = torch.Generator().manual_seed(seed + 1000)
    with torch.no_grad():
        for m in mod.modules():
            if isinstance(m, torch.nn.Conv2d) and m.bias is not None:
                m.bias.copy_(0.5 * torch.randn(m.bias.shape, generator=g))
    return mod
