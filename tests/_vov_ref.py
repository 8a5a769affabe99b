"""Float64 restatement of the image backbone (VoVNet-eSE) on torch's CPU ops (conv2d, batch_norm in eval
mode, relu, max_pool2d(ceil_mode=True), mean, hardtanh), the oracle of tests/test_vov_host.py and
tests/test_gpu_vov.py, and the seeding they share.  The forward is written from the semantics (stem of
three conv-BN-ReLU with strides 2, 1, 2; four stages of OSA blocks, a ceil-mode 3 x 3 / stride 2 pool
before every stage but the first; per block a chain of 3 x 3 convs, the 1 x 1 aggregation of the block's
input and every layer's output, the eSE gate in every block, the identity add after the gate in every
block but a stage's first) and works on a state dict alone, so it does not depend on the module under test.
The pair helpers and random_bn are those of tests/_bev_ref.py."""
import zlib
from collections import OrderedDict

import torch
import torch.nn.functional as F

from _bev_ref import (bn_relu, conv_bn_relu, im2col3x3, nchw_of, pair, pair_rounded, random_bn, rows_of,  # noqa: F401
                      unpair)

NAMES = ("stem", "stage2", "stage3", "stage4", "stage5")
# spec -> (layer_per_block, block_per_stage)
SHAPE = {"V-19-eSE": (3, (1, 1, 1, 1)), "V-39-eSE": (5, (1, 1, 2, 2)), "V-57-eSE": (5, (1, 1, 4, 3)),
         "V-99-eSE": (5, (1, 3, 9, 3))}
BN_EPS = 1e-5
BN_NAMES = ("weight", "bias", "running_mean", "running_var")


def key_generator(seed, key):
    return torch.Generator().manual_seed(seed * 1_000_003 + zlib.crc32(key.encode()))


def seed_by_key(mod, seed):
    """Seed every state-dict tensor of ``mod`` by its key, in place, independent of registration order: conv
    and fc weights N(0, 1) / sqrt(fan_in); the four tensors of a BN from random_bn on the generator of the BN's
    ``weight`` key; fc.bias N(0, 1).  num_batches_tracked stays."""
    sd = mod.state_dict()
    with torch.no_grad():
        for key, t in sd.items():
            g = key_generator(seed, key)
            if key.endswith("/conv.weight") or key.endswith("fc.weight"):
                fan = t.shape[1] * t.shape[2] * t.shape[3]
                t.copy_(torch.randn(t.shape, generator=g) / fan ** 0.5)
            elif key.endswith("/norm.weight"):
                for n, v in zip(BN_NAMES, random_bn(t.numel(), g)):
                    sd[key[:-len("weight")] + n].copy_(v)
            elif key.endswith("fc.bias"):
                t.copy_(torch.randn(t.shape, generator=g))
    return mod


def seeded_image(seed, shape):
    return torch.randn(shape, generator=torch.Generator().manual_seed(seed))


def hsigmoid(t):
    return F.hardtanh(t + 3.0, 0.0, 6.0) / 6.0


def ese_gate_ref(x, fc_w, fc_b):
    """float64 NCHW x -> the gate [B, C, 1, 1]"""
    return hsigmoid(F.conv2d(x.double().mean((2, 3), keepdim=True), fc_w.double(), fc_b.double()))


def vovnet_ref(sd, spec_name, x, out_features=NAMES):
    """VoVNet-eSE on the oracle from a state dict: an ordered dict name -> float64 NCHW map"""
    sd = {k: v.detach().cpu().double() for k, v in sd.items() if v.is_floating_point()}
    lpb, blocks = SHAPE[spec_name]

    def cbr(x, prefix, stride):
        w = sd[prefix + "/conv.weight"]
        y = F.conv2d(x, w, None, stride, w.shape[-1] // 2)
        return bn_relu(y, [sd[f"{prefix}/norm.{n}"] for n in BN_NAMES], BN_EPS)

    outs = OrderedDict()
    x = x.cpu().double()
    for i, stride in enumerate((2, 1, 2)):
        x = cbr(x, f"stem.stem_{i + 1}", stride)
    if "stem" in out_features:
        outs["stem"] = x
    for i, name in enumerate(NAMES[1:]):
        if i > 0:
            x = F.max_pool2d(x, 3, 2, ceil_mode=True)
        for k in range(blocks[i]):
            blk = f"OSA{i + 2}_{k + 1}"
            p = f"{name}.{blk}"
            feats, cur = [x], x
            for j in range(lpb):
                cur = cbr(cur, f"{p}.layers.{j}.{blk}_{j}", 1)
                feats.append(cur)
            y = cbr(torch.cat(feats, 1), f"{p}.concat.{blk}_concat", 1)
            y = y * ese_gate_ref(y, sd[f"{p}.ese.fc.weight"], sd[f"{p}.ese.fc.bias"])
            x = y + x if k > 0 else y
        if name in out_features:
            outs[name] = x
    return outs
