"""SECOND: the reference's ``pts_backbone`` (``pts_backbone=dict(type='SECOND', ...)`` in every LiDAR
and fusion config) on the native conv kernels (csrc/bev.hip, csrc/gemm.hip), inference only.

The semantics are mmdet3d 1.0.0rc6's ``SECOND``, restated (mmdet3d is not a dependency):
``blocks[i] = Sequential(conv(in_i, out_i, 3, stride=layer_strides[i], padding=1), BN, ReLU, then
layer_nums[i] x [conv(out_i, out_i, 3, padding=1), BN, ReLU])``, flat, ``in_i = out_{i-1}``; forward
returns every stage's output.  Convs are bias-free, BN uses its running statistics and is folded into
the packed weights (float64 fold, then the split-f16 pair).

Routing.  The stride-1 convs run on ``cmt_gemm``: the first conv of stage 0 straight from the fp32
NCHW map (CMT_A_CONV3X3_NCHW), the others on pair rows (CMT_A_CONV3X3).  Strided convs run on
``cmt_bev_conv3x3``; a strided stage-0 conv reads the map through ``nchw_to_rows``.

state_dict keys: ``blocks.{i}.{3j}.weight`` (Cout, Cin, 3, 3) and ``blocks.{i}.{3j+1}.{weight, bias,
running_mean, running_var, num_batches_tracked}``.  ``blocks.0.0.weight`` is pinned by the checkpoint
tests; the others are restated from mmdet3d, not checked against a real checkpoint here.
"""
import torch
import torch.nn as nn

from ... import native_bev as NB
from ...native import _dev
from ...registry import BACKBONES
from ..utils.packing import PackCache

__all__ = ["SECOND"]


def bn_eps_momentum(who, norm_cfg):
    if norm_cfg.get("type") not in ("BN", "BN2d"):
        raise NotImplementedError(f"{who} norm_cfg type {norm_cfg.get('type')!r}: only 'BN' / 'BN2d' is built")
    return norm_cfg.get("eps", 1e-5), norm_cfg.get("momentum", 0.1)


def no_bias_conv(who, cfg, types):
    if cfg.get("type") not in types:
        raise NotImplementedError(f"{who} layer type {cfg.get('type')!r}: only {' / '.join(types)} is built")
    if cfg.get("bias", False):
        raise NotImplementedError(f"{who}: biased convolutions have no native path (every reference config "
                                  "sets bias=False)")


def bn_tensors(bn):
    return [bn.weight, bn.bias, bn.running_mean, bn.running_var]


def inference_only(module):
    if module.training and torch.is_grad_enabled():
        raise NotImplementedError(f"{type(module).__name__} is inference only: call .eval() or run under "
                                  "torch.no_grad()")


class RangeFlagMixin:
    """One int32 device word the module's kernels OR 1 into when an operand leaves the f16-pair range."""

    def _range_flag(self, dev):
        f = self.__dict__.get("_range_flag_t")
        if f is None or f.device != dev:
            f = torch.zeros(1, dtype=torch.int32, device=dev)
            self.__dict__["_range_flag_t"] = f
        return f

    def check_input_range(self):
        """Raise ValueError if a forward since the last call met a value outside the f16-pair operand
        range (non-finite or |x| >= 65520), and clear the flag.  One 4-byte device read."""
        f = self.__dict__.get("_range_flag_t")
        if f is None:
            return
        if int(f.item()):
            f.zero_()
            raise ValueError(f"{type(self).__name__}: a feature-map value fell outside the f16 operand range "
                             "(non-finite or |x| >= 65520); the outputs of that forward are not valid")


@BACKBONES.register_module()
class SECOND(nn.Module, RangeFlagMixin):
    def __init__(self, in_channels=128, out_channels=[128, 128, 256], layer_nums=[3, 5, 5], layer_strides=[2, 2, 2],
                 norm_cfg=dict(type="BN", eps=1e-3, momentum=0.01), conv_cfg=dict(type="Conv2d", bias=False),
                 init_cfg=None, pretrained=None):
        super().__init__()
        if not (len(out_channels) == len(layer_nums) == len(layer_strides)):
            raise ValueError("out_channels, layer_nums and layer_strides differ in length")
        eps, mom = bn_eps_momentum("SECOND", norm_cfg)
        no_bias_conv("SECOND conv_cfg", conv_cfg, ("Conv2d",))
        for s in layer_strides:
            if s not in (1, 2):
                raise NotImplementedError(f"SECOND layer_strides {list(layer_strides)}: only strides 1 and 2 are built")
        for c in out_channels:
            if c <= 0 or c % 128:
                raise NotImplementedError(f"SECOND out_channels {list(out_channels)}: the conv kernels need "
                                          "multiples of 128")
        need = 16 if layer_strides[0] == 1 else 32
        if in_channels <= 0 or in_channels % need:
            raise NotImplementedError(f"SECOND in_channels {in_channels}: a stride-{layer_strides[0]} first conv "
                                      f"needs a multiple of {need}")
        self.in_channels, self.out_channels = int(in_channels), [int(c) for c in out_channels]
        self.layer_nums, self.layer_strides = [int(n) for n in layer_nums], [int(s) for s in layer_strides]
        blocks = []
        prev = self.in_channels
        for c, n, s in zip(self.out_channels, self.layer_nums, self.layer_strides):
            layers = [nn.Conv2d(prev, c, 3, stride=s, padding=1, bias=False),
                      nn.BatchNorm2d(c, eps=eps, momentum=mom), nn.ReLU(inplace=True)]
            for _ in range(n):
                layers += [nn.Conv2d(c, c, 3, padding=1, bias=False), nn.BatchNorm2d(c, eps=eps, momentum=mom),
                           nn.ReLU(inplace=True)]
            blocks.append(nn.Sequential(*layers))
            prev = c
        self.blocks = nn.ModuleList(blocks)
        self._pack = PackCache()

    def packed(self, i, j):
        """(pair rows [Cout, 2, 9 Cin], shift [Cout]) of conv ``j`` of stage ``i``, repacked when the conv
        weight or one of the four BN tensors changes"""
        conv, bn = self.blocks[i][3 * j], self.blocks[i][3 * j + 1]
        return self._pack.get((i, j), [conv.weight] + bn_tensors(bn), bn.eps,
                              lambda: NB.pack_conv3x3(conv.weight, bn_tensors(bn) + [bn.eps]))

    def forward(self, x):
        """fp32 NCHW [B, in_channels, H, W] -> a tuple of RowMap, one per stage"""
        inference_only(self)
        if not torch.is_tensor(x) or x.dim() != 4 or x.shape[1] != self.in_channels:
            raise ValueError(f"SECOND takes a [B, {self.in_channels}, H, W] map, got "
                             f"{tuple(x.shape) if torch.is_tensor(x) else type(x)}")
        B, _, H, W = (int(s) for s in x.shape)
        if W > NB.WMAX:
            raise NotImplementedError(f"SECOND: map width {W} above {NB.WMAX}, the conv kernels' limit")
        _dev(x, self.blocks[0][0].weight)
        outs = []
        with torch.no_grad():
            flag = self._range_flag(x.device)
            x = x.float().contiguous()
            rows, C = None, self.in_channels
            for i, (c, n, s) in enumerate(zip(self.out_channels, self.layer_nums, self.layer_strides)):
                wp, shift = self.packed(i, 0)
                if rows is None and s == 1:
                    rows = NB.conv3x3_nchw_gemm(x, wp, shift, Cout=c, range_flag=flag)
                else:
                    if rows is None:
                        rows = NB.to_rows(x, range_flag=flag).rows
                    if s == 1:
                        rows = NB.conv3x3_gemm(rows, wp, shift, B=B, H=H, W=W, Cin=C, Cout=c, range_flag=flag)
                    else:
                        rows = NB.conv3x3(rows, wp, shift, B=B, H=H, W=W, Cin=C, Cout=c, stride=s, range_flag=flag)
                        H, W = NB.out_hw(H, W, s)
                for j in range(1, n + 1):
                    wp, shift = self.packed(i, j)
                    rows = NB.conv3x3_gemm(rows, wp, shift, B=B, H=H, W=W, Cin=c, Cout=c, range_flag=flag)
                C = c
                outs.append(NB.RowMap(rows, (B, c, H, W)))
        return tuple(outs)
