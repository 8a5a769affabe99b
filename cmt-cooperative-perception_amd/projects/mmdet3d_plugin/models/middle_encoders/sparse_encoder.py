"""SparseEncoder: the reference's ``pts_middle_encoder`` (models/detectors/cmt.py:78-86,
``pts_middle_encoder=dict(type='SparseEncoder', ...)`` in every LiDAR and fusion config) on the
native sparse convolution kernels (csrc/sparse.hip), inference only.

The semantics are mmdet3d 1.0.0rc6's ``SparseEncoder`` on spconv 2.1.21, restated (neither
library is a dependency):

* ``conv_input``: SubMConv3d(in_channels -> base_channels, 3, padding 1) + BN1d + ReLU;
* stage ``i`` of ``encoder_channels``, entry ``(j, c)``: the last entry of every stage but the last
  is SparseConv3d(prev -> c, 3, stride 2, padding ``encoder_paddings[i][j]``) + BN1d + ReLU, every
  other entry a SparseBasicBlock(c): subm conv1 -> bn1 -> ReLU -> subm conv2 -> bn2 -> + identity
  -> ReLU;
* ``conv_out``: SparseConv3d(last -> output_channels, (3,1,1), stride (2,1,1), padding 0) + BN1d +
  ReLU; then ``.dense()`` [B, C, D', H', W'] viewed as [B, C * D', H', W'].

All convolutions are bias-free, BN uses its running statistics.  Only ``block_type='basicblock'``
with ``order=('conv', 'norm', 'act')`` -- what every reference config uses -- has a native path.

state_dict keys.  ``conv_input.0.weight`` / ``conv_input.1.*`` are pinned by the checkpoint tests;
the others are restated from mmdet3d, not checked against a real checkpoint here:
``encoder_layers.encoder_layer{i+1}.{j}.{conv1.weight,bn1.*,conv2.weight,bn2.*}`` for basic blocks,
``encoder_layers.encoder_layer{i+1}.{j}.0.weight`` / ``....{j}.1.*`` for strided modules,
``conv_out.0.weight`` / ``conv_out.1.*``.  Conv weights are held as (Cout, kD, kH, kW, Cin), spconv
2's layout; ``load_state_dict`` also takes (kD, kH, kW, Cin, Cout), which
``convert_agent_checkpoint`` writes for cooperative checkpoints (kD <= 3 < 16 <= Cout, so the two
cannot be confused).
"""
import math

import torch
import torch.nn as nn

from ... import native_sparse as S
from ...native import _dev
from ...registry import MIDDLE_ENCODERS
from ..utils.packing import PackCache

__all__ = ["SparseEncoder", "SparseBasicBlock", "SparseConv"]


class SparseConv(nn.Module):
    """The weight of one sparse convolution, (Cout, kD, kH, kW, Cin), and its geometry."""

    def __init__(self, in_channels, out_channels, kernel, stride=1, padding=0, subm=False):
        super().__init__()
        self.in_channels, self.out_channels = int(in_channels), int(out_channels)
        self.kernel, self.stride, self.padding = S.triple(kernel), S.triple(stride), S.triple(padding)
        self.subm = bool(subm)
        self.weight = nn.Parameter(torch.empty(self.out_channels, *self.kernel, self.in_channels))
        nn.init.kaiming_uniform_(self.weight.view(self.out_channels, -1), a=math.sqrt(5))
        self._pack = PackCache()

    def _load_from_state_dict(self, state_dict, prefix, *args, **kwargs):
        key = prefix + "weight"
        w = state_dict.get(key)
        other = (*self.kernel, self.in_channels, self.out_channels)
        if torch.is_tensor(w) and tuple(w.shape) == other and other != tuple(self.weight.shape):
            state_dict[key] = w.permute(4, 0, 1, 2, 3)
        super()._load_from_state_dict(state_dict, prefix, *args, **kwargs)

    def packed(self):
        return self._pack.get("w", [self.weight], None, lambda: S.pack_weight(self.weight))

    def extra_repr(self):
        return (f"{self.in_channels}, {self.out_channels}, kernel={self.kernel}, stride={self.stride}, "
                f"padding={self.padding}, subm={self.subm}")


def _folded_bn(cache, bn):
    """BN1d in eval mode as (scale, shift) fp32: y = scale * x + shift"""
    def build():
        var, mean = bn.running_var.double(), bn.running_mean.double()
        scale = bn.weight.double() / torch.sqrt(var + bn.eps)
        shift = bn.bias.double() - mean * scale
        return scale.float().contiguous(), shift.float().contiguous()
    return cache.get("bn", [bn.weight, bn.bias, bn.running_mean, bn.running_var], bn.eps, build)


class _ConvBN(nn.Sequential):
    """SparseSequential(conv, BN1d, ReLU): keys ``0.weight`` and ``1.*``"""

    def __init__(self, conv, eps, momentum):
        super().__init__(conv, nn.BatchNorm1d(conv.out_channels, eps=eps, momentum=momentum), nn.ReLU(inplace=True))
        self._bn_cache = PackCache()

    def run(self, x, nbr, count):
        scale, shift = _folded_bn(self._bn_cache, self[1])
        return S.conv(x, nbr, count, self[0].packed(), scale, shift, Cin=self[0].in_channels,
                      Cout=self[0].out_channels, relu=True)


class SparseBasicBlock(nn.Module):
    """subm conv1 -> bn1 -> ReLU -> subm conv2 -> bn2 -> + identity -> ReLU"""

    def __init__(self, channels, eps, momentum):
        super().__init__()
        self.conv1 = SparseConv(channels, channels, 3, 1, 1, subm=True)
        self.bn1 = nn.BatchNorm1d(channels, eps=eps, momentum=momentum)
        self.conv2 = SparseConv(channels, channels, 3, 1, 1, subm=True)
        self.bn2 = nn.BatchNorm1d(channels, eps=eps, momentum=momentum)
        self._c1, self._c2 = PackCache(), PackCache()

    def run(self, x, nbr, count):
        c = self.conv1.out_channels
        s1, b1 = _folded_bn(self._c1, self.bn1)
        s2, b2 = _folded_bn(self._c2, self.bn2)
        h = S.conv(x, nbr, count, self.conv1.packed(), s1, b1, Cin=c, Cout=c, relu=True)
        return S.conv(h, nbr, count, self.conv2.packed(), s2, b2, Cin=c, Cout=c, relu=True, R=x)


@MIDDLE_ENCODERS.register_module()
class SparseEncoder(nn.Module):
    """``capacity_factor``: a strided stage may hold up to ``ceil(capacity_factor * rows entering it)``
    output rows.  The default 1 fits LiDAR-like clouds, whose strided stages shrink the active set;
    isolated points can grow it, by up to 8 outputs per input."""

    def __init__(self, in_channels, sparse_shape, order=("conv", "norm", "act"),
                 norm_cfg=dict(type="BN1d", eps=1e-3, momentum=0.01), base_channels=16, output_channels=128,
                 encoder_channels=((16,), (32, 32, 32), (64, 64, 64), (64, 64, 64)),
                 encoder_paddings=((1,), (1, 1, 1), (1, 1, 1), ((0, 1, 1), 1, 1)), block_type="conv_module",
                 capacity_factor=1.0):
        super().__init__()
        if block_type != "basicblock":
            raise NotImplementedError(f"SparseEncoder block_type={block_type!r}: only 'basicblock' (every reference "
                                      "config) has a native path")
        if tuple(order) != ("conv", "norm", "act"):
            raise NotImplementedError(f"SparseEncoder order={tuple(order)!r}: only ('conv', 'norm', 'act') is built")
        if norm_cfg.get("type") != "BN1d":
            raise NotImplementedError(f"SparseEncoder norm_cfg type {norm_cfg.get('type')!r}: only 'BN1d' is built")
        if len(encoder_channels) != len(encoder_paddings):
            raise ValueError("encoder_channels and encoder_paddings differ in length")
        eps, mom = norm_cfg.get("eps", 1e-5), norm_cfg.get("momentum", 0.1)
        self.in_channels, self.sparse_shape = int(in_channels), tuple(int(s) for s in sparse_shape)
        self.base_channels, self.output_channels = int(base_channels), int(output_channels)
        self.encoder_channels, self.encoder_paddings = encoder_channels, encoder_paddings
        self.stage_num = len(encoder_channels)
        self.capacity_factor = float(capacity_factor)
        self.conv_input = _ConvBN(SparseConv(in_channels, base_channels, 3, 1, 1, subm=True), eps, mom)
        self.encoder_layers = nn.Sequential()
        prev = self.base_channels
        for i, blocks in enumerate(encoder_channels):
            stage = []
            for j, c in enumerate(blocks):
                if i != self.stage_num - 1 and j == len(blocks) - 1:
                    stage.append(_ConvBN(SparseConv(prev, c, 3, 2, encoder_paddings[i][j]), eps, mom))
                else:
                    if c != prev:
                        raise ValueError(f"basic block {i}.{j}: {c} channels after {prev} (an identity shortcut "
                                         "needs equal widths)")
                    stage.append(SparseBasicBlock(c, eps, mom))
                prev = c
            self.encoder_layers.add_module(f"encoder_layer{i + 1}", nn.Sequential(*stage))
        self.conv_out = _ConvBN(SparseConv(prev, output_channels, (3, 1, 1), (2, 1, 1), 0), eps, mom)

    def output_shape(self):
        """(C * D', H', W') of the dense map"""
        shape = self.sparse_shape
        for m in self._strided():
            shape = S.out_shape(shape, m[0].kernel, m[0].stride, m[0].padding)
        return (self.output_channels * shape[0], shape[1], shape[2])

    def _strided(self):
        return [m for stage in self.encoder_layers for m in stage if isinstance(m, _ConvBN)] + [self.conv_out]

    def _down(self, name, unit, x, coors, count, index, grid):
        conv = unit[0]
        n = int(coors.shape[0])
        cap = max(int(math.ceil(self.capacity_factor * n)), 1)
        oc, ocount, nbr, oindex, ogrid = S.rulebook_down(coors, count, index, grid, conv.kernel, conv.stride,
                                                         conv.padding, cap)
        y = unit.run(x, nbr, ocount)
        m = int(ocount.item())   # reference-shaped: rows are trimmed to the count (a host read)
        if m < 0:
            raise RuntimeError(f"SparseEncoder {name}: more than {cap} active output sites (capacity "
                               f"{self.capacity_factor} x {n} input rows); build with a larger capacity_factor "
                               "(a strided stage can produce up to 8 outputs per input)")
        return y[:m], oc[:m], ocount, oindex, ogrid

    def forward(self, voxel_features, coors, batch_size):
        """voxel_features [N, in_channels], coors [N, 4] (b, z, y, x) -> [B, C * D', H', W'] fp32"""
        if self.training and torch.is_grad_enabled():
            raise NotImplementedError("SparseEncoder is inference only: call .eval() or run under torch.no_grad()")
        _dev(voxel_features, coors, self.conv_input[0].weight)
        x = voxel_features.float().contiguous()
        coors = coors.int().contiguous()
        grid = (int(batch_size),) + self.sparse_shape
        if x.shape[0] == 0:
            return x.new_zeros((int(batch_size),) + self.output_shape())
        with torch.no_grad():
            count = torch.full((1,), x.shape[0], dtype=torch.int32, device=x.device)
            index = S.build_index(coors, count, grid)
            nbr = S.rulebook_subm(coors, count, index, grid)
            x = self.conv_input.run(x, nbr, count)
            for i, stage in enumerate(self.encoder_layers):
                for j, m in enumerate(stage):
                    if isinstance(m, SparseBasicBlock):
                        if nbr is None:   # one rulebook per resolution, shared by its blocks
                            nbr = S.rulebook_subm(coors, count, index, grid)
                        x = m.run(x, nbr, count)
                    else:
                        x, coors, count, index, grid = self._down(f"encoder_layer{i + 1}.{j}", m, x, coors, count,
                                                                  index, grid)
                        nbr = None
                    if x.shape[0] == 0:
                        return x.new_zeros((int(batch_size),) + self.output_shape())
            x, coors, count, index, grid = self._down("conv_out", self.conv_out, x, coors, count, index, grid)
            if x.shape[0] == 0:
                return x.new_zeros((int(batch_size),) + self.output_shape())
            return S.to_dense(x, coors, count, grid, self.output_channels)
