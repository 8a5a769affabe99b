"""SECONDFPN: the reference's ``pts_neck`` (``pts_neck=dict(type='SECONDFPN', ...)`` in every LiDAR and
fusion config) on ``cmt_bev_deblock`` (csrc/bev.hip), inference only.

The semantics are mmdet3d 1.0.0rc6's ``SECONDFPN``, restated (mmdet3d is not a dependency):
``deblocks[i] = Sequential(up, BN, ReLU)`` with ``up`` a ``ConvTranspose2d(in_i, out_i, k, stride=k)`` for
``k = upsample_strides[i]`` (weight (Cin, Cout, k, k)), or, for ``k == 1`` with
``use_conv_for_no_stride=True``, a 1 x 1 ``Conv2d`` (weight (Cout, Cin, 1, 1)); the outputs are concatenated
along channels.  Every deblock writes its channel slice of the one fp32 NCHW output itself, so there is
no ``torch.cat``, and the result is what the head's shared_conv reads.  Fractional ``upsample_strides`` (a
strided conv in mmdet3d) have no native path.

state_dict keys: ``deblocks.{i}.0.weight`` and ``deblocks.{i}.1.{weight, bias, running_mean, running_var,
num_batches_tracked}``, restated from mmdet3d, not checked against a real checkpoint here.
"""
import torch
import torch.nn as nn

from ... import native_bev as NB
from ...native import _dev
from ...registry import NECKS
from ..backbones.second import RangeFlagMixin, bn_eps_momentum, bn_tensors, inference_only, no_bias_conv
from ..utils.packing import PackCache

__all__ = ["SECONDFPN"]


@NECKS.register_module()
class SECONDFPN(nn.Module, RangeFlagMixin):
    def __init__(self, in_channels=[128, 128, 256], out_channels=[256, 256, 256], upsample_strides=[1, 2, 4],
                 norm_cfg=dict(type="BN", eps=1e-3, momentum=0.01), upsample_cfg=dict(type="deconv", bias=False),
                 conv_cfg=dict(type="Conv2d", bias=False), use_conv_for_no_stride=False, init_cfg=None):
        super().__init__()
        if not (len(in_channels) == len(out_channels) == len(upsample_strides)):
            raise ValueError("in_channels, out_channels and upsample_strides differ in length")
        eps, mom = bn_eps_momentum("SECONDFPN", norm_cfg)
        no_bias_conv("SECONDFPN upsample_cfg", upsample_cfg, ("deconv",))
        no_bias_conv("SECONDFPN conv_cfg", conv_cfg, ("Conv2d",))
        for k in upsample_strides:
            if k not in (1, 2, 4):
                raise NotImplementedError(f"SECONDFPN upsample_strides {list(upsample_strides)}: only 1, 2 and 4 "
                                          "are built (a fractional stride is a strided conv in mmdet3d)")
        for ci, co in zip(in_channels, out_channels):
            if ci <= 0 or ci % 32 or co <= 0 or co % 128:
                raise NotImplementedError(f"SECONDFPN channels {list(in_channels)} -> {list(out_channels)}: the "
                                          "deblock kernel needs in_channels % 32 == 0 and out_channels % 128 == 0")
        self.in_channels, self.out_channels = [int(c) for c in in_channels], [int(c) for c in out_channels]
        self.upsample_strides = [int(k) for k in upsample_strides]
        self.use_conv_for_no_stride = bool(use_conv_for_no_stride)
        deblocks = []
        for ci, co, k in zip(self.in_channels, self.out_channels, self.upsample_strides):
            if k == 1 and self.use_conv_for_no_stride:
                up = nn.Conv2d(ci, co, 1, stride=1, bias=False)
            else:
                up = nn.ConvTranspose2d(ci, co, k, stride=k, bias=False)
            deblocks.append(nn.Sequential(up, nn.BatchNorm2d(co, eps=eps, momentum=mom), nn.ReLU(inplace=True)))
        self.deblocks = nn.ModuleList(deblocks)
        self._pack = PackCache()

    def packed(self, i):
        """(pair rows [k*k*Cout, 2, Cin], shift [Cout]) of deblock ``i``"""
        up, bn = self.deblocks[i][0], self.deblocks[i][1]
        k = self.upsample_strides[i]
        return self._pack.get(i, [up.weight] + bn_tensors(bn), bn.eps,
                              lambda: NB.pack_deblock(up.weight, bn_tensors(bn) + [bn.eps], k,
                                                      transposed=isinstance(up, nn.ConvTranspose2d)))

    def forward(self, x):
        """A sequence of RowMap (SECOND's output) or fp32 NCHW tensors -> ``[out]``, ``out`` fp32 contiguous
        [B, sum(out_channels), H, W]"""
        inference_only(self)
        if len(x) != len(self.in_channels):
            raise ValueError(f"SECONDFPN takes {len(self.in_channels)} maps, got {len(x)}")
        sizes = set()
        for m, ci, k in zip(x, self.in_channels, self.upsample_strides):
            shp = tuple(m.shape)
            if len(shp) != 4 or shp[1] != ci:
                raise ValueError(f"SECONDFPN: a [B, {ci}, H, W] map expected, got {shp}")
            sizes.add((shp[0], k * shp[2], k * shp[3]))
        if len(sizes) != 1:
            raise ValueError(f"SECONDFPN: the deblock outputs differ in size (B, H, W): {sorted(sizes)}")
        B, Ho, Wo = sizes.pop()
        _dev(self.deblocks[0][0].weight, *[m.rows if isinstance(m, NB.RowMap) else m for m in x])
        with torch.no_grad():
            dev = self.deblocks[0][0].weight.device
            flag = self._range_flag(dev)
            out = torch.empty((B, sum(self.out_channels), Ho, Wo), dtype=torch.float32, device=dev)
            c0 = 0
            for i, (m, ci, co, k) in enumerate(zip(x, self.in_channels, self.out_channels, self.upsample_strides)):
                if not isinstance(m, NB.RowMap):
                    m = NB.to_rows(m.float().contiguous(), range_flag=flag)
                wp, shift = self.packed(i)
                NB.deblock(m.rows, wp, shift, out, B=B, H=m.shape[2], W=m.shape[3], Cin=ci, Cout=co, k=k, c0=c0,
                           range_flag=flag)
                c0 += co
        return [out]
