"""CPFPN: the reference's ``img_neck`` (``img_neck=dict(type='CPFPN', ...)`` in every camera and fusion
config) on ``cmt_fpn_lateral`` / ``cmt_rows_to_nchw`` (csrc/fpn.hip) and ``cmt_gemm``'s 3 x 3 conv,
inference only.

The semantics are those of mmdet's FPN with a single output conv, restated (neither mmdet nor mmcv is a
dependency): one 1 x 1 lateral conv per used level; top-down, each finer lateral gets the coarser one
added after nearest upsampling to its size (``F.interpolate(size=..., mode='nearest')``); ``outs[0]`` is
the 3 x 3 / pad 1 conv of lateral 0, ``outs[i > 0]`` is lateral ``i`` itself; outputs beyond the levels
are the previous one subsampled ``[:, :, ::2, ::2]`` (``max_pool2d(kernel 1, stride 2)``).

Routing.  The laterals run from the coarsest level down, each straight from the backbone's fp32 NCHW map
with the coarser lateral's rows as the epilogue's top-down term, so lateral ``i`` already holds everything
above it and no upsampled map or sum is written.  The output conv runs on pair rows (cmt_gemm
CMT_A_CONV3X3); every output leaves through ``cmt_rows_to_nchw`` as the contiguous fp32 NCHW map the head
reads (``outs[0]`` is its ``img_feats[0]``), without a torch op on that path.

Each conv follows mmcv's ``ConvModule`` layout (conv, an optional norm named ``bn``, an optional
activation; the conv has a bias exactly when there is no norm).  state_dict keys:
``lateral_convs.{i}.conv.{weight, bias}`` and ``fpn_convs.0.conv.{weight, bias}``; with a BN
``....bn.{weight, bias, running_mean, running_var, num_batches_tracked}`` and no conv bias.  These keys are
restated from mmcv 1.6.2, not checked against a real checkpoint here.
"""
import torch
import torch.nn as nn

from ... import native_bev as NB
from ... import native_fpn as NF
from ...native import _dev
from ...registry import NECKS
from ..backbones.second import RangeFlagMixin, bn_eps_momentum, bn_tensors, inference_only
from ..utils.packing import PackCache

__all__ = ["CPFPN"]


class _ConvModule(nn.Module):
    """conv -> optional BN (``bn``) -> optional ReLU (``activate``), the attribute names of mmcv's ConvModule"""

    def __init__(self, cin, cout, k, norm, relu):
        super().__init__()
        self.conv = nn.Conv2d(cin, cout, k, padding=k // 2, bias=norm is None)
        if norm is not None:
            self.bn = nn.BatchNorm2d(cout, eps=norm[0], momentum=norm[1])
        if relu:
            self.activate = nn.ReLU(inplace=False)
        self.relu = bool(relu)
        if self.conv.bias is not None:
            nn.init.zeros_(self.conv.bias)

    def pack_source(self):
        """(the tensors a pack is made from, the BN eps or None, pack_conv*'s second argument)"""
        bn = getattr(self, "bn", None)
        if bn is None:
            return [self.conv.weight, self.conv.bias], None, self.conv.bias
        return [self.conv.weight] + bn_tensors(bn), bn.eps, bn_tensors(bn) + [bn.eps]


@NECKS.register_module()
class CPFPN(nn.Module, RangeFlagMixin):
    def __init__(self, in_channels, out_channels, num_outs, start_level=0, end_level=-1, add_extra_convs=False,
                 relu_before_extra_convs=False, no_norm_on_lateral=False, conv_cfg=None, norm_cfg=None, act_cfg=None,
                 upsample_cfg=dict(mode="nearest"),
                 init_cfg=dict(type="Xavier", layer="Conv2d", distribution="uniform")):
        super().__init__()
        if not isinstance(in_channels, (list, tuple)) or not in_channels:
            raise ValueError("CPFPN in_channels must be a non-empty list")
        if add_extra_convs:
            raise NotImplementedError(f"CPFPN add_extra_convs={add_extra_convs!r}: extra stride-2 convs have no "
                                      "native path (no reference config sets it)")
        if start_level != 0:
            raise NotImplementedError(f"CPFPN start_level={start_level}: the output conv exists for level 0 only, so "
                                      "the reference's own forward fails for any other start")
        if dict(upsample_cfg) != dict(mode="nearest"):
            raise NotImplementedError(f"CPFPN upsample_cfg {dict(upsample_cfg)}: only plain mode='nearest' is built "
                                      "(a scale_factor changes torch's index rule)")
        if conv_cfg is not None and dict(conv_cfg) != dict(type="Conv2d"):
            raise NotImplementedError(f"CPFPN conv_cfg {conv_cfg}: only the default Conv2d is built")
        if act_cfg is not None and act_cfg.get("type") != "ReLU":
            raise NotImplementedError(f"CPFPN act_cfg type {act_cfg.get('type')!r}: only 'ReLU' is built")
        norm = None if norm_cfg is None else bn_eps_momentum("CPFPN", norm_cfg)
        n_in = len(in_channels)
        if end_level == -1:
            end = n_in
            if num_outs < end - start_level:
                raise ValueError(f"CPFPN num_outs {num_outs} below the {end - start_level} levels used")
        else:
            end = int(end_level)
            if not 0 < end <= n_in:
                raise ValueError(f"CPFPN end_level {end_level} outside the {n_in} inputs")
            if num_outs != end - start_level:
                raise ValueError(f"CPFPN num_outs {num_outs} must equal end_level - start_level = {end - start_level}")
        if out_channels <= 0 or out_channels % 128 or any(c <= 0 or c % 16 for c in in_channels[:end]):
            raise NotImplementedError(f"CPFPN channels {list(in_channels)} -> {out_channels}: the lateral kernel needs "
                                      "in_channels % 16 == 0 and out_channels % 128 == 0")
        self.in_channels, self.out_channels = [int(c) for c in in_channels], int(out_channels)
        self.num_ins, self.num_outs = n_in, int(num_outs)
        self.start_level, self.end_level, self.backbone_end_level = 0, int(end_level), end
        self.add_extra_convs, self.relu_before_extra_convs = False, bool(relu_before_extra_convs)
        self.no_norm_on_lateral = bool(no_norm_on_lateral)
        self.upsample_cfg = dict(upsample_cfg)
        relu = act_cfg is not None
        self.lateral_convs = nn.ModuleList(
            _ConvModule(c, self.out_channels, 1, None if self.no_norm_on_lateral else norm, relu)
            for c in self.in_channels[:end])
        self.fpn_convs = nn.ModuleList([_ConvModule(self.out_channels, self.out_channels, 3, norm, relu)])
        self._pack = PackCache()

    def packed(self, which, i=0):
        """(pair rows, shift) of ``lateral_convs[i]`` (``which='lateral'``, [Cout, 2, Cin]) or of the output
        conv (``which='fpn'``, [Cout, 2, 9 Cout]), repacked when a tensor it is made from changes"""
        m = self.lateral_convs[i] if which == "lateral" else self.fpn_convs[i]
        tensors, eps, second = m.pack_source()
        pack = NF.pack_conv1x1 if which == "lateral" else NF.pack_conv3x3_bias
        return self._pack.get((which, i), tensors, eps, lambda: pack(m.conv.weight, second))

    def forward(self, inputs):
        """A sequence of fp32 NCHW maps, one per entry of ``in_channels`` -> a tuple of ``num_outs`` contiguous
        fp32 NCHW maps [B, out_channels, H_i, W_i]"""
        inference_only(self)
        if len(inputs) != self.num_ins:
            raise ValueError(f"CPFPN takes {self.num_ins} maps, got {len(inputs)}")
        used = list(inputs[:self.backbone_end_level])
        for m, c in zip(used, self.in_channels):
            if not torch.is_tensor(m) or m.dim() != 4 or m.shape[1] != c or not m.is_floating_point():
                raise ValueError(f"CPFPN: a floating [B, {c}, H, W] map expected, got "
                                 f"{tuple(m.shape) if torch.is_tensor(m) else type(m)}")
        sizes = [(int(m.shape[2]), int(m.shape[3])) for m in used]
        B = int(used[0].shape[0])
        if any(int(m.shape[0]) != B for m in used) or B <= 0 or min(min(s) for s in sizes) <= 0:
            raise ValueError(f"CPFPN: non-empty maps of one batch size expected, got {[tuple(m.shape) for m in used]}")
        for fine, coarse in zip(sizes, sizes[1:]):
            if coarse[0] > fine[0] or coarse[1] > fine[1]:
                raise ValueError(f"CPFPN: a coarser level {coarse} larger than the finer one {fine}")
        if sizes[0][1] > NB.WMAX:
            raise NotImplementedError(f"CPFPN: level-0 width {sizes[0][1]} above {NB.WMAX}, the output conv's limit")
        _dev(self.lateral_convs[0].conv.weight, *used)
        co = self.out_channels
        with torch.no_grad():
            flag = self._range_flag(used[0].device)
            top, laterals = None, [None] * len(used)
            for i in range(len(used) - 1, -1, -1):
                wp, shift = self.packed("lateral", i)
                top = NF.lateral(used[i].float().contiguous(), wp, shift, Cout=co, top=top,
                                 top_hw=None if top is None else sizes[i + 1], relu=self.lateral_convs[i].relu,
                                 range_flag=flag)
                laterals[i] = top
            wp, shift = self.packed("fpn")
            H0, W0 = sizes[0]
            rows = NB.conv3x3_gemm(laterals[0], wp, shift, B=B, H=H0, W=W0, Cin=co, Cout=co,
                                   relu=self.fpn_convs[0].relu, range_flag=flag)
            outs = [NF.rows_to_nchw(rows, (B, co, H0, W0))]
            for i in range(1, len(used)):
                outs.append(NF.rows_to_nchw(laterals[i], (B, co) + sizes[i]))
            while len(outs) < self.num_outs:
                outs.append(outs[-1][:, :, ::2, ::2].contiguous())
        return tuple(outs)
