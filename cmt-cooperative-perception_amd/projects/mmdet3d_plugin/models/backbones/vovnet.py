"""VoVNet: the reference's ``img_backbone`` (``img_backbone=dict(type='VoVNet', spec_name='V-99-eSE',
out_features=('stage4', 'stage5'))`` in the camera and fusion configs) on the image backbone kernels
(csrc/vov.hip, ``cmt_img_*``), inference only, the non-depthwise eSE specs.

The semantics are those of VoVNet-V2 (Lee and Park, "CenterMask", 2020) as the reference builds it,
restated (neither mmcv nor mmdet is a dependency):

* stem: three ``conv3x3 -> BN -> ReLU`` with strides 2, 1, 2 (pad 1, bias-free, BN eps 1e-5);
* four stages ``stage2 .. stage5`` of OSA blocks; every stage but ``stage2`` starts with
  ``MaxPool2d(3, stride 2, ceil_mode=True)`` without padding;
* an OSA block chains ``layer_per_block`` 3 x 3 convs (the first ``in_ch -> stage_ch``), concatenates the
  block's input and every layer's output along channels, reduces them with a 1 x 1 ``conv -> BN -> ReLU``
  to ``concat_ch`` and gates the result, ``x * hsigmoid(fc(mean_{H,W}(x)))`` with a biased 1 x 1 ``fc`` and
  ``hsigmoid(t) = relu6(t + 3) / 6`` -- in every block; blocks after a stage's first add the block's
  input after the gate;
* forward returns an ordered dict name -> map for the names in ``out_features``, in network order.

Routing.  ``stem_1`` runs on ``cmt_img_stem`` straight from the fp32 NCHW image; every other 3 x 3 conv
on ``cmt_img_conv3x3`` (pair rows to pair rows), but the stride-1 128 -> 128 layers (stage2's chain), which
measured faster on ``cmt_gemm``'s CMT_A_CONV3X3 pair-row path (``GEMM_ROUTED``, static per shape, the rows are
bit-equal either way); the aggregation on ``cmt_img_concat1x1`` from the block's
sources without a concatenated map, its epilogue leaving the pool's per-tile sums for ``cmt_img_ese_gate``;
``cmt_img_ese_apply`` scales (and adds the identity) in place; ``cmt_img_maxpool`` between stages.  The
selected maps leave through ``cmt_rows_to_nchw`` as contiguous fp32 NCHW, what ``CPFPN`` reads.

Arithmetic.  ``native_img.set_img_precision('ref' | 'fp16')`` (env ``CMT_IMG_PRECISION``, default ``'ref'``),
read once per forward: ``'ref'`` is the routing above, three-pass split-f16 on pair rows; ``'fp16'`` is the same walk
on ``cmt_img_*_f16`` -- plain fp16 rows between launches, weights folded in float64 and rounded once to fp16, one
MFMA per step with fp32 accumulation -- and leaves through ``cmt_rows_to_nchw_f16``; nothing is routed to
``cmt_gemm`` there.  The gate stays fp32 (``cmt_img_ese_gate``).  Packs are cached per arithmetic.

state_dict keys carry the ``/`` of the reference's module names: ``stem.stem_1/conv.weight``,
``stem.stem_1/norm.{weight, bias, running_mean, running_var, num_batches_tracked}``,
``stage3.OSA3_2.layers.4.OSA3_2_4/conv.weight``, ``stage2.OSA2_1.concat.OSA2_1_concat/conv.weight``,
``stageN.OSAN_k.ese.fc.{weight, bias}``.  They are pinned against the reference's own class
(tests/golden/vovnet_keys.json), not against a real checkpoint.
"""
from collections import OrderedDict

import torch
import torch.nn as nn

from ... import native_bev as NB
from ... import native_fpn as NF
from ... import native_img as NI
from ...native import _dev
from ...registry import BACKBONES
from ..utils.packing import PackCache
from .second import RangeFlagMixin, bn_tensors, inference_only

__all__ = ["VoVNet", "SPECS", "GEMM_ROUTED", "route_conv3x3"]

_CH = dict(stem=(64, 64, 128), stage_conv_ch=(128, 160, 192, 224), stage_out_ch=(256, 512, 768, 1024))
# spec name -> layer_per_block, block_per_stage (the eSE specs with full-width channels)
SPECS = {
    "V-19-eSE": dict(_CH, layer_per_block=3, block_per_stage=(1, 1, 1, 1)),
    "V-39-eSE": dict(_CH, layer_per_block=5, block_per_stage=(1, 1, 2, 2)),
    "V-57-eSE": dict(_CH, layer_per_block=5, block_per_stage=(1, 1, 4, 3)),
    "V-99-eSE": dict(_CH, layer_per_block=5, block_per_stage=(1, 3, 9, 3)),
}
_UNBUILT = {
    "V-19-slim-dw-eSE": "a depthwise spec (grouped 3 x 3 convs have no native kernel)",
    "V-19-dw-eSE": "a depthwise spec (grouped 3 x 3 convs have no native kernel)",
    "V-19-slim-eSE": "a slim spec whose stage channels 80 and 112 are no multiple of 32, which the conv kernels need",
}
NAMES = ("stem", "stage2", "stage3", "stage4", "stage5")
# (Cin, Cout) of the stride-1 3 x 3 layers that run on cmt_gemm's CMT_A_CONV3X3 path: the shapes an alternating
# same-session A/B at the V-99-eSE full-size maps showed faster there outside the spread
GEMM_ROUTED = frozenset({(128, 128)})


def route_conv3x3(rows, wp, shift, *, B, H, W, Cin, Cout, stride, relu=True, out=None, range_flag=None):
    """a 3 x 3 layer on the kernel its shape is routed to (static, no runtime switch)"""
    if stride == 1 and (Cin, Cout) in GEMM_ROUTED:
        return NI.conv3x3_gemm(rows, wp, shift, B=B, H=H, W=W, Cin=Cin, Cout=Cout, relu=relu, out=out,
                               range_flag=range_flag)
    return NI.conv3x3(rows, wp, shift, B=B, H=H, W=W, Cin=Cin, Cout=Cout, stride=stride, relu=relu, out=out,
                      range_flag=range_flag)


def _op(mod, name, fp16):
    """the wrapper of the forward's arithmetic, looked up at the call"""
    return getattr(mod, name + "_f16" if fp16 else name)


def _conv_bn(cin, cout, k, stride, name):
    return [(f"{name}/conv", nn.Conv2d(cin, cout, k, stride=stride, padding=k // 2, bias=False)),
            (f"{name}/norm", nn.BatchNorm2d(cout)), (f"{name}/relu", nn.ReLU(inplace=True))]


def _pair_of(seq):
    """(conv, bn) of a conv -> BN -> ReLU Sequential"""
    return seq[0], seq[1]


class _ESE(nn.Module):
    def __init__(self, ch):
        super().__init__()
        self.fc = nn.Conv2d(ch, ch, 1)


class _OSA(nn.Module):
    def __init__(self, in_ch, stage_ch, concat_ch, layer_per_block, name, identity):
        super().__init__()
        self.identity = bool(identity)
        self.in_ch, self.stage_ch, self.concat_ch = in_ch, stage_ch, concat_ch
        self.layers = nn.ModuleList(
            nn.Sequential(OrderedDict(_conv_bn(in_ch if i == 0 else stage_ch, stage_ch, 3, 1, f"{name}_{i}")))
            for i in range(layer_per_block))
        self.concat = nn.Sequential(OrderedDict(
            _conv_bn(in_ch + layer_per_block * stage_ch, concat_ch, 1, 1, f"{name}_concat")))
        self.ese = _ESE(concat_ch)


class _Pool(nn.Module):
    """MaxPool2d(3, stride 2, ceil_mode=True): no tensors"""


@BACKBONES.register_module()
class VoVNet(nn.Module, RangeFlagMixin):
    def __init__(self, spec_name, input_ch=3, out_features=None, frozen_stages=-1, norm_eval=True, pretrained=None,
                 init_cfg=None):
        super().__init__()
        if spec_name in _UNBUILT:
            raise NotImplementedError(f"VoVNet spec {spec_name!r} is {_UNBUILT[spec_name]}; built: {sorted(SPECS)}")
        if spec_name not in SPECS:
            raise KeyError(f"unknown VoVNet spec {spec_name!r}; known: {sorted(SPECS) + sorted(_UNBUILT)}")
        if not isinstance(input_ch, int) or not 1 <= input_ch <= 3:
            raise NotImplementedError(f"VoVNet input_ch={input_ch!r}: the stem kernel packs K = 9 input_ch into 32, "
                                      "so 1 to 3 input channels are built")
        if out_features is None or len(out_features) == 0:
            raise ValueError(f"VoVNet out_features must name at least one of {NAMES}")
        for n in out_features:
            if n not in NAMES:
                raise ValueError(f"VoVNet out_features {tuple(out_features)}: {n!r} is none of {NAMES}")
        spec = SPECS[spec_name]
        self.spec_name, self.input_ch = spec_name, input_ch
        self._out_features = tuple(out_features)
        self.frozen_stages, self.norm_eval, self.pretrained, self.init_cfg = frozen_stages, norm_eval, pretrained, init_cfg
        s = spec["stem"]
        self.stem = nn.Sequential(OrderedDict(_conv_bn(input_ch, s[0], 3, 2, "stem_1") +
                                              _conv_bn(s[0], s[1], 3, 1, "stem_2") +
                                              _conv_bn(s[1], s[2], 3, 2, "stem_3")))
        self.stage_names = list(NAMES[1:])
        in_ch = s[2]
        self._out_feature_channels = {"stem": s[2]}
        self._out_feature_strides = {"stem": 4}
        for i, name in enumerate(self.stage_names):
            stage_ch, concat_ch = spec["stage_conv_ch"][i], spec["stage_out_ch"][i]
            mods = OrderedDict()
            if i > 0:
                mods["Pooling"] = _Pool()
            for k in range(spec["block_per_stage"][i]):
                blk = f"OSA{i + 2}_{k + 1}"
                mods[blk] = _OSA(in_ch if k == 0 else concat_ch, stage_ch, concat_ch, spec["layer_per_block"], blk,
                                 identity=k > 0)
            setattr(self, name, nn.Sequential(mods))
            in_ch = concat_ch
            self._out_feature_channels[name] = concat_ch
            self._out_feature_strides[name] = 4 << i
        self._pack = PackCache()

    def init_weights(self):
        """weights come from a checkpoint (or the caller); nothing to initialise"""

    # ---- packs -------------------------------------------------------------------------------------------
    def _packed(self, key, seq, pack, fp16=False):
        conv, bn = _pair_of(seq)
        return self._pack.get(key + ("fp16",) if fp16 else key, [conv.weight] + bn_tensors(bn), bn.eps,
                              lambda: pack(conv.weight, bn_tensors(bn) + [bn.eps]))

    def packed_stem(self, i, fp16=False):
        """(pair rows, shift) of stem conv ``i`` (0: [64, 2, 32] for cmt_img_stem; 1, 2: [Cout, 2, 9 Cin]);
        ``fp16``: (fp16 rows [64, 32] or [Cout, 9 Cin], shift) of the one-pass policy, cached apart"""
        seq = self.stem[3 * i:3 * i + 2]
        if fp16:
            return self._packed(("stem", i), seq, NI.pack_stem_f16 if i == 0 else NI.pack_conv3x3_f16, True)
        return self._packed(("stem", i), seq, NI.pack_stem if i == 0 else NB.pack_conv3x3)

    def packed_layer(self, blk_name, blk, i, fp16=False):
        """(pair rows, shift) of 3 x 3 layer ``i`` of an OSA block, or of its aggregation (``i='concat'``);
        ``fp16``: the one-pass policy's fp16 rows, cached apart"""
        if i == "concat":
            return self._packed((blk_name, i), blk.concat, NI.pack_concat_f16 if fp16 else NI.pack_concat, fp16)
        return self._packed((blk_name, i), blk.layers[i], NI.pack_conv3x3_f16 if fp16 else NB.pack_conv3x3, fp16)

    def packed_fc(self, blk_name, blk):
        """(fp32 [C, C], fp32 [C]) of the gate's fc"""
        fc = blk.ese.fc
        return self._pack.get((blk_name, "fc"), [fc.weight, fc.bias], None,
                              lambda: (fc.weight.detach().float().reshape(fc.weight.shape[0], -1).contiguous(),
                                       fc.bias.detach().float().contiguous()))

    # ---- forward -----------------------------------------------------------------------------------------
    def conv3x3(self, rows, w, shift, *, fp16, flag, **kw):
        """a 3 x 3 layer: 'ref' routes by shape (GEMM_ROUTED), 'fp16' routes nothing"""
        return (NI.conv3x3_f16 if fp16 else route_conv3x3)(rows, w, shift, range_flag=flag, **kw)

    def _osa(self, name, blk, x, B, H, W, flag, fp16=False):
        srcs, cur, cin = [x], x, blk.in_ch
        for i in range(len(blk.layers)):
            w, shift = self.packed_layer(name, blk, i, fp16=fp16)
            cur = self.conv3x3(cur, w, shift, B=B, H=H, W=W, Cin=cin, Cout=blk.stage_ch, stride=1, fp16=fp16, flag=flag)
            srcs.append(cur)
            cin = blk.stage_ch
        w, shift = self.packed_layer(name, blk, "concat", fp16=fp16)
        y, part = _op(NI, "concat1x1", fp16)(srcs, w, shift, B=B, HW=H * W, Cout=blk.concat_ch, part=True,
                                             range_flag=flag)
        fw, fb = self.packed_fc(name, blk)
        gate = NI.ese_gate(part, fw, fb, HW=H * W)
        return _op(NI, "ese_apply", fp16)(y, gate, B=B, HW=H * W, C=blk.concat_ch, identity=x if blk.identity else None,
                                          out=y, range_flag=flag)

    def forward(self, x):
        """[B, input_ch, H, W] -> an ordered dict name -> contiguous fp32 NCHW map for ``out_features``, in the
        arithmetic of ``native_img.img_precision()`` at the time of the call"""
        inference_only(self)
        if not torch.is_tensor(x) or x.dim() != 4 or x.shape[1] != self.input_ch or not x.is_floating_point():
            raise ValueError(f"VoVNet takes a floating [B, {self.input_ch}, H, W] image, got "
                             f"{tuple(x.shape) if torch.is_tensor(x) else type(x)}")
        B, _, H, W = (int(s) for s in x.shape)
        if min(B, H, W) <= 0:
            raise ValueError(f"VoVNet: a non-empty image expected, got {tuple(x.shape)}")
        # the sizes down the network, so a map too small for a pool fails before any launch
        h, w = NB.out_hw(*NB.out_hw(H, W, 2), 2)
        for _ in self.stage_names[1:]:
            h, w = NI.pool_hw(h, w)
        _dev(x, self.stem[0].weight)
        outs = OrderedDict()
        with torch.no_grad():
            flag = self._range_flag(x.device)
            x = x.float().contiguous()
            fp16 = NI.img_precision() == "fp16"     # rows between launches: plain fp16 [B*H*W, C], else pair rows
            s = [self.stem[3 * i].out_channels for i in range(3)]
            w, shift = self.packed_stem(0, fp16=fp16)
            rows = _op(NI, "stem", fp16)(x, w, shift, Cout=s[0], range_flag=flag)
            H, W = NB.out_hw(H, W, 2)
            w, shift = self.packed_stem(1, fp16=fp16)
            rows = self.conv3x3(rows, w, shift, B=B, H=H, W=W, Cin=s[0], Cout=s[1], stride=1, fp16=fp16, flag=flag)
            w, shift = self.packed_stem(2, fp16=fp16)
            rows = self.conv3x3(rows, w, shift, B=B, H=H, W=W, Cin=s[1], Cout=s[2], stride=2, fp16=fp16, flag=flag)
            H, W = NB.out_hw(H, W, 2)
            C = s[2]
            if "stem" in self._out_features:
                outs["stem"] = _op(NF, "rows_to_nchw", fp16)(rows, (B, C, H, W))
            for name in self.stage_names:
                for blk_name, blk in getattr(self, name).named_children():
                    if isinstance(blk, _Pool):
                        rows = _op(NI, "maxpool", fp16)(rows, B=B, H=H, W=W, C=C)
                        H, W = NI.pool_hw(H, W)
                    else:
                        rows = self._osa(blk_name, blk, rows, B, H, W, flag, fp16)
                        C = blk.concat_ch
                if name in self._out_features:
                    outs[name] = _op(NF, "rows_to_nchw", fp16)(rows, (B, C, H, W))
        return outs
