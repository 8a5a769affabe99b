"""MI355X-native drop-in for the reference's ``projects.mmdet3d_plugin`` hot
path (CMT / CMTCoop decoder heads, transformer, attention, voxelization).

Importing the package registers the reference's type names
(CmtHead, CmtLidarHead, CmtImageHead, CmtHeadCoop, CmtLidarHeadCoop,
CmtImageHeadCoop, CmtTransformer, CmtLidarTransformer, CmtImageTransformer,
PETRTransformerDecoder, PETRTransformerDecoderLayer,
PETRMultiheadFlashAttention, MultiheadAttention, FFN, SeparateTaskHead,
MultiTaskBBoxCoder, SPConvVoxelization, SparseEncoder, SECOND, SECONDFPN) so
the reference's ``pts_bbox_head`` config dicts build unchanged with
``build_head`` (and ``pts_middle_encoder`` / ``pts_backbone`` / ``pts_neck``
with ``build_middle_encoder`` / ``build_backbone`` / ``build_neck``).
"""
from . import core, mmcv_custom, models  # noqa: F401
from .registry import (ATTENTION, BACKBONES, BBOX_CODERS, HEADS, MIDDLE_ENCODERS, NECKS, TRANSFORMER,  # noqa: F401
                       TRANSFORMER_LAYER, TRANSFORMER_LAYER_SEQUENCE, build_backbone, build_from_cfg, build_head,
                       build_middle_encoder, build_neck)
from .runtime import get_precision, set_precision  # noqa: F401
