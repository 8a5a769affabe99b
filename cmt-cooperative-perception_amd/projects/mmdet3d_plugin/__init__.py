"""MI355X-native drop-in for the reference's ``projects.mmdet3d_plugin`` hot
path (CMT / CMTCoop decoder heads, transformer, attention, voxelization).

Importing the package registers the reference's type names
(CmtHead, CmtLidarHead, CmtImageHead, CmtHeadCoop, CmtLidarHeadCoop,
CmtImageHeadCoop, CmtTransformer, CmtLidarTransformer, CmtImageTransformer,
PETRTransformerDecoder, PETRTransformerDecoderLayer,
PETRMultiheadFlashAttention, MultiheadAttention, FFN, SeparateTaskHead,
MultiTaskBBoxCoder, SPConvVoxelization, HardSimpleVFE, SparseEncoder, SECOND,
SECONDFPN, VoVNet, CPFPN, CmtDetector, CmtCoopDetector) so the reference's
``model`` config dicts build unchanged with ``build_detector`` (and
``pts_bbox_head`` / ``pts_middle_encoder`` / ``pts_backbone`` / ``pts_neck``
alone with ``build_head`` / ``build_middle_encoder`` / ``build_backbone`` /
``build_neck``).
"""
from . import core, mmcv_custom, models  # noqa: F401
from .registry import (ATTENTION, BACKBONES, BBOX_CODERS, DETECTORS, HEADS, MIDDLE_ENCODERS, NECKS,  # noqa: F401
                       TRANSFORMER, TRANSFORMER_LAYER, TRANSFORMER_LAYER_SEQUENCE, VOXEL_ENCODERS, build_backbone,
                       build_detector, build_from_cfg, build_head, build_middle_encoder, build_model, build_neck,
                       build_voxel_encoder)
from .runtime import get_precision, set_precision  # noqa: F401
