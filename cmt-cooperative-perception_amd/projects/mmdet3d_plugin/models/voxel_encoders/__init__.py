"""HardSimpleVFE (mmdet3d/models/voxel_encoders/voxel_encoder.py): the mean of each voxel's points, no
parameters.  A CmtDetector whose encoder is this class never calls it: the voxelizer's kernel already
returns the mean (``SPConvVoxelization.forward_mean`` / ``voxelize_batch``).  The forward below restates the
module for callers that hold padded voxels."""
import torch.nn as nn

from ...registry import VOXEL_ENCODERS

__all__ = ["HardSimpleVFE"]


@VOXEL_ENCODERS.register_module()
class HardSimpleVFE(nn.Module):
    def __init__(self, num_features=4):
        super().__init__()
        self.num_features = int(num_features)
        self.fp16_enabled = False

    def forward(self, features, num_points, coors=None):
        """features [M, max_points, >= num_features] (zero-padded slots), num_points [M] -> [M, num_features]"""
        points_mean = features[:, :, :self.num_features].sum(dim=1) / num_points.type_as(features).view(-1, 1)
        return points_mean.contiguous()
