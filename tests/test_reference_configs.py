"""The reference's own 13 config files drop in unchanged: each is read as TEXT
by the non-executing AST loader (projects/mmdet3d_plugin/config.py -- the file
is parsed, never imported or executed), its ``model.pts_bbox_head`` dict is
built through this package's registries, and the parameter count is checked
against an independent count from the config values (SURVEY.md 8(e)
breakdown: decoder 1 053 440 per layer + post_norm, shared_conv, reference
points, bev/rv embedding MLPs, grouped task heads).  Skipped where the
reference checkout is absent (e.g. on the GPU box)."""
import glob
import os

import pytest

REF_CONFIGS = "/root/reference/projects/configs"
# the reference's config files by name, so the cases (and their ids) are the same on every machine
NAMES = sorted(f"{d}/{n}.py" for d, n in [
    ("CMTCoop_TUMTraf/camera/coop", "cmt_camera_vov_1600x640_cbgs_a9coop_pretrained"),
    ("CMTCoop_TUMTraf/camera/infra", "cmt_camera_vov_1600x640_cbgs_a9coop_infrastructure_pretrained"),
    ("CMTCoop_TUMTraf/camera/vehicle", "cmt_camera_vov_1600x640_cbgs_a9coop_vehicle_pretrained"),
    ("CMTCoop_TUMTraf/fusion/coop", "cmt_voxel0075_vov_1600x640_cbgs_a9coop_pretrained"),
    ("CMTCoop_TUMTraf/fusion/infra", "cmt_voxel0075_vov_1600x640_cbgs_a9coop_infrastructure_pretrained"),
    ("CMTCoop_TUMTraf/fusion/vehicle", "cmt_voxel0075_vov_1600x640_cbgs_a9coop_vehicle_pretrained"),
    ("CMTCoop_TUMTraf/lidar/coop", "cmt_lidar_voxel0075_cbgs_a9coop_pretrained"),
    ("CMTCoop_TUMTraf/lidar/infra", "cmt_lidar_voxel0075_cbgs_a9coop_infrastructure_pretrained"),
    ("CMTCoop_TUMTraf/lidar/vehicle", "cmt_lidar_voxel0075_cbgs_a9coop_vehicle_pretrained"),
    ("CMT_Nuscenes/camera", "cmt_camera_vov_1600x640_cbgs"),
    ("CMT_Nuscenes/fusion", "cmt_voxel0075_vov_1600x640_cbgs"),
    ("CMT_Nuscenes/fusion", "cmt_voxel0100_r50_800x320_cbgs"),
    ("CMT_Nuscenes/lidar", "cmt_lidar_voxel0075_cbgs"),
])


def _need_checkout():
    """Skip (at run time, before any work) where the reference checkout is absent."""
    if not os.path.isdir(REF_CONFIGS):
        pytest.skip("reference checkout not present")


def expected_params(h):
    C = h.get("hidden_dim", 128)
    dec = h["transformer"]["decoder"]
    L = dec["num_layers"]
    ffc = dec["transformerlayers"].get("feedforward_channels", 1024)
    layer = 2 * (3 * C * C + 3 * C) + 2 * (C * C + C) + (C * ffc + ffc) + (ffc * C + C) + 3 * 2 * C
    n = L * layer + 2 * C                                             # + post_norm
    kind = h["type"]
    if "Image" not in kind:
        n += h["in_channels"] * C * 9 + 2 * C                          # shared_conv (no bias) + BN affine
    if "Lidar" not in kind:
        D = h.get("depth_num", 64)
        n += (3 * D * 4 * C + 4 * C) + (4 * C * C + C)               # rv_embedding
    n += h.get("num_query", 900) * 3 + (2 * C * C + C) + (C * C + C)           # reference_points, bev_embedding
    k = h["separate_head"]["final_kernel"]
    for t in h["tasks"]:
        heads = dict(h["common_heads"], cls_logits=(t["num_class"], 2))
        for out, _ in heads.values():
            n += L * 64 * C * k + 2 * L * 64 + L * out * 64 * k + L * out
    return n


@pytest.mark.parametrize("name", NAMES)
def test_reference_config_builds_unchanged(name):
    _need_checkout()
    path = os.path.join(REF_CONFIGS, name)
    from projects.mmdet3d_plugin import build_head
    from projects.mmdet3d_plugin.config import load_config
    from projects.mmdet3d_plugin.registry import HEADS
    cfg = load_config(path)
    assert cfg.get("plugin") is True
    h = cfg["model"]["pts_bbox_head"]
    assert h["type"] in HEADS
    head = build_head(h)
    assert type(head).__name__ == h["type"]
    n = sum(p.numel() for p in head.parameters())
    assert n == expected_params(h), (n, expected_params(h))
    keys = set(head.state_dict())
    L = h["transformer"]["decoder"]["num_layers"]
    for i in range(L):
        p = f"transformer.decoder.layers.{i}."
        for k in ("attentions.0.attn.in_proj_weight", "attentions.1.attn.in_proj_weight",
                  "attentions.1.attn.out_proj.bias", "ffns.0.layers.0.0.weight", "ffns.0.layers.1.weight",
                  "norms.2.bias"):
            assert p + k in keys, p + k
    assert "transformer.decoder.post_norm.weight" in keys
    assert any(k.startswith("task_heads.0.cls_logits.3.") for k in keys)
    assert ("shared_conv.conv.weight" in keys) == ("Image" not in h["type"])
    assert ("rv_embedding.0.weight" in keys) == ("Lidar" not in h["type"])


def test_all_thirteen_present():
    _need_checkout()
    files = sorted(glob.glob(os.path.join(REF_CONFIGS, "**", "*.py"), recursive=True))
    assert len(files) == 13
    assert [os.path.relpath(f, REF_CONFIGS) for f in files] == NAMES
