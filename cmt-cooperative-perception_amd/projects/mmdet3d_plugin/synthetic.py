"""Synthetic frames, camera geometry and seeded weights for the BASELINE.json
configs (no datasets or checkpoints are available offline).

  * BEV features  [B, 512, H, W] = relu(N(0,1))  (SECONDFPN ends in BN+ReLU)
  * image features [B*V, 256, 40, 100] ~ N(0,1)  (CPFPN output, 1600x640 / 16)
  * lidar2img: f = 1266, principal point (800, 190) (900-row image bottom-cropped
    to 640, transform_3d.py:449-457), cameras 1.5 m above the LiDAR origin at the
    given yaws; pad_shape (640, 1600, 3)
  * points [N, 5]: xyz uniform in the point-cloud range, intensity U[0,255],
    time-lag U[0, 0.5]
  * sweeps: a key frame and K sweeps as slices of one raw buffer, each sweep with a seeded rigid
    sensor2lidar transform (yaw within 0.05 rad, up to 0.5 m per sweep of age) and a timestamp 50 ms
    older than the one before; a seeded vehicle2infrastructure matrix for the coop configs
  * weights: the reference's init (xavier decoder, kaiming task heads, cls bias
    -2.19, reference_points U(0,1)), optionally with biases / norm affine
    parameters jittered so every fused epilogue is exercised by the parity tests.
"""
import copy
import math
import os

import numpy as np
import torch

from .config import load_config
from .registry import build_head

__all__ = ["CONFIG_DIR", "make_head_cfg", "build_synthetic_head", "camera_lidar2img", "synthetic_metas",
           "synthetic_bev", "synthetic_img", "synthetic_points", "head_state_dict", "CONFIGS", "make_detector_cfg",
           "synthetic_frames", "synthetic_sweeps", "synthetic_vehicle2infrastructure"]

CONFIG_DIR = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "configs")
CONFIGS = ("cmt_lidar_nus", "cmt_fusion_nus", "cmtcoop_fusion_tumtraf", "cmtcoop_lidar_tumtraf")

NUS_YAWS = (0.0, 55.0, -55.0, 110.0, -110.0, 180.0)
VEHICLE_YAWS = (0.0,)
INFRA_YAWS = (30.0, 150.0, -90.0)


def make_head_cfg(name, num_query=900, num_layers=None, grid_size=None, head_type=None):
    """The ``pts_bbox_head`` dict of a reference config (plus train/test cfg)."""
    base = load_config(os.path.join(CONFIG_DIR, "_decoder.py"))
    c = load_config(os.path.join(CONFIG_DIR, name + ".py"))
    decoder = copy.deepcopy(base["decoder"])
    if num_layers is not None:
        decoder["num_layers"] = num_layers
    classes = c.get("nus_classes") or c.get("tumtraf_classes")
    grid = list(grid_size) if grid_size is not None else list(c["grid_size"])
    head = dict(
        type=head_type or c["head_type"], in_channels=512, hidden_dim=256, downsample_scale=8, num_query=num_query,
        common_heads=copy.deepcopy(base["common_heads"]),
        tasks=[dict(num_class=len(classes), class_names=list(classes))],
        bbox_coder=dict(type="MultiTaskBBoxCoder", post_center_range=c["post_center_range"],
                        pc_range=c["point_cloud_range"], max_num=300, voxel_size=c["voxel_size"],
                        num_classes=len(classes)),
        separate_head=dict(type="SeparateTaskHead", init_bias=-2.19, final_kernel=c["final_kernel"]),
        transformer=dict(type=c["transformer_type"], decoder=decoder),
        # the reference configs' losses (e.g. CMTCoop_TUMTraf/fusion/coop/...py:327-328)
        loss_cls=dict(type="FocalLoss", use_sigmoid=True, gamma=2, alpha=0.25, reduction="mean", loss_weight=2.0),
        loss_bbox=dict(type="L1Loss", reduction="mean", loss_weight=0.25),
        train_cfg=None,
        test_cfg=dict(grid_size=grid, out_size_factor=8, pc_range=c["point_cloud_range"], voxel_size=c["voxel_size"],
                      nms_type=None, max_num=200),
    )
    return head, c


def make_detector_cfg(name, num_query=900, num_layers=None, grid_size=None, spec_name="V-99-eSE"):
    """The whole ``model`` dict of a package config: the head of ``make_head_cfg`` under the feature-extractor
    blocks of the reference configs (e.g. CMT_Nuscenes/fusion/cmt_voxel0075_vov_1600x640_cbgs.py:160-200,
    CMTCoop_TUMTraf/fusion/coop/...py:216-273).  ``grid_size=[X, Y, 40]`` shrinks the scene around the origin
    at the config's voxel size: x, y in +-X vx / 2, +-Y vy / 2, ``sparse_shape = [41, Y, X]``; the voxel layer,
    the middle encoder, the head's ``pc_range`` and ``test_cfg`` then agree.  ``spec_name``: the VoVNet spec.
    One key is not the reference's: the SparseEncoder gets ``capacity_factor=8``, the worst case, because
    ``synthetic_points`` are uniform and isolated, so the strided stages grow the active set where a LiDAR
    sweep shrinks it; the factor sizes buffers only and changes no value."""
    head, c = make_head_cfg(name, num_query=num_query, num_layers=num_layers, grid_size=grid_size)
    vx, vy, _ = c["voxel_size"]
    pcr = list(c["point_cloud_range"])
    grid = list(c["grid_size"])
    if grid_size is not None:
        grid = [int(g) for g in grid_size]
        if len(grid) != 3 or grid[2] != c["grid_size"][2]:
            raise ValueError(f"grid_size must be [X, Y, {c['grid_size'][2]}], got {list(grid_size)}")
        pcr = [-grid[0] * vx / 2, -grid[1] * vy / 2, pcr[2], grid[0] * vx / 2, grid[1] * vy / 2, pcr[5]]
    head["bbox_coder"]["pc_range"] = pcr
    test_cfg = head.pop("test_cfg")
    test_cfg.update(grid_size=grid, pc_range=pcr)
    head.pop("train_cfg")
    fusion = "fusion" in name
    body = dict(type="CmtDetector", use_grid_mask=True)
    if fusion:
        body.update(
            img_backbone=dict(type="VoVNet", spec_name=spec_name, norm_eval=True, frozen_stages=-1, input_ch=3,
                              out_features=("stage4", "stage5")),
            img_neck=dict(type="CPFPN", in_channels=[768, 1024], out_channels=256, num_outs=2))
    voxel_layer = dict(c["pts_voxel_layer"], point_cloud_range=pcr)
    body.update(
        pts_voxel_layer=voxel_layer,
        pts_voxel_encoder=dict(type="HardSimpleVFE", num_features=5),
        pts_middle_encoder=dict(type="SparseEncoder", in_channels=5, sparse_shape=[grid[2] + 1, grid[1], grid[0]],
                                output_channels=128, order=("conv", "norm", "act"),
                                encoder_channels=((16, 16, 32), (32, 32, 64), (64, 64, 128), (128, 128)),
                                encoder_paddings=((0, 0, 1), (0, 0, 1), (0, 0, [0, 1, 1]), (0, 0)),
                                block_type="basicblock", capacity_factor=8.0),
        pts_backbone=dict(type="SECOND", in_channels=256, out_channels=[128, 256], layer_nums=[5, 5],
                          layer_strides=[1, 2], norm_cfg=dict(type="BN", eps=0.001, momentum=0.01),
                          conv_cfg=dict(type="Conv2d", bias=False)),
        pts_neck=dict(type="SECONDFPN", in_channels=[128, 256], out_channels=[256, 256], upsample_strides=[1, 2],
                      norm_cfg=dict(type="BN", eps=0.001, momentum=0.01),
                      upsample_cfg=dict(type="deconv", bias=False), use_conv_for_no_stride=True))
    tail = dict(pts_bbox_head=head, train_cfg=None, test_cfg=dict(pts=test_cfg))
    if name.startswith("cmtcoop"):
        return dict(type="CmtCoopDetector", vehicle_model=body, infrastructure_model=copy.deepcopy(body),
                    coop_fusion_neck=None, **tail)
    return dict(body, **tail)


def synthetic_frames(n, h=900, w=1600, seed=0, device=None):
    """camera frames as cv2 loads them: uint8 [n, h, w, 3], interleaved"""
    g = torch.Generator().manual_seed(seed + 17)
    x = torch.randint(0, 256, (n, h, w, 3), generator=g, dtype=torch.uint8)
    return x.to(device) if device is not None else x


def _jitter_(module, gen, scale=0.05):
    with torch.no_grad():
        for name, p in module.named_parameters():
            if name.endswith("bias") or ("norm" in name and name.endswith("weight")) or ".1.weight" in name:
                p.add_(torch.randn(p.shape, generator=gen) * scale)
        for name, b in module.named_buffers():
            if name.endswith("running_mean"):
                b.copy_(torch.randn(b.shape, generator=gen) * 0.1)
            elif name.endswith("running_var"):
                b.copy_(torch.rand(b.shape, generator=gen) * 0.5 + 0.75)


def build_synthetic_head(name, *, seed=0, num_query=900, num_layers=None, grid_size=None, jitter=True,
                         device=None):
    cfg, meta = make_head_cfg(name, num_query=num_query, num_layers=num_layers, grid_size=grid_size)
    torch.manual_seed(seed)
    head = build_head(cfg)
    head.init_weights()
    if jitter:
        _jitter_(head, torch.Generator().manual_seed(seed + 1))
    head.eval()
    if device is not None:
        head.to(device)
    return head, cfg, meta


def head_state_dict(head):
    return {k: v.detach().float().cpu() for k, v in head.state_dict().items()}


def camera_lidar2img(yaw_deg, height=1.5, f=1266.0, cx=800.0, cy=190.0):
    """4x4 lidar->image projection of a pinhole camera at (0, 0, height)
    looking along yaw (x right, y down, z forward in the camera frame)."""
    t = math.radians(yaw_deg)
    fwd = np.array([math.cos(t), math.sin(t), 0.0])
    right = np.array([math.sin(t), -math.cos(t), 0.0])
    down = np.array([0.0, 0.0, -1.0])
    R = np.stack([right, down, fwd])
    c = np.array([0.0, 0.0, height])
    E = np.eye(4)
    E[:3, :3] = R
    E[:3, 3] = -R @ c
    K = np.eye(4)
    K[0, 0] = K[1, 1] = f
    K[0, 2], K[1, 2] = cx, cy
    return K @ E


def synthetic_metas(B, yaws=NUS_YAWS, pad_shape=(640, 1600, 3), prefix="", seed=0, extra=None):
    """img_metas with ``lidar2img`` (intrinsics scaled to pad_shape from the
    1600x640 nuScenes crop) and ``pad_shape``; ``prefix`` = '' / 'vehicle_' /
    'infrastructure_' (the coop meta convention, cmt_head_coop.py:41-69)."""
    rng = np.random.default_rng(seed)
    sx, sy = pad_shape[1] / 1600.0, pad_shape[0] / 640.0
    metas = []
    for _ in range(B):
        # small per-frame extrinsic jitter so batch entries differ
        l2i = [camera_lidar2img(y + rng.uniform(-2, 2), height=1.5 + rng.uniform(-0.1, 0.1), f=1266.0 * sx,
                                cx=800.0 * sx, cy=190.0 * sy) for y in yaws]
        m = {prefix + "lidar2img": l2i, prefix + "pad_shape": [pad_shape] * len(yaws)}
        metas.append(m)
    if extra is not None:
        for m, e in zip(metas, extra):
            m.update(e)
    return metas


def synthetic_bev(B, H=180, W=180, C=512, seed=0, device=None):
    g = torch.Generator().manual_seed(seed)
    x = torch.relu(torch.randn((B, C, H, W), generator=g))
    return x.to(device) if device is not None else x


def synthetic_img(BV, h=40, w=100, C=256, seed=0, device=None):
    g = torch.Generator().manual_seed(seed + 7)
    x = torch.randn((BV, C, h, w), generator=g)
    return x.to(device) if device is not None else x


def synthetic_gt(B, pc_range, num_classes, n=20, seed=0, device=None):
    """Training targets (20 boxes per frame):
    gravity-centre boxes [n, 9] (x, y, z, w, l, h, yaw, vx, vy) inside the
    central 70 % of the range, dims 1-4 m, and labels < num_classes."""
    g = torch.Generator().manual_seed(seed + 29)
    boxes, labels = [], []
    lo, hi = torch.tensor(pc_range[:3]), torch.tensor(pc_range[3:])
    for _ in range(B):
        c = lo + (hi - lo) * (0.15 + 0.7 * torch.rand(n, 3, generator=g))
        d = 1.0 + 3.0 * torch.rand(n, 3, generator=g)
        yaw = (torch.rand(n, 1, generator=g) * 2 - 1) * math.pi
        vel = torch.randn(n, 2, generator=g)
        b = torch.cat([c, d, yaw, vel], 1)
        l = torch.randint(0, num_classes, (n,), generator=g)
        boxes.append(b.to(device) if device is not None else b)
        labels.append(l.to(device) if device is not None else l)
    return boxes, labels


def synthetic_points(N, pc_range, seed=0, device=None, margin=0.0):
    g = torch.Generator().manual_seed(seed + 13)
    lo = torch.tensor(pc_range[:3], dtype=torch.float32) - margin
    hi = torch.tensor(pc_range[3:], dtype=torch.float32) + margin
    xyz = lo + torch.rand((N, 3), generator=g) * (hi - lo)
    inten = torch.rand((N, 1), generator=g) * 255.0
    dt = torch.rand((N, 1), generator=g) * 0.5
    p = torch.cat([xyz, inten, dt], 1)
    return p.to(device) if device is not None else p


def _rigid(g, max_yaw, max_trans, max_z):
    """a seeded rigid transform as float64 numpy: yaw within max_yaw, x / y within max_trans, z within max_z"""
    u = torch.rand(4, generator=g, dtype=torch.float64).numpy() * 2.0 - 1.0
    c, s = math.cos(u[0] * max_yaw), math.sin(u[0] * max_yaw)
    rot = np.array([[c, -s, 0.0], [s, c, 0.0], [0.0, 0.0, 1.0]])
    return rot, np.array([u[1] * max_trans, u[2] * max_trans, u[3] * max_z])


def synthetic_sweeps(K, N, pc_range, seed=0, device=None, margin=0.0):
    """One cloud as the loaders hold it -> (key_points, sweeps, key_ts) for native_pts.sweep_segments: the key frame
    [N, 5] and K sweeps of N points each, all slices of one raw buffer [(1 + K) N, 5] (``synthetic_points`` with
    ``margin``, so a range filter has something to drop), ``sweeps`` as the info files list them (``points``,
    ``sensor2lidar_rotation`` 3 x 3 and ``sensor2lidar_translation`` float64, ``timestamp`` in microseconds, 50 ms
    apart), ``key_ts`` the key frame's timestamp."""
    raw = synthetic_points((1 + K) * N, pc_range, seed=seed, device=device, margin=margin)
    g = torch.Generator().manual_seed(seed + 29)
    key_ts = 1_600_000_000_000_000 + 100_000 * seed
    sweeps = []
    for k in range(K):
        rot, trans = _rigid(g, 0.05, 0.5 * (k + 1), 0.05)
        sweeps.append(dict(points=raw[(k + 1) * N:(k + 2) * N], sensor2lidar_rotation=rot,
                           sensor2lidar_translation=trans, timestamp=key_ts - 50_000 * (k + 1)))
    return raw[:N], sweeps, key_ts


def synthetic_vehicle2infrastructure(seed=0):
    """a seeded 4 x 4 vehicle -> infrastructure matrix (float64): any yaw, up to 10 m in x / y, 0.5 m in z"""
    rot, trans = _rigid(torch.Generator().manual_seed(seed + 31), math.pi, 10.0, 0.5)
    m = np.eye(4)
    m[:3, :3], m[:3, 3] = rot, trans
    return m


def moving_scene(seed, n_objects=12, frames=30, dt=0.1, grid_cols=4, spacing=10.0, max_speed=1.0, noise=0.2,
                 p_drop=0.1, max_drop_run=2, n_false=2, false_margin=5.0, num_classes=3, pad_to=None, with_truth=False):
    """A seeded scene of moving boxes for the tracker (native_track.Tracker), as numpy on the host.

    ``n_objects`` objects start on a grid of ``grid_cols`` columns ``spacing`` metres apart and move with constant
    velocities of at most ``max_speed`` m/s in random directions.  Per frame (``dt`` seconds apart): a detection
    of every object whose position is within +-``noise`` metres (uniform, per axis) of the truth, dropped with
    probability ``p_drop`` but never more than ``max_drop_run`` frames running; ``n_false`` false boxes at least
    ``false_margin`` metres from every object; the rows shuffled.  Scores of the objects' boxes lie in
    [0.5, 0.9], of the false ones in [0.35, 0.5].
    -> a list of dicts: ``boxes`` fp32 [n, 9] (x y z dx dy dz yaw vx vy), ``scores`` fp32 [n], ``labels`` int32 [n],
    ``object`` int32 [n] (the object of a row, -1 for a false box), ``timestamp`` (seconds, float).  With
    ``pad_to`` every array has ``pad_to`` rows (zeros beyond ``count``, ``object`` -1) and ``count`` is n.  With
    ``with_truth`` every frame also has the true state of every object, dropped ones included: ``gt_boxes`` fp32
    [n_objects, 9], ``gt_labels`` int32 and ``gt_ids`` int32 (the object's index); it draws no random number, so the
    other keys are the same bytes with and without it."""
    rng = np.random.RandomState(seed)
    idx = np.arange(n_objects)
    pos0 = np.stack([(idx % grid_cols) * spacing, (idx // grid_cols) * spacing, np.zeros(n_objects)], 1)
    ang, speed = rng.uniform(-math.pi, math.pi, n_objects), rng.uniform(0.0, max_speed, n_objects)
    vel = np.stack([speed * np.cos(ang), speed * np.sin(ang)], 1)
    size = rng.uniform([3.5, 1.6, 1.4], [5.0, 2.1, 1.9], (n_objects, 3))
    label = (idx % num_classes).astype(np.int32)
    lo, hi = pos0[:, :2].min(0) - 3 * false_margin, pos0[:, :2].max(0) + 3 * false_margin
    run = np.zeros(n_objects, np.int64)
    out = []
    for t in range(frames):
        truth = pos0.copy()
        truth[:, :2] += vel * (t * dt)
        drop = rng.uniform(size=n_objects) < p_drop
        drop &= run < max_drop_run
        run = np.where(drop, run + 1, 0)
        keep = np.nonzero(~drop)[0]
        b = np.zeros((len(keep) + n_false, 9))
        b[:len(keep), :3] = truth[keep]
        b[:len(keep), :2] += rng.uniform(-noise, noise, (len(keep), 2))
        b[:len(keep), 3:6] = size[keep]
        b[:len(keep), 6] = np.arctan2(vel[keep, 1], vel[keep, 0])
        b[:len(keep), 7:9] = vel[keep]
        s = np.concatenate([rng.uniform(0.5, 0.9, len(keep)), rng.uniform(0.35, 0.5, n_false)])
        lab = np.concatenate([label[keep], rng.randint(0, num_classes, n_false).astype(np.int32)])
        obj = np.concatenate([keep, np.full(n_false, -1)]).astype(np.int32)
        for k in range(n_false):
            for _ in range(1000):   # bounded rejection sampling; the area is mostly free
                c = rng.uniform(lo, hi)
                if np.hypot(*(truth[:, :2] - c).T).min() >= false_margin:
                    break
            b[len(keep) + k] = [c[0], c[1], 0.0, 4.0, 1.8, 1.6, rng.uniform(-math.pi, math.pi), 0.0, 0.0]
        order = rng.permutation(len(b))
        b, s, lab, obj = b[order].astype(np.float32), s[order].astype(np.float32), lab[order], obj[order]
        n = len(b)
        if pad_to is not None:
            if pad_to < n:
                raise ValueError(f"pad_to {pad_to} below the frame's {n} rows")
            pad = pad_to - n
            b = np.concatenate([b, np.zeros((pad, 9), np.float32)])
            s = np.concatenate([s, np.zeros(pad, np.float32)])
            lab = np.concatenate([lab, np.zeros(pad, np.int32)])
            obj = np.concatenate([obj, np.full(pad, -1, np.int32)])
        out.append(dict(boxes=b, scores=s, labels=lab.astype(np.int32), object=obj, count=n, timestamp=t * dt))
        if with_truth:
            g = np.zeros((n_objects, 9))
            g[:, :3], g[:, 3:6], g[:, 6], g[:, 7:9] = truth, size, np.arctan2(vel[:, 1], vel[:, 0]), vel
            out[-1].update(gt_boxes=g.astype(np.float32), gt_labels=label.copy(), gt_ids=idx.astype(np.int32))
    return out
