"""The point side of the test pipeline on the device: cmt_pts_prepare (include/cmt_hip.h) and the host helpers
that restate the reference's choices around it.

``prepare_points`` takes one cloud's raw sweep buffers (the key frame and its sweeps, as they are read from
disk) and returns the detector's ``points``: remove_close, the sweep -> key-frame transform, the time column,
the ``use_dim`` selection, the agent transform (VehiclePointsToInfraCoords) and the range filter in two
launches with no host read.  The result is padded: kept rows first, in the reference's order, the rest NaN,
plus a device count.  The voxelizer drops non-finite points and keeps input order, so the padded buffer
voxelizes exactly like the trimmed one and goes to ``CmtDetector`` / ``voxelize_batch`` as it is.

Like native_img.py: argument checks raise ValueError before the device check, tensors must live on a HIP
device, there is no CPU fallback and no wrapper synchronises with the host (``trim=True`` excepted).
"""
import ctypes
import math

import numpy as np
import torch

from . import native as N
from .native import _check, _p, _stream, lib

__all__ = ["MAX_SEGMENTS", "PointsWorkspace", "tile_rows", "workspace_bytes", "prepare_points", "sweep_segments",
           "points_plan_from_config", "lidar2img_to_infra"]

MAX_SEGMENTS = N.PTS_MAX_SEG


def tile_rows():
    """rows per workgroup tile of cmt_pts_prepare"""
    return int(lib().cmt_pts_prepare_tile_rows())


def workspace_bytes(n_total):
    return int(lib().cmt_pts_prepare_workspace_bytes(int(n_total)))


class PointsWorkspace:
    """Holder of cmt_pts_prepare's workspace (the per-tile counts), grown on demand and reused: every call
    rewrites what it reads, so nothing is cleaned between calls.  One stream at a time."""

    def __init__(self):
        self._ws = None

    def get(self, nbytes, device):
        if self._ws is None or self._ws.device != device or self._ws.numel() * 4 < nbytes:
            cap = 1024
            while cap * 4 < nbytes:
                cap <<= 1
            self._ws = torch.empty(cap, dtype=torch.int32, device=device)
        return self._ws


_DEFAULT_WS = PointsWorkspace()
_EYE3, _ZERO3 = np.eye(3), np.zeros(3)


def _segment_fields(i, seg, load_dim):
    """checked host-side fields of one segment dict -> (points, rot64 | None, trans64 | None, radius, time_col, time)"""
    if not isinstance(seg, dict) or "points" not in seg:
        raise ValueError(f"segment {i} must be a dict with a 'points' tensor")
    unknown = set(seg) - {"points", "rotation", "translation", "remove_close", "time_col", "time"}
    if unknown:
        raise ValueError(f"segment {i}: unknown keys {sorted(unknown)}")
    pts = seg["points"]
    if not torch.is_tensor(pts) or pts.dtype != torch.float32 or pts.dim() != 2 or pts.shape[1] != load_dim:
        raise ValueError(f"segment {i}: points must be an fp32 [n, {load_dim}] tensor, got "
                         f"{(pts.dtype, tuple(pts.shape)) if torch.is_tensor(pts) else type(pts)}")
    if not pts.is_contiguous():
        raise ValueError(f"segment {i}: points must be contiguous rows")
    rot, trans = seg.get("rotation"), seg.get("translation")
    if rot is not None or trans is not None:
        rot = _EYE3 if rot is None else np.asarray(rot, dtype=np.float64)
        trans = _ZERO3 if trans is None else np.asarray(trans, dtype=np.float64).reshape(-1)
        if rot.shape != (3, 3) or trans.shape != (3,):
            raise ValueError(f"segment {i}: rotation must be 3 x 3 and translation 3 values")
        if not math.isfinite(rot.sum() + trans.sum()):   # a NaN or an inf survives the sums
            raise ValueError(f"segment {i}: non-finite sweep transform")
    rc = seg.get("remove_close", 0.0)
    radius = 1.0 if rc is True else float(rc or 0.0)   # True: the reference's _remove_close default radius
    if not np.isfinite(radius) or radius < 0:
        raise ValueError(f"segment {i}: remove_close must be a finite radius >= 0, got {rc!r}")
    tc = seg.get("time_col")
    tc = -1 if tc is None else int(tc)
    if tc < -1 or tc >= load_dim:
        raise ValueError(f"segment {i}: time_col {tc} outside [0, {load_dim})")
    tv = seg.get("time")
    if tc >= 0 and tv is None:
        raise ValueError(f"segment {i}: time_col without a time value")
    return pts, rot, trans, radius, tc, 0.0 if tv is None else float(tv)   # the struct's float field rounds to float32


def _one_buffer(parts):
    """the tensors as one [n_total, load_dim] source: the first one's address when they already lie back to back in
    memory (slices of one raw buffer; the caller's list keeps them alive), their concatenation otherwise
    -> (address, the tensor that owns it)"""
    end = parts[0].data_ptr()
    for t in parts:
        if t.numel():
            if t.data_ptr() != end:
                cat = torch.cat(parts, 0)
                return cat.data_ptr(), cat
            end += t.numel() * 4
    return parts[0].data_ptr(), parts[0]


def prepare_points(segments, *, use_dim, load_dim=5, agent_transform=None, point_cloud_range=None, out=None,
                   workspace=None, trim=False):
    """cmt_pts_prepare for one cloud -> (points_padded [n_total, F_out] fp32, count [1] int32), both on the device:
    rows [0, count) are the reference's points in its order (key frame, then the sweeps), rows [count, n_total)
    are NaN.  No host read: the pair goes to ``voxelize_batch`` / ``CmtDetector`` as it is.

    ``segments``: 1 to 16 dicts ``dict(points=fp32 [n, load_dim] tensor, rotation=None | 3 x 3,
    translation=None | 3, remove_close=0.0, time_col=None, time=None)`` as ``sweep_segments`` builds them;
    ``rotation`` / ``translation`` are the sweep's float64 sensor2lidar pair, ``remove_close`` a radius (True: 1.0),
    ``time`` the value written to column ``time_col``.  Segments that are consecutive slices of one raw buffer are
    used in place; anything else is concatenated first (one copy).
    ``use_dim``: the output columns (an int k means range(k)); must start with 0, 1, 2.
    ``agent_transform``: None, a 4 x 4 (or 3 x 4) vehicle2infrastructure matrix, or (rotation 3 x 3, translation 3);
    applied in float32 as VehiclePointsToInfraCoords does.  ``point_cloud_range``: None or 6 values, the strict
    filter of PointsRangeFilter.  ``out``: an fp32 [n_total, F_out] buffer to write; ``workspace``: a
    PointsWorkspace or an int32 tensor of at least ``workspace_bytes(n_total)`` bytes (default: one holder of this
    module).  ``trim=True`` returns ``points_padded[:count]`` instead of the pair; that is a host read."""
    segments = list(segments)
    if not 1 <= len(segments) <= MAX_SEGMENTS:
        raise ValueError(f"1 to {MAX_SEGMENTS} segments required, got {len(segments)}")
    load_dim = int(load_dim)
    if not 3 <= load_dim <= 8:
        raise ValueError(f"load_dim must be 3..8, got {load_dim}")
    use = list(range(use_dim)) if isinstance(use_dim, int) else [int(u) for u in use_dim]
    if not 3 <= len(use) <= 8 or use[:3] != [0, 1, 2] or any(u < 0 or u >= load_dim for u in use):
        raise ValueError(f"use_dim must hold 3..8 columns below load_dim {load_dim} and start with 0, 1, 2, got {use}")
    fields = [_segment_fields(i, s, load_dim) for i, s in enumerate(segments)]
    a = N.PtsPrepareArgs()
    a.S, a.load_dim, a.F_out = len(fields), load_dim, len(use)
    for j, u in enumerate(use):
        a.use_dim[j] = u
    start = 0
    for i, (pts, rot, trans, radius, tc, tv) in enumerate(fields):
        a.seg_start[i] = start
        start += int(pts.shape[0])
        g = a.seg[i]
        g.has_sweep_xform = int(rot is not None)
        if rot is not None:
            g.rot[:] = rot.ravel().tolist()
            g.trans[:] = trans.tolist()
        g.close_radius, g.time_col, g.time_val = radius, tc, tv
    n_total = start
    for i in range(len(fields), MAX_SEGMENTS + 1):
        a.seg_start[i] = n_total
    if n_total >= 2 ** 31:
        raise ValueError("n_total must be below 2^31")
    a.n_total = n_total
    if agent_transform is not None:
        if isinstance(agent_transform, (tuple, list)) and len(agent_transform) == 2:
            r, t = np.asarray(agent_transform[0]), np.asarray(agent_transform[1]).reshape(-1)
        else:
            m = np.asarray(agent_transform)
            if m.shape not in ((4, 4), (3, 4)):
                raise ValueError(f"agent_transform must be 4 x 4, 3 x 4 or (rotation, translation), got {m.shape}")
            r, t = m[:3, :3], m[:3, 3]
        r32, t32 = r.astype(np.float32), t.astype(np.float32)   # new_tensor on a float32 cloud
        if r32.shape != (3, 3) or t32.shape != (3,) or not (np.isfinite(r32).all() and np.isfinite(t32).all()):
            raise ValueError("agent_transform must be a finite 3 x 3 rotation and 3 translation values")
        a.has_agent_xform = 1
        a.rot32[:] = r32.ravel().tolist()
        a.trans32[:] = t32.tolist()
    if point_cloud_range is not None:
        rng = np.asarray(point_cloud_range, dtype=np.float32).reshape(-1)
        if rng.shape != (6,) or not np.isfinite(rng).all() or not (rng[:3] < rng[3:]).all():
            raise ValueError(f"point_cloud_range must be 6 finite values with min < max, got {point_cloud_range!r}")
        a.has_range = 1
        a.range[:] = rng.tolist()
    parts = [f[0] for f in fields]
    dev = parts[0].device
    if any(not t.is_cuda for t in parts):
        raise ValueError("points must live on a HIP device (no CPU path)")
    if any(t.device != dev for t in parts):
        raise ValueError("all segments must live on one device")
    if out is not None:
        if (not torch.is_tensor(out) or out.dtype != torch.float32 or tuple(out.shape) != (n_total, len(use))
                or not out.is_contiguous() or out.device != dev):
            raise ValueError(f"out must be a contiguous fp32 {(n_total, len(use))} tensor on the points' device")
    need = workspace_bytes(n_total)
    if workspace is None:
        workspace = _DEFAULT_WS
    if isinstance(workspace, PointsWorkspace):
        ws = workspace.get(need, dev)
    else:
        ws = workspace
        if (not torch.is_tensor(ws) or ws.dtype != torch.int32 or not ws.is_contiguous() or ws.device != dev
                or ws.numel() * 4 < need):
            raise ValueError(f"workspace must be a contiguous int32 tensor of at least {need} bytes on the points' device")
    src_ptr, src = _one_buffer(parts)   # src keeps a concatenation alive until the launch is queued
    dst = out if out is not None else torch.empty((n_total, len(use)), dtype=torch.float32, device=dev)
    count = torch.empty(1, dtype=torch.int32, device=dev)
    a.src, a.dst, a.count = src_ptr, _p(dst), _p(count)
    a.workspace, a.workspace_bytes = _p(ws), ws.numel() * 4
    _check(lib().cmt_pts_prepare(ctypes.byref(a), _stream()), "cmt_pts_prepare")
    if trim:
        return dst[:int(count.item())]   # a host read
    return dst, count


def sweep_segments(key_points, sweeps, key_ts, *, time_dim=4, remove_close=False, sweeps_num=10, test_mode=True,
                   pad_empty_sweeps=False, coop=False, reduce_beams=False, load_augmented=False):
    """The segments of one cloud as LoadPointsFromMultiSweeps[Coop].__call__ chooses them (loading_coop.py:193-298),
    for ``prepare_points``.

    ``key_points``: the key frame's raw rows; ``key_ts`` its timestamp in microseconds; ``sweeps``: the info
    file's list of ``dict(points=raw rows, sensor2lidar_rotation, sensor2lidar_translation, timestamp)`` with the
    file already read into ``points``.  The key frame comes first with column ``time_dim`` set to 0.  Without
    sweeps and with ``pad_empty_sweeps`` the key frame is repeated ``sweeps_num`` times (each copy through
    remove_close when that is on).  Otherwise all sweeps are taken when there are at most ``sweeps_num``, the
    first ``sweeps_num`` in test mode; each gets remove_close (radius 1.0), its sensor2lidar transform and the
    time lag float32(key_ts / 1e6 - timestamp / 1e6) in column ``time_dim`` (``coop``: column 4 whatever
    ``time_dim`` is, as the coop loader hard-codes it).  The random choice of training mode, ``reduce_beams``
    and ``load_augmented`` are training-only or dead code there and raise NotImplementedError."""
    if reduce_beams or load_augmented:
        raise NotImplementedError("reduce_beams / load_augmented are not part of the test pipeline")
    sweeps = list(sweeps)
    radius = 1.0 if remove_close else 0.0
    ts = key_ts / 1e6
    segs = [dict(points=key_points, time_col=int(time_dim), time=0.0)]
    if pad_empty_sweeps and len(sweeps) == 0:
        segs += [dict(points=key_points, remove_close=radius, time_col=int(time_dim), time=0.0)
                 for _ in range(int(sweeps_num))]
        return segs
    if len(sweeps) <= sweeps_num:
        chosen = sweeps
    elif test_mode:
        chosen = sweeps[:int(sweeps_num)]
    else:
        raise NotImplementedError("the random sweep choice of training mode is not built")
    for sw in chosen:
        lag = np.float32(ts - sw["timestamp"] / 1e6)
        segs.append(dict(points=sw["points"], rotation=sw["sensor2lidar_rotation"],
                         translation=sw["sensor2lidar_translation"], remove_close=radius,
                         time_col=4 if coop else int(time_dim), time=float(lag)))
    return segs


def _pipeline_steps(steps):
    for st in steps or []:
        if isinstance(st, dict):
            yield st
            yield from _pipeline_steps(st.get("transforms"))


def points_plan_from_config(cfg):
    """The point preparation of a config dict (config.load_config): the LoadPointsFromFile[Coop],
    LoadPointsFromMultiSweeps[Coop], VehiclePointsToInfraCoords and PointsRangeFilter[Coop] steps of
    ``data.test.pipeline``, looked for inside MultiScaleFlipAug3D's ``transforms`` too -> dict(load_dim, use_dim,
    sweeps_num, remove_close, time_dim, point_cloud_range, coop); None for a pipeline that loads no points (camera
    only).  ``sweeps_num`` is 0 without a multi-sweep step, ``point_cloud_range`` None without a range filter (the
    nuScenes test pipelines have none), ``coop`` tells that the vehicle cloud is moved into the infrastructure
    frame.  A GlobalRotScaleTrans[Coop] step with the identity ranges of every test pipeline (rot_range [0, 0],
    scale_ratio_range [1, 1], translation_std 0) multiplies by 1 and adds 0 and is skipped; any other raises."""
    steps = list(_pipeline_steps(cfg["data"]["test"]["pipeline"]))

    def find(kind):
        hits = [st for st in steps if st.get("type") in (kind, kind + "Coop")]
        return hits[0] if hits else None

    load = find("LoadPointsFromFile")
    if load is None:
        return None
    load_dim = int(load.get("load_dim", 6))
    use = load.get("use_dim", [0, 1, 2])
    use = list(range(use)) if isinstance(use, int) else [int(u) for u in use]
    plan = dict(load_dim=load_dim, use_dim=use, sweeps_num=0, remove_close=False, time_dim=4,
                point_cloud_range=None, coop=find("VehiclePointsToInfraCoords") is not None)
    ms = find("LoadPointsFromMultiSweeps")
    if ms is not None:
        if use != list(range(load_dim)):
            raise ValueError(f"the file loader's use_dim {use} drops columns in front of the multi-sweep step")
        ms_dim = int(ms.get("load_dim", 5))
        if ms_dim != load_dim:
            raise ValueError(f"the multi-sweep step loads {ms_dim} columns, the file loader {load_dim}")
        mu = ms.get("use_dim", [0, 1, 2, 4])
        plan.update(use_dim=list(range(mu)) if isinstance(mu, int) else [int(u) for u in mu],
                    sweeps_num=int(ms.get("sweeps_num", 10)), remove_close=bool(ms.get("remove_close", False)),
                    time_dim=int(ms.get("time_dim", 4)))
    for st in steps:
        if st.get("type") in ("GlobalRotScaleTrans", "GlobalRotScaleTransCoop"):
            rot = st.get("rot_range", [-0.78539816, 0.78539816])
            rot = [-rot, rot] if isinstance(rot, (int, float)) else list(rot)
            scale = list(st.get("scale_ratio_range", [0.95, 1.05]))
            std = st.get("translation_std", [0, 0, 0])
            std = [std] * 3 if isinstance(std, (int, float)) else list(std)
            if any(v != 0 for v in rot) or any(v != 1 for v in scale) or any(v != 0 for v in std):
                raise ValueError(f"the test pipeline's {st['type']} is not the identity: rot_range {rot}, "
                                 f"scale_ratio_range {scale}, translation_std {std}")
    flt = find("PointsRangeFilter")
    if flt is not None:
        plan["point_cloud_range"] = [float(v) for v in flt["point_cloud_range"]]
    return plan


def lidar2img_to_infra(lidar2img, vehicle2infrastructure):
    """TransformLidar2ImgToInfraCoords (transforms_3d_coop.py:214-222) for one matrix or a stack of them:
    ``M @ inv(vehicle2infrastructure)`` in float64 (the vehicle cameras' lidar2img / lidar2cam once the vehicle
    cloud lives in the infrastructure frame).  The inputs are not modified."""
    m = np.asarray(lidar2img, dtype=np.float64)
    v2i = np.asarray(vehicle2infrastructure, dtype=np.float64)
    if m.shape[-2:] != (4, 4) or v2i.shape != (4, 4):
        raise ValueError(f"4 x 4 matrices required, got {m.shape} and {v2i.shape}")
    return m @ np.linalg.inv(v2i)
