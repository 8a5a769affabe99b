"""The ground-truth database on the device: cmt_gtdb_extract, cmt_gtdb_gather and cmt_gtdb_collide
(include/cmt_hip.h), and around them what ``create_groundtruth_database`` and ``UnifiedDataBaseSampler`` do in the
reference, without the files.

``GtDatabase.add_frame`` cuts the points of every annotated box out of a cloud that is already on the device
(``prepare_points``' output) and appends them as segments of one device buffer, with the reference's ``db_info``
record per object and, with frames and ``lidar2img``, the image crop ``find_img_crop`` would have saved.
``UnifiedDataBaseSampler.sample_all`` draws candidates in the reference's order of random draws, runs the BEV
collision test and its greedy loop for all classes in one launch, and gathers the kept objects' points in a second
one: its ``points`` / ``gt_bboxes_3d`` are the ``paste_points`` / ``paste_boxes`` of ``native_aug.augment_points``,
its ``images`` the ``patches`` of ``native_imgaug.paste_images``.  Files stay out of scope.

Like native_aug.py: argument checks raise ValueError before the device check, tensors must live on a HIP device,
there is no CPU fallback.  The kernels' wrappers never synchronise with the host; ``add_frame`` reads one small
table per frame and ``sample_all`` one per call, as their docstrings say.
"""
import ctypes

import numpy as np
import torch

from . import native as N
from ._argcheck import count_word as _count_word, rows as _rows, same_device, tensor
from .native import _check, _p, _stream, lib
from .native_aug import _SAMPLERS
from .native_pts import PointsWorkspace, _pipeline_steps

__all__ = ["MAX_FRAME_BOXES", "MAX_COLLIDE_BOXES", "MAX_PASTE_BOXES", "workspace_bytes", "extract_objects",
           "gather_objects", "collide", "box_corners", "crop_plan", "BatchSampler", "GtDatabase",
           "UnifiedDataBaseSampler", "db_sampler_from_config"]

MAX_FRAME_BOXES = N.GTDB_MAX_BOXES
MAX_COLLIDE_BOXES = N.GTDB_MAX_COLLIDE
MAX_PASTE_BOXES = N.AUG_MAX_BOXES
_DEFAULT_WS = PointsWorkspace()


def workspace_bytes(n_points, n_boxes):
    return int(lib().cmt_gtdb_extract_workspace_bytes(int(n_points), int(n_boxes)))


def _on_device(dev, **tensors):
    same_device(dev, "the database needs tensors", **tensors)


def extract_objects(points, boxes, count=None, out=None, workspace=None):
    """cmt_gtdb_extract for one frame -> (rows fp32 [cap, F], offsets int32 [M + 1]), both on the device.

    ``points``: fp32 [N, F], F 3..8, with the optional device ``count`` (the padded pair of ``prepare_points``);
    ``boxes``: fp32 [M, 7 | 9] LiDAR boxes, M <= 1024.  Segment b, rows [offsets[b], offsets[b + 1]), holds the
    points inside box b in cloud order with the box's bottom centre subtracted from columns 0..2
    (``points[point_indices[:, b]]`` of create_groundtruth_database); a point inside two boxes is in both.
    ``offsets[M]`` is the uncapped total: rows at or beyond ``cap`` are not written.  ``out``: the destination
    (contiguous fp32 [cap, F], a slice of a larger buffer will do); None allocates N rows, which is enough
    unless boxes overlap.  ``workspace``: as ``prepare_points``.  No host read."""
    points = _rows(points, "points", range(3, 9))
    boxes = _rows(boxes, "boxes", (7, 9))
    count = _count_word(count)
    n, m, F = int(points.shape[0]), int(boxes.shape[0]), int(points.shape[1])
    if m > MAX_FRAME_BOXES:
        raise ValueError(f"at most {MAX_FRAME_BOXES} boxes, got {m}")
    if n >= 2 ** 31 or n * m >= 2 ** 31:
        raise ValueError("N and N * M must be below 2^31")
    if out is not None:
        if (not torch.is_tensor(out) or out.dtype != torch.float32 or out.dim() != 2 or out.shape[1] != F
                or not out.is_contiguous() or out.shape[0] >= 2 ** 31):
            raise ValueError(f"out must be a contiguous fp32 [cap, {F}] tensor")
    dev = points.device
    _on_device(dev, boxes=boxes, count=count, out=out)
    need = workspace_bytes(n, m)
    if workspace is None:
        workspace = _DEFAULT_WS
    if isinstance(workspace, PointsWorkspace):
        ws = workspace.get(need, dev)
    else:
        ws = workspace
        if (not torch.is_tensor(ws) or ws.dtype != torch.int32 or not ws.is_contiguous() or ws.device != dev
                or ws.numel() * 4 < need):
            raise ValueError(f"workspace must be a contiguous int32 tensor of at least {need} bytes on the points' device")
    rows = out if out is not None else torch.empty((n, F), dtype=torch.float32, device=dev)
    offsets = torch.empty(m + 1, dtype=torch.int32, device=dev)
    a = N.GtdbExtractArgs()
    a.N, a.cap, a.M, a.F, a.D = n, int(rows.shape[0]), m, F, int(boxes.shape[1])
    a.points, a.count_in, a.boxes = _p(points), _p(count), _p(boxes)
    a.rows, a.offsets, a.workspace, a.workspace_bytes = _p(rows), _p(offsets), _p(ws), ws.numel() * 4
    _check(lib().cmt_gtdb_extract(ctypes.byref(a), _stream()), "cmt_gtdb_extract")
    return rows, offsets


def gather_objects(rows, seg_offset, seg_len, dst_offset, centre, n_dst, out=None):
    """cmt_gtdb_gather -> fp32 [n_dst, F] on the device: for every k, rows [seg_offset[k], + seg_len[k]) of ``rows``
    go to rows [dst_offset[k], ...) of the result with ``centre[k]`` added to columns 0..2
    (``s_points.translate(info['box3d_lidar'][:3])``).  The three tables are device int32 [K], ``centre`` device
    fp32 [K, 3], K <= 128.  The caller lays the segments out without overlap; rows of the result that no segment
    covers are left as allocated.  No host read."""
    rows = _rows(rows, "rows", range(3, 9))
    F = int(rows.shape[1])
    if not torch.is_tensor(seg_offset) or seg_offset.dim() != 1:
        raise ValueError("seg_offset must be an int32 [K] tensor")
    K = int(seg_offset.shape[0])
    if K > MAX_PASTE_BOXES:
        raise ValueError(f"at most {MAX_PASTE_BOXES} segments, got {K}")
    seg_offset, seg_len, dst_offset = (tensor(t, nm, torch.int32, (K,)) for t, nm in (
        (seg_offset, "seg_offset"), (seg_len, "seg_len"), (dst_offset, "dst_offset")))
    centre = tensor(centre, "centre", torch.float32, (K, 3))
    n_dst = int(n_dst)
    if n_dst < 0 or n_dst >= 2 ** 31 or rows.shape[0] >= 2 ** 31:
        raise ValueError("n_dst and len(rows) must be in [0, 2^31)")
    if out is not None:
        tensor(out, "out", torch.float32, (n_dst, F))
    dev = rows.device
    _on_device(dev, seg_offset=seg_offset, seg_len=seg_len, dst_offset=dst_offset, centre=centre, out=out)
    dst = out if out is not None else torch.empty((n_dst, F), dtype=torch.float32, device=dev)
    a = N.GtdbGatherArgs()
    a.n_rows, a.n_dst, a.K, a.F = int(rows.shape[0]), n_dst, K, F
    a.rows, a.seg_offset, a.seg_len, a.dst_offset = _p(rows), _p(seg_offset), _p(seg_len), _p(dst_offset)
    a.centre, a.dst = _p(centre), _p(dst)
    _check(lib().cmt_gtdb_gather(ctypes.byref(a), _stream()), "cmt_gtdb_gather")
    return dst


def _group_array(group, n_s):
    g = np.ascontiguousarray(np.asarray(group, dtype=np.int64).reshape(-1))
    if g.shape[0] != n_s:
        raise ValueError(f"group must have one entry per candidate ({n_s}), got {g.shape[0]}")
    if n_s and (np.diff(g) < 0).any():
        raise ValueError("group must not decrease")
    if n_s and (g.min() < -2 ** 31 or g.max() >= 2 ** 31):
        raise ValueError("group entries must fit int32")
    return g.astype(np.int32)


def collide(boxes, n_gt, group):
    """cmt_gtdb_collide -> (keep int32 [n_s], count int32 [1]) on the device.

    ``boxes``: fp32 [n, 7 | 9] on the device, n <= 512: ``n_gt`` boxes to avoid followed by the candidates;
    ``group``: a HOST sequence of n - n_gt non-decreasing ints, the ``sample_class_v2`` call (the class) each
    candidate belongs to.  A candidate is rejected iff its BEV rectangle collides (``box_collision_test``) with a
    box to avoid, a kept candidate of an earlier group, or a not yet rejected candidate of its own group.
    No host read."""
    boxes = _rows(boxes, "boxes", (7, 9))
    n, n_gt = int(boxes.shape[0]), int(n_gt)
    if n > MAX_COLLIDE_BOXES:
        raise ValueError(f"at most {MAX_COLLIDE_BOXES} boxes, got {n}")
    if n_gt < 0 or n_gt > n:
        raise ValueError(f"n_gt must be in [0, {n}], got {n_gt}")
    g = _group_array(group, n - n_gt)
    dev = boxes.device
    _on_device(dev)
    keep = torch.empty(n - n_gt, dtype=torch.int32, device=dev)
    cnt = torch.empty(1, dtype=torch.int32, device=dev)
    a = N.GtdbCollideArgs()
    a.n_gt, a.n_s, a.D = n_gt, n - n_gt, int(boxes.shape[1])
    a.boxes, a.group, a.keep, a.count = _p(boxes), ctypes.c_void_p(g.ctypes.data), _p(keep), _p(cnt)
    _check(lib().cmt_gtdb_collide(ctypes.byref(a), _stream()), "cmt_gtdb_collide")
    return keep, cnt


# ---- host side ---------------------------------------------------------------------------------------------------
_CORNER_NORM = np.array([[0, 0, 0], [0, 0, 1], [0, 1, 1], [0, 1, 0], [1, 0, 0], [1, 0, 1], [1, 1, 1], [1, 1, 0]],
                        np.float64) - [0.5, 0.5, 0.0]


def box_corners(boxes):
    """``LiDARInstance3DBoxes.corners`` for [n, >= 7] boxes -> float64 [n, 8, 3]: the corner order of mmdet3d
    ((x0 y0 z0), (x0 y0 z1), (x0 y1 z1), (x0 y1 z0), then x1), origin (0.5, 0.5, 0), rotated counter-clockwise by
    yaw.  Stated deviation: the reference computes them in float32 torch; this is float64."""
    b = np.asarray(boxes, dtype=np.float64)
    if b.ndim != 2 or b.shape[1] < 7:
        raise ValueError(f"boxes must be [n, >= 7], got {b.shape}")
    loc = _CORNER_NORM[None] * b[:, None, 3:6]
    c, s = np.cos(b[:, 6])[:, None], np.sin(b[:, 6])[:, None]
    x = loc[..., 0] * c - loc[..., 1] * s + b[:, None, 0]
    y = loc[..., 0] * s + loc[..., 1] * c + b[:, None, 1]
    return np.stack([x, y, loc[..., 2] + b[:, None, 2]], -1)


def crop_plan(corners, lidar2img, frame_hw, keep_largest=True):
    """``find_img_crop`` of create_gt_database_cmt.py for one box, in float64 numpy: ``corners`` [8, 3],
    ``lidar2img`` a stack of 4 x 4 matrices (the cameras in the reference's order), ``frame_hw = (H, W)`` -> None or
    dict(cam, bbox=(x0, y0, x1, y1), depth): the crop is ``frame[cam, y0:y1, x0:x1]``, ``depth`` the mean of the
    eight corner depths.

    As the reference, per camera: x and y of every corner are divided by its depth; the camera is skipped when
    ``coord_img[2] <= 0`` holds anywhere, which reads ROW 2, that is corner 2's (u, v, depth, w), not the depth
    column: a box with another corner behind the camera passes, a box whose corner 2 projects to u <= 0 or v <= 0
    does not.  min / max of the projected corners are clipped to [0, W - 1] and [0, H - 1] and then truncated; the
    camera is skipped when a side is <= 10.
    Stated deviation (``keep_largest=True``): a camera replaces the choice only with a STRICTLY larger area, so the
    largest crop wins and the first camera wins ties.  The reference compares with ``crop_area``, which it never
    updates from 0: its LAST qualifying camera wins; ``keep_largest=False`` gives exactly that.
    Non-finite projections raise ValueError, as in ``paste_plan``."""
    c = np.asarray(corners, dtype=np.float64)
    L = np.asarray(lidar2img, dtype=np.float64)
    if c.shape != (8, 3):
        raise ValueError(f"corners must be [8, 3], got {c.shape}")
    if L.ndim != 3 or L.shape[1:] != (4, 4):
        raise ValueError(f"lidar2img must be [cams, 4, 4], got {L.shape}")
    H, W = (int(v) for v in frame_hw)
    if H <= 0 or W <= 0:
        raise ValueError(f"frame_hw must be positive, got {frame_hw}")
    c4 = np.concatenate([c, np.ones((8, 1))], -1)
    best, area = None, 0
    for cam, mat in enumerate(L):
        with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
            coord = c4 @ mat.T
            coord[:, :2] /= coord[:, 2, None]
        if not np.isfinite(coord).all():
            raise ValueError("non-finite projection of a box corner")
        if (coord[2] <= 0).any():
            continue
        depth = float(coord[:, 2].mean())
        bbox = np.concatenate([coord[:, :2].min(0), coord[:, :2].max(0)])
        bbox[0::2] = np.clip(bbox[0::2], 0, W - 1)
        bbox[1::2] = np.clip(bbox[1::2], 0, H - 1)
        bbox = bbox.astype(np.int64)
        if ((bbox[2:] - bbox[:2]) <= 10).any():
            continue
        a = int((bbox[3] - bbox[1]) * (bbox[2] - bbox[0]))
        if a > area:
            best = dict(cam=cam, bbox=tuple(int(v) for v in bbox), depth=depth)
            if keep_largest:
                area = a
    return best


class BatchSampler:
    """mmdet3d's ``BatchSampler`` over ``sampled_list`` with an explicit numpy RandomState: the indices are
    shuffled with ``rng.shuffle`` at construction and again at each wrap; a request that reaches the end
    (``idx + num >= len``) returns the tail, which may be shorter than asked, and resets."""

    def __init__(self, sampled_list, rng, name=None, shuffle=True):
        self._sampled_list = sampled_list
        self._indices = np.arange(len(sampled_list))
        self._rng, self._shuffle, self._name = rng, shuffle, name
        if shuffle:
            rng.shuffle(self._indices)
        self._idx = 0

    def sample_indices(self, num):
        if self._idx + num >= len(self._sampled_list):
            ret = self._indices[self._idx:].copy()
            if self._shuffle:
                self._rng.shuffle(self._indices)
            self._idx = 0
        else:
            ret = self._indices[self._idx:self._idx + num]
            self._idx += num
        return ret

    def sample(self, num):
        return [self._sampled_list[i] for i in self.sample_indices(num)]


class GtDatabase:
    """The ground-truth database in device memory: one fp32 [capacity_rows, num_features] buffer of segments and,
    on the host, the reference's ``db_infos`` (a dict class name -> list of records)."""

    def __init__(self, classes, num_features, device, capacity_rows):
        self.classes = list(classes)
        self.num_features = int(num_features)
        self.device = torch.device(device)
        self.capacity_rows = int(capacity_rows)
        if not 3 <= self.num_features <= 8:
            raise ValueError(f"num_features must be 3..8, got {num_features}")
        if not 0 < self.capacity_rows < 2 ** 31:
            raise ValueError(f"capacity_rows must be in (0, 2^31), got {capacity_rows}")
        if self.device.type != "cuda":
            raise ValueError("the database lives on a HIP device (no CPU path)")
        self.rows = torch.empty((self.capacity_rows, self.num_features), dtype=torch.float32, device=self.device)
        self.used_rows = 0
        self.db_infos = {}
        self._group_counter = 0
        self._frames = 0

    def __len__(self):
        return sum(len(v) for v in self.db_infos.values())

    def add_frame(self, points, boxes, names, *, count=None, frames=None, lidar2img=None, sample_idx=None,
                  difficulty=None, group_ids=None, used_classes=None):
        """What create_groundtruth_database does with one sample -> the list of records it added.

        ``points`` fp32 [N, F] on the device with the optional device ``count``; ``boxes`` [M, 7 | 9] (a host array
        or a tensor; the records keep host copies, so a device tensor costs a second read); ``names`` the M class
        names.  The segments of the boxes whose name is in ``used_classes`` (None: all) are appended to the
        buffer by one cmt_gtdb_extract call; then ``offsets`` is read back, ONE host read per frame: building the
        database is a build step, not the training loop.  RuntimeError, with nothing recorded, when the buffer
        cannot hold the frame.
        A record has the reference's fields ``name``, ``box3d_lidar`` (float32), ``num_points_in_gt``,
        ``difficulty`` (default 0), ``gt_idx``, ``image_idx`` (``sample_idx``, default the frame's ordinal),
        ``group_id`` (a counter over the distinct ``group_ids`` of recorded objects, default one group per box),
        ``image_crop_key`` and ``image_crop_depth``; in place of ``path`` it has ``segment = (first row, rows)``
        and in place of ``image_path`` ``patch``.  With ``frames`` (uint8 [V, H, W, 3] on the device) and
        ``lidar2img`` [V, 4, 4], ``crop_plan(box_corners(box), lidar2img, (H, W))`` chooses the crop: ``patch`` is a
        device clone of that slice and ``image_crop_key`` the camera's index; without a crop they are None and ''
        (and ``image_crop_depth`` 0, as in the reference)."""
        points = _rows(points, "points", (self.num_features,))
        host_boxes = np.ascontiguousarray((boxes.detach().cpu().numpy() if torch.is_tensor(boxes) else np.asarray(boxes)),
                                          dtype=np.float32)
        if host_boxes.ndim != 2 or host_boxes.shape[1] not in (7, 9):
            raise ValueError(f"boxes must be [M, 7 | 9], got {host_boxes.shape}")
        M = host_boxes.shape[0]
        names = list(names)
        if len(names) != M:
            raise ValueError(f"{M} boxes but {len(names)} names")
        difficulty = np.zeros(M, np.int32) if difficulty is None else np.asarray(difficulty)
        group_ids = np.arange(M, dtype=np.int64) if group_ids is None else np.asarray(group_ids)
        if difficulty.shape != (M,) or group_ids.shape != (M,):
            raise ValueError("difficulty and group_ids must have one entry per box")
        if (frames is None) != (lidar2img is None):
            raise ValueError("frames and lidar2img come together")
        if frames is not None:
            if not torch.is_tensor(frames) or frames.dtype != torch.uint8 or frames.dim() != 4 or frames.shape[3] != 3:
                raise ValueError("frames must be a uint8 [V, H, W, 3] tensor")
            lidar2img = np.asarray(lidar2img, dtype=np.float64)
            if lidar2img.shape != (frames.shape[0], 4, 4):
                raise ValueError(f"lidar2img must be [{frames.shape[0]}, 4, 4], got {lidar2img.shape}")
        sel = [i for i in range(M) if used_classes is None or names[i] in used_classes]
        if len(sel) > MAX_FRAME_BOXES:
            raise ValueError(f"at most {MAX_FRAME_BOXES} boxes a frame, got {len(sel)}")
        count = _count_word(count)
        _on_device(self.device, points=points, count=count, frames=frames)
        image_idx = self._frames if sample_idx is None else sample_idx
        self._frames += 1
        if not sel:
            return []
        dev_boxes = torch.from_numpy(host_boxes[sel]).to(self.device)
        _, offsets = extract_objects(points, dev_boxes, count=count, out=self.rows[self.used_rows:])
        off = offsets.cpu().numpy().astype(np.int64)          # the frame's one host read
        if self.used_rows + off[-1] > self.capacity_rows:
            raise RuntimeError(f"the database buffer holds {self.capacity_rows} rows, {self.used_rows} used; this "
                               f"frame needs {int(off[-1])}")
        added, group_dict = [], {}
        for k, i in enumerate(sel):
            info = dict(name=names[i], segment=(self.used_rows + int(off[k]), int(off[k + 1] - off[k])),
                        image_idx=image_idx, patch=None, image_crop_key="", image_crop_depth=0, gt_idx=i,
                        box3d_lidar=host_boxes[i].copy(), num_points_in_gt=int(off[k + 1] - off[k]),
                        difficulty=difficulty[i])
            if frames is not None:
                plan = crop_plan(box_corners(host_boxes[i:i + 1])[0], lidar2img, frames.shape[1:3])
                if plan is not None:
                    x0, y0, x1, y1 = plan["bbox"]
                    info.update(patch=frames[plan["cam"], y0:y1, x0:x1].clone(), image_crop_key=plan["cam"],
                                image_crop_depth=plan["depth"])
            gid = group_ids[i].item() if hasattr(group_ids[i], "item") else group_ids[i]
            if gid not in group_dict:
                group_dict[gid] = self._group_counter
                self._group_counter += 1
            info["group_id"] = group_dict[gid]
            self.db_infos.setdefault(names[i], []).append(info)
            added.append(info)
        self.used_rows += int(off[-1])
        return added


class UnifiedDataBaseSampler:
    """The reference's ``UnifiedDataBaseSampler`` over a ``GtDatabase``.  ``rate``, ``prepare`` (``filter_by_difficulty``
    / ``filter_by_min_points``, applied in the dict's order), ``sample_groups`` (class -> the most objects of it a
    scene should hold) and ``classes`` are the ``db_sampler`` entries of a config; ``rng`` a numpy RandomState that
    stands for the reference's global ``np.random``: one ``BatchSampler`` per class of the database, built (and
    shuffled) in the database's order."""

    def __init__(self, db, rate, prepare, sample_groups, classes, rng):
        if not isinstance(getattr(db, "db_infos", None), dict):
            raise ValueError(f"db must be a GtDatabase (or offer its db_infos, rows and device), got {type(db)}")
        if classes is None:
            raise ValueError("classes is required")
        self.db, self.rate, self.prepare, self.rng = db, rate, dict(prepare or {}), rng
        self.classes = list(classes)
        self.cat2label = {name: i for i, name in enumerate(self.classes)}
        infos = {k: list(v) for k, v in db.db_infos.items()}
        for func, val in self.prepare.items():
            if func not in ("filter_by_difficulty", "filter_by_min_points"):
                raise ValueError(f"prepare: unknown function {func!r}")
            infos = getattr(self, func)(infos, val)
        self.db_infos = infos
        self.sample_classes = list(sample_groups.keys())
        self.sample_max_nums = [int(v) for v in sample_groups.values()]
        for name in self.sample_classes:
            if name not in self.cat2label:
                raise ValueError(f"sample_groups names {name!r}, which is not in classes")
        self.sampler_dict = {k: BatchSampler(v, rng, k, shuffle=True) for k, v in infos.items()}

    @staticmethod
    def filter_by_difficulty(db_infos, removed_difficulty):
        return {k: [i for i in v if i["difficulty"] not in removed_difficulty] for k, v in db_infos.items()}

    @staticmethod
    def filter_by_min_points(db_infos, min_gt_points_dict):
        for name, min_num in min_gt_points_dict.items():
            min_num = int(min_num)
            if min_num > 0 and name in db_infos:     # the reference raises KeyError for a class the database lacks
                db_infos[name] = [i for i in db_infos[name] if i["num_points_in_gt"] >= min_num]
        return db_infos

    def sample_counts(self, gt_labels):
        """the objects to draw per entry of ``sample_groups``: ``int(max - present)``, then ``np.round(rate * .)``"""
        gt_labels = np.asarray(gt_labels).reshape(-1)
        out = []
        for name, max_num in zip(self.sample_classes, self.sample_max_nums):
            num = int(max_num - np.sum([n == self.cat2label[name] for n in gt_labels]))
            out.append(int(np.round(self.rate * num).astype(np.int64)))
        return out

    def sample_all(self, gt_bboxes, gt_labels, with_img=False):
        """The reference's ``sample_all`` -> None when nothing is kept, else dict(gt_bboxes_3d fp32 [K, D] and
        gt_labels_3d int64 [K] on the device (``augment_boxes``' ``paste_boxes`` / ``paste_labels``), points fp32
        [n, F] on the device (``augment_points``' ``paste_points``), points_idx int64 numpy [n] (the object of each
        row), images (``with_img``: per object its uint8 [h, w, 3] device patch, an empty tensor without one),
        group_ids numpy).  ``gt_bboxes`` is the scene's [n_gt, 7 | 9] ground truth (host array or tensor),
        ``gt_labels`` its labels.
        The candidates of every class are drawn first, in the reference's order (the collision test draws
        nothing); ONE cmt_gtdb_collide call tests them all and ``keep`` is read back, the sampler's only host read;
        ONE cmt_gtdb_gather call moves the kept objects' points."""
        gt = np.ascontiguousarray(gt_bboxes.detach().cpu().numpy() if torch.is_tensor(gt_bboxes) else np.asarray(gt_bboxes),
                                  dtype=np.float32)
        if gt.ndim != 2 or gt.shape[1] not in (7, 9):
            raise ValueError(f"gt_bboxes must be [n, 7 | 9], got {gt.shape}")
        labels = (gt_labels.detach().cpu().numpy() if torch.is_tensor(gt_labels) else np.asarray(gt_labels)).reshape(-1)
        if labels.shape[0] != gt.shape[0]:
            raise ValueError(f"{gt.shape[0]} boxes but {labels.shape[0]} labels")
        cand, group = [], []
        for g, (name, num) in enumerate(zip(self.sample_classes, self.sample_counts(labels))):
            if num > 0:
                drawn = self.sampler_dict[name].sample(num)
                cand += drawn
                group += [g] * len(drawn)
        if not cand:
            return None
        D = gt.shape[1]
        sp = np.stack([c["box3d_lidar"] for c in cand], 0)
        if sp.shape[1] != D:
            raise ValueError(f"the database holds {sp.shape[1]}-column boxes, gt_bboxes has {D}")
        n_gt = gt.shape[0]
        if n_gt + len(cand) > MAX_COLLIDE_BOXES:
            raise ValueError(f"at most {MAX_COLLIDE_BOXES} boxes in one collision test, got {n_gt + len(cand)}")
        dev = self.db.device
        boxes = torch.from_numpy(np.concatenate([gt, sp], 0)).to(dev)
        keep, _ = collide(boxes, n_gt, group)
        kept = np.nonzero(keep.cpu().numpy())[0]               # the only host read
        if kept.size == 0:
            return None
        if kept.size > MAX_PASTE_BOXES:
            raise ValueError(f"at most {MAX_PASTE_BOXES} objects can be pasted, {kept.size} were kept")
        sampled = [cand[i] for i in kept]
        lens = np.array([s["segment"][1] for s in sampled], np.int64)
        starts = np.concatenate([[0], np.cumsum(lens)])
        table = np.zeros((6, len(sampled)), np.int32)
        table[0] = [s["segment"][0] for s in sampled]
        table[1], table[2] = lens, starts[:-1]
        table[3:] = sp[kept, :3].T.copy().view(np.int32)        # the centres' bits ride along: one upload
        t = torch.from_numpy(table).to(dev)
        centre = t[3:].view(torch.float32).t().contiguous()
        points = gather_objects(self.db.rows, t[0], t[1], t[2], centre, int(starts[-1]))
        ret = dict(gt_labels_3d=torch.tensor([self.cat2label[s["name"]] for s in sampled], dtype=torch.int64, device=dev),
                   gt_bboxes_3d=boxes[n_gt + torch.from_numpy(kept).to(dev)],
                   points=points, points_idx=np.repeat(np.arange(len(sampled)), lens),
                   images=[], group_ids=np.arange(n_gt, n_gt + len(sampled)))
        if with_img:
            empty = torch.empty((0, 0, 3), dtype=torch.uint8, device=dev)
            ret["images"] = [s["patch"] if s.get("patch") is not None else empty for s in sampled]
        return ret


def db_sampler_from_config(cfg, db, rng=None):
    """The ``db_sampler`` of the [Unified]ObjectSample[Coop] step of a config's ``data.train`` pipeline (through
    CBGSDataset's ``dataset``) over ``db`` -> UnifiedDataBaseSampler.  ``rate``, ``prepare``, ``sample_groups`` and
    ``classes`` are used; ``info_path``, ``data_root`` and ``points_loader`` name files and are ignored, because the
    database is in memory.  ``rng``: a numpy RandomState (None: a fresh unseeded one).  ValueError for a
    pipeline without such a step."""
    train = cfg["data"]["train"]
    while isinstance(train, dict) and "pipeline" not in train and "dataset" in train:
        train = train["dataset"]
    for st in _pipeline_steps(train["pipeline"]):
        if st.get("type") in _SAMPLERS and isinstance(st.get("db_sampler"), dict):
            s = st["db_sampler"]
            return UnifiedDataBaseSampler(db, rate=s.get("rate", 1.0), prepare=s.get("prepare", {}),
                                          sample_groups=s["sample_groups"], classes=s.get("classes"),
                                          rng=rng if rng is not None else np.random.RandomState())
    raise ValueError("the training pipeline has no object sampler with a db_sampler")
