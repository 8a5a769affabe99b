"""Result pictures: the top view and camera overlays of a frame, drawn on the device (native_render.py,
cmt_render_* of include/cmt_hip.h), and PNG files written with zlib and struct only.

``Visualizer.bev`` draws the clouds of a frame (each in its own colour ramp by height), ground truth, predictions,
track trails and track ids into one top view; ``Visualizer.cameras`` projects them into camera frames through
``lidar2img``.  Every ingredient is one launch on buffers that already live on the device; no box or point is read
back, the finished picture is the only thing that leaves (``.cpu()`` by the caller or ``write_png``).  Pictures are
bitwise repeatable: the kernels only raise a key plane with atomic maxima.

``show_results`` is the body of the detectors' method of that name.  Stated deviation from the reference
(mmdet3d's ``show_result``): PNG pictures instead of ``.obj`` files, and ``show=True`` raises NotImplementedError
(there is no display).
"""
import os
import struct
import zlib

import numpy as np
import torch

from ... import native_render as NR

__all__ = ["Visualizer", "write_png", "read_png", "show_results"]


# ---- PNG: 8-bit RGB, filter 0, not interlaced --------------------------------------------------------------------

def _chunk(kind, data):
    return struct.pack(">I", len(data)) + kind + data + struct.pack(">I", zlib.crc32(kind + data) & 0xFFFFFFFF)


def write_png(path, image):
    """``image``: uint8 [H, W, 3], a tensor on either side or an array -> an 8-bit RGB PNG file"""
    if torch.is_tensor(image):
        image = image.detach().cpu().numpy()
    image = np.ascontiguousarray(image)
    if image.dtype != np.uint8 or image.ndim != 3 or image.shape[2] != 3 or image.shape[0] < 1 or image.shape[1] < 1:
        raise ValueError(f"write_png takes a uint8 [H, W, 3] picture, got {image.dtype} {image.shape}")
    H, W = image.shape[:2]
    raw = np.zeros((H, 1 + 3 * W), dtype=np.uint8)      # a filter byte 0 before every row
    raw[:, 1:] = image.reshape(H, 3 * W)
    data = (b"\x89PNG\r\n\x1a\n" + _chunk(b"IHDR", struct.pack(">IIBBBBB", W, H, 8, 2, 0, 0, 0))
            + _chunk(b"IDAT", zlib.compress(raw.tobytes(), 6)) + _chunk(b"IEND", b""))
    with open(path, "wb") as fh:
        fh.write(data)


def read_png(path):
    """The inverse of ``write_png`` -> uint8 [H, W, 3] array.  It reads what write_png writes (8-bit RGB, filter 0,
    not interlaced) and raises ValueError on anything else."""
    with open(path, "rb") as fh:
        data = fh.read()
    if data[:8] != b"\x89PNG\r\n\x1a\n":
        raise ValueError(f"{path}: not a PNG file")
    pos, idat, head = 8, [], None
    while pos + 8 <= len(data):
        n, kind = struct.unpack(">I", data[pos:pos + 4])[0], data[pos + 4:pos + 8]
        body = data[pos + 8:pos + 8 + n]
        if struct.unpack(">I", data[pos + 8 + n:pos + 12 + n])[0] != zlib.crc32(kind + body) & 0xFFFFFFFF:
            raise ValueError(f"{path}: bad checksum in chunk {kind!r}")
        if kind == b"IHDR":
            head = struct.unpack(">IIBBBBB", body)
        elif kind == b"IDAT":
            idat.append(body)
        elif kind == b"IEND":
            break
        pos += 12 + n
    if head is None or head[2:] != (8, 2, 0, 0, 0):
        raise ValueError(f"{path}: only 8-bit RGB, not interlaced, is read")
    W, H = head[:2]
    raw = np.frombuffer(zlib.decompress(b"".join(idat)), dtype=np.uint8)
    if raw.size != H * (1 + 3 * W):
        raise ValueError(f"{path}: the pixel data has the wrong size")
    raw = raw.reshape(H, 1 + 3 * W)
    if raw[:, 0].any():
        raise ValueError(f"{path}: only filter 0 is read")
    return raw[:, 1:].reshape(H, W, 3).copy()


# ---- the visualizer ----------------------------------------------------------------------------------------------

def _f32(t, device, cols=None):
    t = torch.as_tensor(t).to(device=device, dtype=torch.float32)
    if cols is not None and (t.dim() != 2 or t.shape[1] < cols):
        raise ValueError(f"expected a [n, >= {cols}] tensor, got {tuple(t.shape)}")
    return t if t.dim() != 2 or t.stride(1) == 1 or t.shape[0] == 0 else t.contiguous()


def _i32(t, device):
    return None if t is None else torch.as_tensor(t).to(device=device, dtype=torch.int32).contiguous()


class Visualizer:
    """Pictures of a frame on ``device``.  ``class_names``: the classes of the labels (the palette's length);
    ``point_cloud_range``: what the top view shows, at ``bev_size = (H, W)`` pixels.  ``z_origin`` / ``gt_z_origin``
    of the methods say what a box row's z is: 0 the bottom (a detector's ``boxes_3d``), 0.5 the gravity centre
    (``cmt_box_decode``'s rows, the tracker's, the evaluators' ground truth)."""

    def __init__(self, class_names, point_cloud_range, bev_size=(800, 800), device="cuda", thickness=1, digit_scale=1):
        self.class_names = list(class_names)
        self.pcr = [float(v) for v in point_cloud_range]
        if len(self.pcr) != 6:
            raise ValueError(f"point_cloud_range has 6 entries, got {len(self.pcr)}")
        self.H, self.W = int(bev_size[0]), int(bev_size[1])
        self.view = NR.bev_view(self.pcr, self.H, self.W)[None]
        NR._size(1, self.H, self.W)
        self.device = torch.device(device)
        self.thickness, self.digit_scale = int(thickness), int(digit_scale)
        self._const = None

    def _tables(self):
        """the colour tables on the device, uploaded once"""
        if self._const is None:
            dev = self.device
            self._const = dict(height=[torch.from_numpy(NR.height_lut(k)).to(dev) for k in (0, 1)],
                               depth=torch.from_numpy(NR.depth_lut()).to(dev),
                               palette=torch.from_numpy(NR.class_palette(max(len(self.class_names), 1))).to(dev))
        return self._const

    # the overlays every picture shares
    def _overlays(self, plane, views, near, boxes, scores, labels, count, gt_boxes, gt_labels, track_ids, trails,
                  score_thr, z_origin, gt_z_origin):
        dev, tab = self.device, self._tables()
        if gt_boxes is not None:
            NR.render_boxes(plane, views, _f32(gt_boxes, dev, 7), z_origin=gt_z_origin, labels=_i32(gt_labels, dev),
                            rgb_default=NR.GT_RGB, layer=NR.LAYER_GT, near=near, thickness=self.thickness)
        if trails:
            pts = [np.asarray(h, dtype=np.float32).reshape(-1, 3) for h in trails]
            p0 = np.concatenate([h[:-1] for h in pts] + [np.zeros((0, 3), np.float32)])
            p1 = np.concatenate([h[1:] for h in pts] + [np.zeros((0, 3), np.float32)])
            if len(p0):
                rgb = torch.full((len(p0),), NR.TRAIL_RGB, dtype=torch.int32, device=dev)
                NR.render_segments(plane, views, torch.from_numpy(p0).to(dev), torch.from_numpy(p1).to(dev), rgb,
                                   layer=NR.LAYER_TRAILS, near=near)
        if boxes is None:
            return
        boxes = _f32(boxes, dev, 7)
        scores = None if scores is None else _f32(scores, dev)
        thr = float("-inf") if score_thr is None else float(score_thr)
        NR.render_boxes(plane, views, boxes, z_origin=z_origin, count=count, labels=_i32(labels, dev), scores=scores,
                        score_thr=thr, class_rgb=tab["palette"], layer=NR.LAYER_PRED, near=near,
                        thickness=self.thickness)
        if track_ids is not None:
            ids = _i32(track_ids, dev)
            M = int(boxes.shape[0])
            if ids.shape != (M,):
                raise ValueError(f"track_ids must have one id per box row ({M}), got {tuple(ids.shape)}")
            # rows that draw no box draw no number: masked on the device, nothing is read back.  A row is invalid as
            # cmt_render_boxes has it: one of its seven values not finite, or a size <= 0
            hide = ~(torch.isfinite(boxes[:, :7]).all(1) & (boxes[:, 3:6] > 0).all(1))
            if count is not None:
                hide |= torch.arange(M, device=dev) >= count.reshape(1)
            if scores is not None:
                hide |= ~(scores > thr)
            ids = torch.where(hide, torch.full_like(ids, -1), ids)
            anchors = boxes[:, :3].clone()
            if z_origin == 0.0:      # the number stands at the top face, like the heading mark
                anchors[:, 2] += boxes[:, 5]
            else:
                anchors[:, 2] += boxes[:, 5] * 0.5
            NR.render_digits(plane, views, ids, anchors, scale=self.digit_scale, layer=NR.LAYER_DIGITS, near=near)

    def bev(self, points_list, boxes=None, scores=None, labels=None, count=None, gt_boxes=None, gt_labels=None,
            track_ids=None, trails=None, score_thr=None, z_origin=0.0, gt_z_origin=0.5, radius=0):
        """The top view -> uint8 [H, W, 3] on the device.  ``points_list``: one cloud or several (fp32 [n, >= 3],
        the NaN-padded buffers of ``prepare_points`` as they are), cloud k in colour ramp k % 2 by height, the highest
        point of a pixel on top.  ``boxes`` [M, >= 7] with optional ``scores``, ``labels``, a device ``count`` and
        ``score_thr``; ``gt_boxes`` in one colour below them; ``track_ids`` int [M] (-1: no number) drawn at the
        boxes; ``trails``: ``Tracker.tracks()['history']``, a list of [m, 3] position arrays."""
        dev, tab = self.device, self._tables()
        if torch.is_tensor(points_list):
            points_list = [points_list]
        plane = NR.new_plane(1, self.H, self.W, dev)
        z0, z1 = self.pcr[2], self.pcr[5]
        for k, pts in enumerate(points_list or []):
            NR.render_points(plane, self.view, _f32(pts, dev, 3), tab["height"][k % 2], layer=NR.LAYER_POINTS, near=0.5,
                             radius=radius, color_col=2, lo=z0, span=z1 - z0)
        self._overlays(plane, self.view, 0.5, boxes, scores, labels, count, gt_boxes, gt_labels, track_ids, trails,
                       score_thr, z_origin, gt_z_origin)
        return NR.render_resolve(plane)[0]

    def cameras(self, frames, lidar2img, points=None, boxes=None, scores=None, labels=None, count=None, gt_boxes=None,
                gt_labels=None, track_ids=None, trails=None, score_thr=None, z_origin=0.0, gt_z_origin=0.5, radius=1,
                max_depth=60.0, inplace=False):
        """Camera overlays -> uint8 [V, H, W, 3] on the device.  ``frames``: uint8 [V, H, W, 3] as loaded (interleaved),
        V <= 8; ``lidar2img``: V host 4 x 4 matrices into those frames.  ``points``: one cloud or a list, coloured by
        depth up to ``max_depth``, the nearest point of a pixel on top.  The caller's frames are left alone unless
        ``inplace``; then the overlays are written into them and they are returned, which needs contiguous frames on
        the visualizer's device (ValueError otherwise)."""
        dev, tab = self.device, self._tables()
        if not torch.is_tensor(frames) or frames.dtype != torch.uint8 or frames.dim() != 4 or frames.shape[3] != 3:
            raise ValueError("frames must be a uint8 [V, H, W, 3] tensor")
        if inplace and (frames.device != dev or not frames.is_contiguous()):
            raise ValueError(f"inplace=True writes into the caller's frames: they must be contiguous and on {dev}, got "
                             f"{frames.device}, contiguous {frames.is_contiguous()}")
        src = frames.to(dev).contiguous()
        V, H, W = (int(s) for s in src.shape[:3])
        if len(lidar2img) != V:
            raise ValueError(f"lidar2img must hold {V} 4 x 4 matrices, one per frame, got {len(lidar2img)}")
        views = np.stack([NR.camera_view(m) for m in lidar2img])
        plane = NR.new_plane(V, H, W, dev)
        if points is not None:
            for pts in ([points] if torch.is_tensor(points) else points):
                NR.render_points(plane, views, _f32(pts, dev, 3), tab["depth"], layer=NR.LAYER_POINTS, near=0.1,
                                 radius=radius, near_wins=True, color_col=-1, lo=0.0, span=max_depth)
        self._overlays(plane, views, 0.1, boxes, scores, labels, count, gt_boxes, gt_labels, track_ids, trails,
                       score_thr, z_origin, gt_z_origin)
        return NR.render_resolve(plane, src=src, out=src if inplace else None)


# ---- show_results of the detectors -------------------------------------------------------------------------------

def _sample_clouds(data, b):
    clouds = []
    for key in ("points", "vehicle_points", "infrastructure_points"):
        entry = data.get(key)
        if entry is None:
            continue
        batch = entry[0]
        if not isinstance(batch, (list, tuple)) or not all(torch.is_tensor(t) for t in batch):
            raise ValueError(f"Unsupported data type {type(batch)} for visualization: data[{key!r}][0] is a list of tensors")
        clouds.append(batch[b])
    return clouds


def show_results(model, data, result, out_dir, show=False, score_thr=None, gt_bboxes=None):
    """The detectors' ``show_results``: for every sample b of ``result`` the top view ``<out_dir>/<name>_bev.png`` of
    ``data['points'][0][b]`` (for the cooperative detector also ``vehicle_points`` / ``infrastructure_points``) with
    ``result[b]['pts_bbox']`` and, when ``data['img'][0][b]`` holds uint8 [V, H, W, 3] frames and the sample's
    ``img_metas`` a ``lidar2img`` into them, ``<name>_cam<v>.png``.  ``name`` is the stem of the metas' ``pts_filename``,
    else the sample index in six digits.  ``gt_bboxes``: [g, >= 7] bottom-centre rows (one tensor, or one per sample).
    -> the list of the files written."""
    if show:
        raise NotImplementedError("show_results(show=True): there is no display; the pictures are written to out_dir")
    if out_dir is None:
        raise ValueError("Expect out_dir, got none.")
    head = model.pts_bbox_head
    names = [n for task in head.class_names for n in task]
    dev = next(head.parameters()).device
    vis = Visualizer(names, head.pc_range, device=dev)
    os.makedirs(out_dir, exist_ok=True)
    metas = (data.get("img_metas") or [None])[0]
    written = []
    for b in range(len(result)):
        res = result[b]["pts_bbox"]
        meta = metas[b] if isinstance(metas, (list, tuple)) and b < len(metas) and isinstance(metas[b], dict) else {}
        name = os.path.splitext(os.path.basename(meta["pts_filename"]))[0] if meta.get("pts_filename") else f"{b:06d}"
        gt = gt_bboxes[b] if isinstance(gt_bboxes, (list, tuple)) else gt_bboxes
        kw = dict(boxes=res["boxes_3d"], scores=res["scores_3d"], labels=res["labels_3d"], score_thr=score_thr,
                  gt_boxes=gt, z_origin=0.0, gt_z_origin=0.0)
        clouds = _sample_clouds(data, b)
        path = os.path.join(out_dir, f"{name}_bev.png")
        write_png(path, vis.bev(clouds, **kw))
        written.append(path)
        img = data.get("img")
        frames = img[0][b] if img is not None and img[0] is not None else None
        if torch.is_tensor(frames) and frames.dtype == torch.uint8 and frames.dim() == 4 and meta.get("lidar2img") is not None:
            pics = vis.cameras(frames, meta["lidar2img"], points=clouds, **kw).cpu()
            for v in range(pics.shape[0]):
                path = os.path.join(out_dir, f"{name}_cam{v}.png")
                write_png(path, pics[v])
                written.append(path)
    return written
