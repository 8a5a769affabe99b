"""``tools/test.py``-shaped inference CLI for the head.

Mirrors the reference's ``tools/test.py`` (parse_args 36-127, main 130-285):
``test.py CONFIG [CHECKPOINT] [--out FILE] [--eval bbox] [--format-only]
[--cfg-options k=v ...] [--seed S] [--launcher none|pytorch] [--gpu-id G]``,
the same "at least one of --out / --eval / --format-only" check and the same
``--eval`` / ``--format-only`` exclusion.  Differences, all forced by scope:

* datasets are out of scope, so frames come from
  ``--synthetic`` (required): points uniform in the config's point-cloud
  range (seed + frame), voxelized + scatter-meaned by the native voxelizer
  (row a17), and the SECONDFPN / image-FPN outputs the backbones would give
  as relu(N(0,1)) / N(0,1) features of the BASELINE shapes (``synthetic.py``);
* ``--out`` writes JSON (boxes_3d [n, 9] bottom-centre, scores_3d,
  labels_3d per frame), not a pickle;
* ``--format-only --openlabel-dir DIR`` writes one OpenLABEL file per frame
  (``core/openlabel.py``, the reference's inference_to_openlabel_coop.py);
* ``--eval bbox`` has no annotations offline: it prints detection / voxel
  statistics instead of nuScenes AP;
* ``--eval nds`` (alone or with ``bbox``) scores the boxes against synthetic
  ground truth (``synthetic_gt`` seeded by seed and frame, 20 boxes per frame)
  with ``DetectionEvaluator``: every frame's device boxes go into the
  evaluator's device buffers and the reference's metrics summary (label_aps,
  mean_ap, tp_errors, nd_score, ...) is printed as one more JSON line after
  the statistics line.  With random weights the score says nothing about a
  model; the path is the one a dataset's ground truth would take;
* ``--eval iou`` (alone or with ``bbox`` / ``nds``) scores the same boxes
  against the same ground truth by overlap with ``IouDetectionEvaluator``
  (``--iou-mode bev|3d``, ``--iou-thr F [F ...]``; the package's own settings,
  not a devkit's) and prints one more JSON line ``metric="iou_ap"``: ap_all,
  ap_r40 and ap_101 per class and threshold, map_all, map_r40, the TP errors
  and the mean matched IoU;
* ``--launcher pytorch``: frames are sharded over ranks (frame i on rank
  i % world) and rank 0 gathers the results (all_gather_object), as
  multi_gpu_test's result collection.

``--detector`` runs the whole model instead of the head alone: synthetic points and synthetic uint8 camera
frames (``--frame-size H W``, 900 x 1600 by default) go through ``build_detector(make_detector_cfg(...))``:
``prepare_images`` with the crop of ``test_crop`` (the config's final_dim scaled to the frame width),
``lidar2img`` from ``crop_lidar2img``, ``pad_shape`` in the metas, and a CHECKPOINT is read by
``load_detector_checkpoint`` (every branch, not only ``pts_bbox_head.*``).  With ``--ida-size H W`` (the H and W
of the config's ``ida_aug_conf``; no default) frames of any ``--frame-size`` take the reference's whole test
branch instead: ``resize_crop_plan((H, W), final_dim)``, ``prepare_images(resize_dims=...)`` (bilinear resize
fused into the preparation kernel) and ``resize_crop_lidar2img``; TUMTraf is ``--frame-size 1200 1920 --ida-size
900 1600``.

With ``--sweeps K`` every cloud is a key frame plus K synthetic sweeps (seeded rigid sensor2lidar transforms and
time lags, a seeded ``vehicle2infrastructure`` for the coop configs) and goes through ``native_pts.prepare_points``
with the plan ``points_plan_from_config`` reads from the config: remove_close, sweep transform, time column,
``use_dim``, the vehicle cloud moved into the infrastructure frame, the range filter.  The detector gets the padded
buffer (kept rows, then NaN) as it is; the vehicle cameras' ``lidar2img`` follow through ``lidar2img_to_infra``.

``--eval nds --count-gt-points`` (opt-in) counts the frame's points inside every ground-truth box on the device
(``native_aug.points_in_boxes`` over the frame's cloud or clouds, padded buffers included) and passes the counts to
the evaluator as ``gt_num_pts``: ground truth without a point is dropped, as the reference's dataset does.  The nds
line then also carries ``gt_without_points``.  Not with ``--launcher pytorch`` (rank 0 holds no clouds).

``--nms rotate [--nms-thr X]`` (opt-in; the reference configs all say ``nms_type=None``) runs class-aware rotated
NMS on every frame's boxes on the device (``native_iou.nms_rotated``, BEV IoU) before anything else sees them: the
kept boxes, best first, are what ``--out``, ``--eval``, ``--track`` and ``--format-only`` get, and the JSON frames
gain ``nms_kept``.  Without it nothing changes.

``--track`` (with or without ``--detector``) runs every frame's boxes, in frame order, through one
``native_track.Tracker`` over the config's class names with its default settings, the frames 0.1 s apart: the JSON
frames gain ``track_ids`` (one id per box, -1 for a box that belongs to no track), and ``--format-only`` keys an
object by its track's uuid from frame to frame and writes the track's positions as ``track_history``.  The synthetic
frames are independent draws, so the ids say nothing about a scene; the path is the one a sequence would take.  Not
with ``--launcher pytorch`` (the frames are sharded over ranks).

``--eval track`` (alone or beside ``bbox`` / ``nds`` / ``iou``; it needs ``--track`` and exits with status 2 and a
message otherwise) scores the tracker's ids on the device (``core/evaluation.TrackingEvaluator``, cmt_mot_eval_*).
Under this flag only, the ground truth of frame f is frame 0's ``synthetic_gt`` moved by its own velocity columns
over f * 0.1 s, with instance ids equal to the row index.  It prints one JSON line ``metric="mot"`` with ``amota``,
``amotp`` and, per class at the recall level of highest MOTA, ``mota`` / ``motp`` / ``recall`` / ``ids`` / ``frag`` /
``fp`` / ``fn`` (null for a class without ground truth).  The detections are still independent draws, so the numbers
say nothing about tracking quality; the path is the one a sequence would take.

``--show-dir DIR [--show-score-thr S]`` (the reference's ``--show-dir``; it counts as an operation beside ``--out`` /
``--eval`` / ``--format-only``) writes one top view per frame, ``DIR/{frame:06d}_bev.png``: every agent's cloud in its
own colour ramp, the frame's boxes (after ``--nms``) in the class colours, the ground truth when an ``--eval`` built it,
track ids and trails with ``--track``.  With ``--detector`` on a config with cameras it also writes
``DIR/{frame:06d}_cam{v}.png``, the loaded frames with the same overlays through the uncropped ``lidar2img``.  The
pictures are drawn on the device (``core/visualizer``, cmt_render_*); the run prints ``wrote N pictures to DIR``.
Stated deviation: PNG pictures, not mmdet3d's ``.obj`` files, and ``--show`` alone (a window) exits with status 2.

Config 1 of BASELINE.json: ``python cmt-cooperative-perception_amd/tools/test.py
cmt_lidar_nus --synthetic --num-query 32 --num-layers 1 --points 1000 --eval bbox``.
The head runs on a HIP device only -- there is no CPU path; without a GPU the
CLI exits with status 2 and says so.
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

CONFIG_NAMES = ("cmt_lidar_nus", "cmt_fusion_nus", "cmtcoop_fusion_tumtraf", "cmtcoop_lidar_tumtraf")


def parse_args(argv=None):
    p = argparse.ArgumentParser(description="Test (inference) the CMT / CMTCoop head on synthetic frames")
    p.add_argument("config", help="config name or path (projects/configs/<name>.py)")
    p.add_argument("checkpoint", nargs="?", default=None,
                   help="mmcv detector checkpoint (pts_bbox_head.* keys) or a head state dict; "
                        "random init (the reference's init) when omitted")
    p.add_argument("--out", help="output result file (JSON)")
    p.add_argument("--format-only", action="store_true", help="format the results (OpenLABEL) without evaluation")
    p.add_argument("--openlabel-dir", default="openlabel_out", help="OpenLABEL output folder for --format-only")
    p.add_argument("--eval", type=str, nargs="+",
                   help="evaluation metrics (bbox: detection statistics; nds: nuScenes-style AP / TP errors / NDS "
                        "against synthetic ground truth, on the device; iou: IoU-matched AP against the same ground "
                        "truth; track: MOTA / MOTP / id switches and AMOTA / AMOTP of --track's ids against frame 0's "
                        "ground truth moved by its own velocity)")
    p.add_argument("--iou-mode", choices=["bev", "3d"], default="3d", help="overlap of --eval iou (default 3d)")
    p.add_argument("--iou-thr", type=float, nargs="+", default=None, metavar="F",
                   help="IoU thresholds of --eval iou (default: the package's 0.1 0.25 0.5 0.7); the TP errors are "
                        "taken at 0.5 when it is among them, else at the first")
    p.add_argument("--synthetic", action="store_true", help="synthetic frames of the config's shapes (required)")
    p.add_argument("--frames", type=int, default=1, help="synthetic frames")
    p.add_argument("--num-query", type=int, default=None, help="override num_query (config 1: 32)")
    p.add_argument("--num-layers", type=int, default=None, help="override the decoder depth (config 1: 1)")
    p.add_argument("--grid", type=int, nargs=2, default=None, metavar=("H", "W"),
                   help="BEV feature map size (default 180 180)")
    p.add_argument("--detector", action="store_true",
                   help="run CmtDetector / CmtCoopDetector on raw points and uint8 camera frames, not the head on "
                        "synthetic feature maps")
    p.add_argument("--frame-size", type=int, nargs=2, default=(900, 1600), metavar=("H", "W"),
                   help="camera frame size as loaded, for --detector (default 900 1600)")
    p.add_argument("--ida-size", type=int, nargs=2, default=None, metavar=("H", "W"),
                   help="H and W of the config's ida_aug_conf, for --detector: frames are resized to "
                        "resize_crop_plan((H, W), final_dim) and cropped, whatever --frame-size is (no default: "
                        "without it a frame must already have the size the crop is taken from)")
    p.add_argument("--points", type=int, default=1000, help="synthetic points per frame and agent (per sweep with "
                                                            "--sweeps)")
    p.add_argument("--sweeps", type=int, default=None, metavar="K",
                   help="for --detector: K synthetic sweeps per cloud, prepared on the device by prepare_points with "
                        "the config's point plan (default: key-frame points as they are)")
    p.add_argument("--count-gt-points", action="store_true",
                   help="with --eval nds: count the points inside every ground-truth box on the device and drop "
                        "ground truth without points (gt_num_pts)")
    p.add_argument("--precision", default="bf16", choices=["bf16", "fp16", "ref"], help="compute policy")
    p.add_argument("--img-precision", default=None, choices=["ref", "fp16"],
                   help="arithmetic of the image backbone (--detector): three-pass split-f16 or one-pass fp16; "
                        "default: the process setting (CMT_IMG_PRECISION, else ref)")
    p.add_argument("--bbox-classes", nargs="+", type=int, default=None, help="keep these labels (OpenLABEL)")
    p.add_argument("--bbox-score", type=float, default=None, help="minimum score (OpenLABEL)")
    p.add_argument("--track", action="store_true",
                   help="run every frame's boxes through one native_track.Tracker (frames 0.1 s apart): the JSON frames "
                        "gain track_ids, --format-only writes stable object keys and track_history")
    p.add_argument("--nms", choices=["rotate"], default=None,
                   help="class-aware rotated NMS (BEV IoU, on the device) of every frame's boxes before they are "
                        "written, evaluated, tracked or formatted; the JSON frames gain nms_kept (default: off)")
    p.add_argument("--nms-thr", type=float, default=None,
                   help="IoU threshold of --nms (default: the config's test_cfg nms_thr, else 0.2)")
    p.add_argument("--show", action="store_true", help="not built (there is no display): use --show-dir")
    p.add_argument("--show-dir", default=None, metavar="DIR",
                   help="write every frame's top view (and with --detector the camera overlays) as PNG files into DIR")
    p.add_argument("--show-score-thr", type=float, default=None, metavar="S",
                   help="draw only boxes that score above S (default: every box)")
    p.add_argument("--seed", type=int, default=0, help="random seed")
    p.add_argument("--cfg-options", nargs="+", default=None, metavar="KEY=VALUE",
                   help="override head config entries (dotted keys into pts_bbox_head, Python literals)")
    p.add_argument("--launcher", choices=["none", "pytorch"], default="none", help="job launcher")
    p.add_argument("--gpu-id", type=int, default=0, help="id of gpu to use (non-distributed)")
    p.add_argument("--local_rank", type=int, default=0)
    a = p.parse_args(argv)
    if a.show:
        p.error("--show opens a window and there is no display: write the pictures with --show-dir DIR")
    if not (a.out or a.eval or a.format_only or a.show_dir):
        p.error('Please specify at least one operation (save/eval/format the results) with the argument '
                '"--out", "--eval" or "--format-only"')
    if a.eval and a.format_only:
        p.error("--eval and --format-only cannot be both specified")
    if a.out is not None and not a.out.endswith(".json"):
        p.error("The output file must be a .json file.")
    if a.sweeps is not None and (not a.detector or a.sweeps < 0):
        p.error("--sweeps K needs --detector and K >= 0")
    if a.count_gt_points and (not a.eval or "nds" not in a.eval or a.launcher != "none"):
        p.error("--count-gt-points needs --eval nds and --launcher none")
    if a.eval and "track" in a.eval and not a.track:
        p.error("--eval track scores the tracker's ids: it needs --track")
    if not a.synthetic:
        p.error("dataset loading is out of scope (SURVEY.md 2 rows 18/21): run with --synthetic")
    return a


def config_name(path):
    name = os.path.splitext(os.path.basename(path))[0]
    if name not in CONFIG_NAMES:
        raise SystemExit(f"test.py: unknown config {path!r} (one of {', '.join(CONFIG_NAMES)})")
    return name


def apply_cfg_options(cfg, options):
    """``--cfg-options a.b=v``: v parsed as a Python literal (ast.literal_eval),
    else kept as a string; keys are dotted paths into the head config."""
    import ast
    for item in options or []:
        key, _, val = item.partition("=")
        try:
            val = ast.literal_eval(val)
        except (ValueError, SyntaxError):
            pass
        d = cfg
        parts = key.split(".")
        for k in parts[:-1]:
            d = d.setdefault(k, {})
        d[parts[-1]] = val
    return cfg


def build_head(args, name, device):
    from projects.mmdet3d_plugin import synthetic as S
    from projects.mmdet3d_plugin.registry import build_head as _build
    from projects.mmdet3d_plugin.checkpoint import load_head_checkpoint
    import torch
    nq = args.num_query if args.num_query is not None else 900
    # the BEV feature map is grid / out_size_factor (8): --grid H W sets grid_size = (8W, 8H, 40)
    grid = [8 * args.grid[1], 8 * args.grid[0], 40] if args.grid else None
    cfg, meta = S.make_head_cfg(name, num_query=nq, num_layers=args.num_layers, grid_size=grid)
    apply_cfg_options(cfg, args.cfg_options)
    torch.manual_seed(args.seed)
    head = _build(cfg)
    head.init_weights()
    if args.checkpoint:
        load_head_checkpoint(head, args.checkpoint)
    head.eval().to(device)
    return head, cfg, meta


def frame_inputs(name, meta, frame, args, device):
    """(forward closure inputs, list of per-agent point clouds) for one synthetic frame."""
    from projects.mmdet3d_plugin import synthetic as S
    seed = args.seed + 1000 * frame
    H, W = args.grid if args.grid else (180, 180)
    coop = name.startswith("cmtcoop")
    fusion = "fusion" in name
    if coop:
        agents = [("vehicle_", S.VEHICLE_YAWS if fusion else None), ("infrastructure_", S.INFRA_YAWS if fusion else None)]
    else:
        agents = [("", S.NUS_YAWS if fusion else None)]
    metas = [dict()]
    feats, points = [], []
    for i, (prefix, yaws) in enumerate(agents):
        pts = S.synthetic_points(args.points, meta["point_cloud_range"], seed=seed + 10 * i, device=device)
        points.append(pts)
        x = S.synthetic_bev(1, H, W, seed=seed + 1 + 10 * i, device=device)
        xi = None
        if yaws is not None:
            xi = S.synthetic_img(len(yaws), 40, 100, seed=seed + 2 + 10 * i, device=device)
            metas[0].update(S.synthetic_metas(1, yaws=yaws, prefix=prefix, seed=seed + 3 + 10 * i)[0])
        feats.append((x, xi))
    return feats, metas, points


def build_detector_model(args, name, device):
    from projects.mmdet3d_plugin import synthetic as S
    from projects.mmdet3d_plugin.registry import build_detector
    from projects.mmdet3d_plugin.checkpoint import load_detector_checkpoint
    import torch
    nq = args.num_query if args.num_query is not None else 900
    grid = [8 * args.grid[1], 8 * args.grid[0], 40] if args.grid else None
    cfg = S.make_detector_cfg(name, num_query=nq, num_layers=args.num_layers, grid_size=grid)
    apply_cfg_options(cfg["pts_bbox_head"], args.cfg_options)
    torch.manual_seed(args.seed)
    model = build_detector(cfg)
    model.init_weights()
    if args.checkpoint:
        load_detector_checkpoint(model, args.checkpoint)
    model.eval().to(device)
    return model, cfg


def detector_frame_inputs(name, cfg, meta, frame, args, device, show=None):
    """One synthetic frame for the detector -> (forward_test keyword arguments, per-agent point clouds).  ``show``: a
    list that receives, per agent with cameras, (the uint8 frames as loaded, their lidar2img without resize or crop)."""
    import numpy as np
    from projects.mmdet3d_plugin import native_img as NI
    from projects.mmdet3d_plugin import native_pts as NP
    from projects.mmdet3d_plugin import synthetic as S
    from projects.mmdet3d_plugin.config import load_config
    seed = args.seed + 1000 * frame
    coop = name.startswith("cmtcoop")
    fusion = "fusion" in name
    plan = v2i = None
    if args.sweeps is not None:
        plan = NP.points_plan_from_config(load_config(os.path.join(S.CONFIG_DIR, name + ".py")))
        if plan["coop"]:
            v2i = S.synthetic_vehicle2infrastructure(seed)
    body = cfg["vehicle_model"] if coop else cfg
    pcr = body["pts_voxel_layer"]["point_cloud_range"]
    Hf, Wf = args.frame_size
    fH, fW = meta.get("final_dim", (640, 1600))
    if args.ida_size is not None:
        Wi = args.ida_size[1]
        final_dim = (int(round(fH * Wi / fW)), Wi)   # the config's final_dim at the ida width
        resize, resize_dims, crop = NI.resize_crop_plan(args.ida_size, final_dim)
    else:
        final_dim = (int(round(fH * Wf / fW)), Wf)   # the config's final_dim at this frame width
    if coop:
        agents = [("vehicle_", S.VEHICLE_YAWS), ("infrastructure_", S.INFRA_YAWS)]
    else:
        agents = [("", S.NUS_YAWS)]
    metas, kw, points = dict(), dict(), []
    for i, (prefix, yaws) in enumerate(agents):
        to_infra = v2i if prefix == "vehicle_" else None
        if plan is None:
            pts = S.synthetic_points(args.points, pcr, seed=seed + 10 * i, device=device)
        else:
            # raw sweep buffers -> the detector's points on the device; the padded buffer goes in as it is
            key, sweeps, key_ts = S.synthetic_sweeps(args.sweeps, args.points, pcr, seed=seed + 10 * i, device=device,
                                                     margin=2.0)
            segs = NP.sweep_segments(key, sweeps, key_ts, time_dim=plan["time_dim"], remove_close=plan["remove_close"],
                                     sweeps_num=plan["sweeps_num"], coop=plan["coop"])
            pts, _ = NP.prepare_points(segs, use_dim=plan["use_dim"], load_dim=plan["load_dim"], agent_transform=to_infra,
                                       point_cloud_range=pcr if plan["point_cloud_range"] is not None else None)
        points.append(pts)
        kw[prefix + "points"] = [[pts]]
        if not fusion:
            continue
        frames = S.synthetic_frames(len(yaws), Hf, Wf, seed=seed + 2 + 10 * i, device=device)
        K = np.array([[1266.0 * Wf / 1600.0, 0.0, Wf / 2.0], [0.0, 1266.0 * Wf / 1600.0, Hf / 2.0], [0.0, 0.0, 1.0]])
        if args.ida_size is not None:
            img = NI.prepare_images(frames, crop=crop, resize_dims=resize_dims)
            metas[prefix + "lidar2img"] = [NI.resize_crop_lidar2img(K, S.camera_lidar2img(y, f=1.0, cx=0.0, cy=0.0),
                                                                    resize, crop) for y in yaws]
        else:
            _, crop = NI.test_crop((Hf, Wf), final_dim)
            img = NI.prepare_images(frames, crop=crop)
            metas[prefix + "lidar2img"] = [NI.crop_lidar2img(K, S.camera_lidar2img(y, f=1.0, cx=0.0, cy=0.0), crop)
                                           for y in yaws]
        if show is not None:
            full = [NI.crop_lidar2img(K, S.camera_lidar2img(y, f=1.0, cx=0.0, cy=0.0), (0, 0)) for y in yaws]
            show.append((frames, list(NP.lidar2img_to_infra(np.stack(full), to_infra)) if to_infra is not None else full))
        if to_infra is not None:
            metas[prefix + "lidar2img"] = list(NP.lidar2img_to_infra(np.stack(metas[prefix + "lidar2img"]), to_infra))
        metas[prefix + "pad_shape"] = [tuple(img.shape[2:]) + (3,)] * len(yaws)
        kw[prefix + "img"] = [img[None]]
    kw["img_metas"] = [[metas]]
    return kw, points


GT_PER_FRAME = 20


def eval_pc_range(name):
    from projects.mmdet3d_plugin import synthetic as S
    return S.make_head_cfg(name)[1]["point_cloud_range"]


def frame_ground_truth(frame, seed, pc_range, num_classes):
    """the synthetic ground truth of one frame -> (boxes [20, 9] fp32, labels [20] int64), on the host"""
    from projects.mmdet3d_plugin import synthetic as S
    boxes, labels = S.synthetic_gt(1, pc_range, num_classes, n=GT_PER_FRAME, seed=seed + 1000 * frame)
    return boxes[0].float(), labels[0]


def gt_point_counts(gt_boxes, points):
    """gt_num_pts of one frame: the points of every cloud in ``points`` (fp32 [n, F] on the device, NaN padding
    allowed) inside each gravity-centre ground-truth box [g, 9] -> int32 [g] on the device, no host read"""
    from projects.mmdet3d_plugin import native_aug as NA
    lidar = gt_boxes[:, :7].clone()
    lidar[:, 2] -= lidar[:, 5] * 0.5   # gravity centre -> bottom centre
    total = None
    for pts in points:
        c = NA.points_in_boxes(pts.float().contiguous(), lidar, want="count_per_box")
        total = c if total is None else total + c
    return total


TRACK_FRAME_SECONDS = 0.1   # --track: the synthetic frames are this far apart


def track_ground_truth(frame, seed, pc_range, num_classes):
    """--eval track: frame 0's synthetic ground truth moved by its own velocity columns over frame * 0.1 s ->
    (boxes [20, 9] fp32, labels [20] int64, ids [20] int32 = the row index), on the host"""
    import torch
    boxes, labels = frame_ground_truth(0, seed, pc_range, num_classes)
    boxes = boxes.clone()
    boxes[:, :2] += boxes[:, 7:9] * (frame * TRACK_FRAME_SECONDS)
    return boxes, labels, torch.arange(boxes.shape[0], dtype=torch.int32)


def mot_eval_config(class_names, max_boxes):
    """TUMTraf class ranges for TUMTraf class names, the nuScenes detection ranges otherwise; a 2 m match distance and
    40 recall levels from 0.1 (core/evaluation.MotEvalConfig)"""
    from projects.mmdet3d_plugin.core import evaluation as E
    return E.MotEvalConfig(class_names=tuple(class_names), class_range=eval_config(class_names).class_range,
                           max_boxes_per_frame=max_boxes)


def track_frame(tracker, frame, boxes, scores, labels, device, want_history, score=None):
    """One frame's boxes ([n, 9], scores [n], labels [n], on either side) through the tracker -> dict(track_ids [n]
    as a list, and with ``want_history`` track_history {id: positions, oldest first}).  ``score(boxes, scores, labels,
    det_track, count)`` receives the padded device tensors of the step (--eval track)."""
    import torch
    n, D = int(scores.shape[0]), tracker.max_dets
    if n > D:
        raise SystemExit(f"--track: a frame has {n} boxes, the tracker takes {D}")
    b = torch.zeros((D, 9), dtype=torch.float32, device=device)
    s = torch.zeros(D, dtype=torch.float32, device=device)
    lab = torch.zeros(D, dtype=torch.int32, device=device)
    b[:n], s[:n], lab[:n] = boxes.float().to(device)[:, :9], scores.float().to(device), labels.to(device).to(torch.int32)
    count = torch.full((1,), n, dtype=torch.int32, device=device)
    det_track = tracker.step(b, s, lab, count, timestamp=frame * TRACK_FRAME_SECONDS)
    if score is not None:
        score(b, s, lab, det_track, count)
    ids = det_track[:n].cpu().tolist()
    out = dict(track_ids=ids)
    if want_history:
        t = tracker.tracks(confirmed=False)
        out["track_history"] = {int(k): h.tolist() for k, h in zip(t["ids"], t["history"])}
    return out


def nms_frame(boxes, scores, labels, iou_thr, device):
    """--nms rotate: class-aware rotated NMS of one frame's boxes ([n, >= 7] with the bottom z of get_bboxes, on
    either side) on the device -> (boxes, scores, labels of the kept rows, best first, on the device; their number)"""
    import torch
    from projects.mmdet3d_plugin import native_iou as NI
    n = int(scores.shape[0])
    if n > NI.NMS_MAX:
        raise SystemExit(f"--nms: a frame has {n} boxes, rotated NMS takes {NI.NMS_MAX}")
    boxes, scores, labels = boxes.to(device), scores.to(device), labels.to(device)
    keep_idx, count = NI.nms_rotated(boxes.float().contiguous(), scores.float().contiguous(), iou_thr,
                                     labels=labels.to(torch.int32).contiguous(), z_origin=0.0)
    kept = int(count.item())
    sel = keep_idx[:kept].long()
    return boxes[sel], scores[sel], labels[sel], kept


def eval_config(class_names):
    """TUMTraf constants for TUMTraf class names, the nuScenes detection constants otherwise"""
    from projects.mmdet3d_plugin.core import evaluation as E
    if all(n in E.TUMTRAF_CLASSES for n in class_names):
        return E.tumtraf_eval_config(class_names)
    return E.nuscenes_eval_config(class_names)


def iou_eval_config(class_names, mode="3d", iou_thr=None):
    """the package's IoU settings (core/evaluation.tumtraf_iou_config) for any class names; ground-truth velocity zero
    for TUMTraf names, as eval_config"""
    from projects.mmdet3d_plugin.core import evaluation as E
    kw = {}
    if iou_thr:
        ths = [float(t) for t in iou_thr]
        kw = dict(iou_ths=ths, iou_th_tp=0.5 if 0.5 in ths else ths[0])
    return E.IouEvalConfig(class_names=tuple(class_names), mode=mode,
                           gt_velocity_zero=all(n in E.TUMTRAF_CLASSES for n in class_names), **kw)


def run_frame(head, name, feats, metas):
    if name.startswith("cmtcoop"):
        (xv, iv), (xi_, ii) = feats
        outs = head([xv], [xi_], [iv] if iv is not None else None, [ii] if ii is not None else None, metas)
    else:
        x, xi = feats[0]
        outs = head([x], [xi] if xi is not None else None, metas)
    # outs: tuple over tasks of lists over levels (multi_apply); get_bboxes -> per sample [boxes, scores, labels]
    return head.get_bboxes(outs, metas)[0]


def main(argv=None):
    args = parse_args(argv)
    name = config_name(args.config)
    import torch
    if not torch.cuda.is_available():
        print("test.py: no HIP device -- the head runs through the gfx950 kernels only (no CPU path)",
              file=sys.stderr)
        return 2
    from projects.mmdet3d_plugin import get_precision, set_precision

    distributed = args.launcher != "none"
    rank, world = 0, 1
    if distributed:
        import torch.distributed as dist
        dist.init_process_group("nccl")
        rank, world = dist.get_rank(), dist.get_world_size()
        device = torch.device("cuda", int(os.environ.get("LOCAL_RANK", args.local_rank)))
    else:
        device = torch.device("cuda", args.gpu_id)
    torch.cuda.set_device(device)
    from projects.mmdet3d_plugin import native_img
    prev = get_precision()
    set_precision(args.precision)
    prev_img = native_img.img_precision()
    if args.img_precision is not None:
        native_img.set_img_precision(args.img_precision)
    try:
        return _run(args, name, device, rank, world, distributed)
    finally:
        set_precision(prev)   # the CLI may run inside another process (tests)
        native_img.set_img_precision(prev_img)


def _run(args, name, device, rank, world, distributed):
    import torch
    from projects.mmdet3d_plugin.mmcv_custom.ops.voxel import SPConvVoxelization
    from projects.mmdet3d_plugin.mmcv_custom.ops.voxel.spconv_voxelize import voxelize_batch

    if args.detector:
        from projects.mmdet3d_plugin import synthetic as S
        model, dcfg = build_detector_model(args, name, device)
        meta = S.make_head_cfg(name)[1]
        cfg = dcfg["pts_bbox_head"]
        vcfg = dict((dcfg["vehicle_model"] if name.startswith("cmtcoop") else dcfg)["pts_voxel_layer"])
    else:
        head, cfg, meta = build_head(args, name, device)
        vcfg = dict(meta["pts_voxel_layer"])
    vox = SPConvVoxelization(voxel_size=vcfg["voxel_size"], point_cloud_range=vcfg["point_cloud_range"],
                             max_num_points=vcfg["max_num_points"], max_voxels=vcfg["max_voxels"],
                             num_point_features=vcfg["num_point_features"]).eval()
    class_names = list(cfg["tasks"][0]["class_names"])
    want_nds = bool(args.eval) and "nds" in args.eval
    want_iou = bool(args.eval) and "iou" in args.eval
    evaluator = iou_evaluator = None
    if want_nds or want_iou:
        pcr = meta["point_cloud_range"]
    if want_nds:
        from projects.mmdet3d_plugin.core.evaluation import DetectionEvaluator
        if rank == 0:
            evaluator = DetectionEvaluator(eval_config(class_names), max(args.frames, 1), device)
    if want_iou and rank == 0:
        from projects.mmdet3d_plugin.core.evaluation import IouDetectionEvaluator
        iou_evaluator = IouDetectionEvaluator(iou_eval_config(class_names, args.iou_mode, args.iou_thr),
                                              max(args.frames, 1), device)

    tracker = None
    if args.track:
        if distributed:
            raise SystemExit("--track follows the frames in order: run it without a launcher")
        from projects.mmdet3d_plugin import native_track as NT
        tracker = NT.Tracker(class_names, device, max_dets=NT.MAX_DETS)

    mot_evaluator = None
    if args.eval and "track" in args.eval:
        from projects.mmdet3d_plugin.core.evaluation import TrackingEvaluator
        mot_evaluator = TrackingEvaluator(mot_eval_config(class_names, tracker.max_dets), max(args.frames, 1), device)

    def feed_track(frame):
        if mot_evaluator is None:
            return None
        gb, gl, gi = track_ground_truth(frame, args.seed, meta["point_cloud_range"], len(class_names))

        def score(b, s, lab, det_track, count):
            mot_evaluator.add(b, s, lab, det_track, count, gt_boxes=gb.to(device), gt_labels=gl.to(device),
                              gt_ids=gi.to(device), scene=0, step=frame)
        return score

    nms_thr = None
    if args.nms:
        nms_thr = args.nms_thr if args.nms_thr is not None else float((cfg.get("test_cfg") or {}).get("nms_thr", 0.2))

    visualizer, pictures = None, 0
    if args.show_dir and distributed:
        raise SystemExit("--show-dir draws the frames of one process: run it without a launcher")
    if args.show_dir:
        from projects.mmdet3d_plugin.core.visualizer import Visualizer, write_png
        visualizer = Visualizer(class_names, meta["point_cloud_range"], device=device)
        os.makedirs(args.show_dir, exist_ok=True)

    def show_frame(frame, points, boxes, scores, labels, track, cams):
        """--show-dir: the frame's pictures; the boxes carry the bottom z of get_bboxes, the ground truth the centre"""
        kw = dict(boxes=boxes.float().to(device), scores=scores.float().to(device), labels=labels.to(device),
                  score_thr=args.show_score_thr, z_origin=0.0, gt_z_origin=0.5)
        if mot_evaluator is not None:
            kw["gt_boxes"], kw["gt_labels"] = track_ground_truth(frame, args.seed, meta["point_cloud_range"], len(class_names))[:2]
        elif want_nds or want_iou:
            kw["gt_boxes"], kw["gt_labels"] = frame_ground_truth(frame, args.seed, pcr, len(class_names))
        if tracker is not None:
            kw["track_ids"] = track["track_ids"]
            kw["trails"] = tracker.tracks(confirmed=False)["history"]
        write_png(os.path.join(args.show_dir, f"{frame:06d}_bev.png"), visualizer.bev(points, **kw))
        n, v0 = 1, 0
        for frames, l2i in cams:
            pics = visualizer.cameras(frames, l2i, points=points, **kw).cpu()
            for v in range(pics.shape[0]):
                write_png(os.path.join(args.show_dir, f"{frame:06d}_cam{v0 + v}.png"), pics[v])
            v0 += int(pics.shape[0])
            n += int(pics.shape[0])
        return n

    empty_gt = []   # per frame, a device count of the ground truth without points (--count-gt-points)

    def feed(frame, boxes, scores, labels, points=None):
        gb, gl = frame_ground_truth(frame, args.seed, pcr, len(class_names))
        # the head's boxes are on the device already; the detector's result dict (bbox3d2result) is on the host
        if iou_evaluator is not None:   # every ground-truth box counts, with or without --count-gt-points
            iou_evaluator.add(boxes.to(device), scores.to(device), labels.to(device), None, gb.to(device), gl.to(device))
        if evaluator is None:
            return
        if points is None:
            evaluator.add(boxes.to(device), scores.to(device), labels.to(device), None, gb.to(device), gl.to(device))
            return
        gb = gb.to(device)
        num_pts = gt_point_counts(gb, points)
        empty_gt.append((num_pts == 0).sum())
        evaluator.add(boxes.to(device), scores.to(device), labels.to(device), None, gb, gl.to(device), num_pts)

    results = []
    t0 = time.perf_counter()
    with torch.no_grad():
        for f in range(rank, args.frames, world):
            if args.detector:
                cams = [] if visualizer is not None else None
                kw, points = detector_frame_inputs(name, dcfg, meta, f, args, device, show=cams)
            else:
                feats, metas, points = frame_inputs(name, meta, f, args, device)
            # the voxel layer of the detector (cmt.py:88-113 + HardSimpleVFE), per agent
            vox_stats = []
            for pts in points:
                mean, nums, coors = voxelize_batch(vox, [pts], num_features=vcfg["num_point_features"])
                vox_stats.append(dict(voxels=int(mean.shape[0]), points_kept=int(nums.sum().item())))
            if args.detector:
                res = model(return_loss=False, **kw)[0]["pts_bbox"]
                boxes, scores, labels = res["boxes_3d"], res["scores_3d"], res["labels_3d"]
            else:
                boxes, scores, labels = run_frame(head, name, feats, metas)
            nms = {}
            if args.nms:
                boxes, scores, labels, nms["nms_kept"] = nms_frame(boxes, scores, labels, nms_thr, device)
            if (want_nds or want_iou) and not distributed:   # the boxes as tensors: no lists, no JSON
                feed(f, boxes.float(), scores.float(), labels, points if args.count_gt_points else None)
            track = {}
            if tracker is not None:
                track = track_frame(tracker, f, boxes, scores, labels, device, args.format_only, feed_track(f))
            if visualizer is not None:
                pictures += show_frame(f, points, boxes, scores, labels, track, (cams or []) if args.detector else [])
            results.append(dict(frame=f, voxels=vox_stats, **track, **nms,
                                boxes_3d=boxes.float().cpu().tolist(), scores_3d=scores.float().cpu().tolist(),
                                labels_3d=labels.cpu().tolist(),
                                points_xyz=torch.cat([p[:, :3][torch.isfinite(p[:, :3]).all(1)] for p in points]).cpu().tolist()
                                if args.format_only else None))
    torch.cuda.synchronize()
    elapsed = time.perf_counter() - t0
    if distributed:
        import torch.distributed as dist
        gathered = [None] * world
        dist.all_gather_object(gathered, results)
        results = sorted([r for part in gathered for r in part], key=lambda r: r["frame"])
        dist.destroy_process_group()
    if rank != 0:
        return 0
    if args.out:
        with open(args.out, "w") as fh:
            json.dump(dict(config=name, class_names=class_names,
                           frames=[{k: v for k, v in r.items() if k not in ("points_xyz", "track_history")}
                                   for r in results]), fh)
        print(f"writing results to {args.out}")
    if args.format_only:
        import numpy as np
        from projects.mmdet3d_plugin.core.openlabel import boxes_to_detections, detections_to_openlabel, reset_track_uuids
        reset_track_uuids()   # a run's track ids start at 0: no uuid of an earlier run in this process
        for r in results:
            dets = boxes_to_detections(np.asarray(r["boxes_3d"]).reshape(-1, 9), np.asarray(r["scores_3d"]),
                                       np.asarray(r["labels_3d"]), class_names,
                                       points_xyz=np.asarray(r["points_xyz"]), bbox_classes=args.bbox_classes,
                                       bbox_score=args.bbox_score, track_ids=r.get("track_ids"),
                                       histories=r.get("track_history"))
            detections_to_openlabel(dets, filename=f"frame_{r['frame']:06d}.json",
                                    output_folder_path=args.openlabel_dir, frame_id=r["frame"])
        print(f"wrote {len(results)} OpenLABEL file(s) to {args.openlabel_dir}")
    if visualizer is not None:
        print(f"wrote {pictures} pictures to {args.show_dir}")
    if args.eval:
        n = [len(r["scores_3d"]) for r in results]
        s = [x for r in results for x in r["scores_3d"]]
        stats = dict(metric=args.eval, frames=len(results), boxes_per_frame=sum(n) / max(len(n), 1),
                     score_max=max(s) if s else None, score_mean=sum(s) / len(s) if s else None,
                     voxels_per_frame=sum(v["voxels"] for r in results for v in r["voxels"]) / max(len(results), 1),
                     seconds=round(elapsed, 4),
                     note="synthetic frames: no annotations offline, so no nuScenes AP")
        print(json.dumps(stats))
    if want_nds or want_iou:
        if distributed:   # rank 0 evaluates the gathered results
            for r in results:
                feed(r["frame"], torch.tensor(r["boxes_3d"], dtype=torch.float32, device=device).reshape(-1, 9),
                     torch.tensor(r["scores_3d"], dtype=torch.float32, device=device),
                     torch.tensor(r["labels_3d"], dtype=torch.int64, device=device))
    if want_nds:
        extra = dict(gt_without_points=int(sum(int(c.item()) for c in empty_gt))) if args.count_gt_points else {}
        print(json.dumps(dict(metric="nds", frames=len(results), gt_per_frame=GT_PER_FRAME, **extra, **evaluator.compute())))
    if want_iou:
        m = iou_evaluator.compute()
        m["label_mean_iou"] = {k: (None if v != v else v) for k, v in m["label_mean_iou"].items()}   # no match: null
        print(json.dumps(dict(metric="iou_ap", frames=len(results), gt_per_frame=GT_PER_FRAME, **m)))
    if mot_evaluator is not None:
        m = mot_evaluator.compute()

        def clean(v):   # a class without ground truth, or without a match: null
            return None if isinstance(v, float) and v != v else v
        per_class = {n: {k: clean(d[k]) for k in ("mota", "motp", "recall", "ids", "frag", "fp", "fn", "amota", "amotp")}
                     for n, d in m["label_metrics"].items()}
        print(json.dumps(dict(metric="mot", frames=len(results), gt_per_frame=GT_PER_FRAME, amota=clean(m["amota"]),
                              amotp=clean(m["amotp"]), mota=clean(m["mota"]), motp=clean(m["motp"]),
                              recall=clean(m["recall"]), ids=m["ids"], frag=m["frag"], label_metrics=per_class)))
    return 0


if __name__ == "__main__":
    sys.exit(main())
