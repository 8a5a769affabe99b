"""Bit-level fingerprint of the data-path kernels (ptsprep, ptsaug, gtdb, track, boxiou, deteval): a fixed list of
small seeded cases through the public wrappers (native_pts, native_aug, native_gtdb, native_track, native_iou,
native_eval), one line per case with the SHA-256 of the raw output bytes.  Run it on two builds, each in its own
process, and compare the outputs line by line: a refactor of the kernels or wrappers must leave every line equal.

    python dev/data_bits.py [--out FILE]

The shapes are the tests' edge shapes: rows around the 1024-row tile, boxes around the 64-box chunk and the
256-thread pass, the tracker's and the NMS's caps, count words on and off.  Inputs come from a numpy generator seeded
by the case's name; every output buffer the kernels may leave partly unwritten is allocated as zeros.  Needs a HIP
device and the built library; the whole list runs in seconds.
"""
import argparse
import hashlib
import os
import sys
import zlib

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (os.path.join(ROOT, "cmt-cooperative-perception_amd"), ROOT):
    if p not in sys.path:
        sys.path.insert(0, p)

T = 1024
RANGE = [-40.0, -40.0, -4.0, 40.0, 40.0, 2.0]
ALL = dict(angle=0.3, scale=1.04, trans=[0.4, -0.3, 0.1], flip_h=True, flip_v=True)


def sha(t):
    return hashlib.sha256(t.detach().cpu().contiguous().view(torch.uint8).numpy().tobytes()).hexdigest()[:32]


def gen(name):
    return np.random.RandomState(zlib.crc32(name.encode()))


def cloud(g, n, F):
    p = g.uniform(-1, 1, (n, F)).astype(np.float32)
    p[:, :2] *= np.float32(48)
    p[:, 2] = p[:, 2] * np.float32(3.5) - np.float32(1)
    p[:, 3:] = g.uniform(0, 255, (n, F - 3)).astype(np.float32)
    return p


def boxes_of(g, m, D=7, spread=30.0):
    b = np.zeros((m, D), np.float32)
    b[:, :2] = g.uniform(-spread, spread, (m, 2))
    b[:, 2] = g.uniform(-2, 0, m)
    b[:, 3:6] = g.uniform(1.5, 6.0, (m, 3))
    b[:, 6] = g.uniform(-3.5, 3.5, m)
    if D > 7:
        b[:, 7:9] = g.uniform(-5, 5, (m, 2))
    return b


def rigid(g, shift):
    a = g.uniform(-np.pi, np.pi)
    m = np.eye(4)
    m[:2, :2] = [[np.cos(a), -np.sin(a)], [np.sin(a), np.cos(a)]]
    m[:3, 3] = g.uniform(-shift, shift, 3) * [1, 1, 0.1]
    return m


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("data_bits needs a HIP device")
    from projects.mmdet3d_plugin import native_aug as NA
    from projects.mmdet3d_plugin import native_eval as NE
    from projects.mmdet3d_plugin import native_gtdb as NG
    from projects.mmdet3d_plugin import native_iou as NI
    from projects.mmdet3d_plugin import native_pts as NP
    from projects.mmdet3d_plugin import native_track as NT
    dev = torch.device("cuda:0")
    lines = []
    i32 = dict(dtype=torch.int32, device=dev)

    def up(a):
        return torch.from_numpy(np.ascontiguousarray(a)).to(dev)

    def word(v):
        return None if v is None else torch.tensor([v], **i32)

    def say(name, *tensors):
        torch.cuda.synchronize()
        lines.append(f"{name}: " + " ".join(sha(t) for t in tensors))
        print(lines[-1], flush=True)

    # ---- cmt_pts_prepare
    for n in (T - 1, T, T + 1, 2 * T + 1, 257 * T + 1):
        name = f"prepare_points n {n}"
        g = gen(name)
        p = cloud(g, n, 5)
        cuts = [0, n // 3, 2 * n // 3, n]
        segs = []
        for s in range(3):
            m = rigid(g, 2.0)
            segs.append(dict(points=up(p[cuts[s]:cuts[s + 1]]), rotation=m[:3, :3] if s else None,
                             translation=m[:3, 3] if s else None, remove_close=1.0 if s else 0.0, time_col=4, time=0.05 * s))
        say(name, *NP.prepare_points(segs, use_dim=[0, 1, 2, 3, 4], load_dim=5, agent_transform=rigid(g, 5.0),
                                     point_cloud_range=RANGE))
        say(name + " plain", *NP.prepare_points(segs[:1], use_dim=[0, 1, 2, 3], load_dim=5))

    # ---- cmt_points_in_boxes, cmt_pts_augment, cmt_boxes_augment
    for n in (T - 1, T + 1):
        for m in (0, 1, 64, 65, 300):
            name = f"points_in_boxes N {n} M {m}"
            g = gen(name)
            count = None if m % 2 else n - 40
            say(name, *NA.points_in_boxes(up(cloud(g, n, 4)), up(boxes_of(g, m, 9 if m % 2 else 7)), count=word(count)))
    for k, n in enumerate((T - 1, T, T + 1, 2 * T + 1, 257 * T + 1)):
        name = f"augment_points n_src {n}"
        g = gen(name)
        src, paste, pb = cloud(g, n, 5), cloud(g, 7, 5), boxes_of(g, 33)
        n_in = n + 7
        say(name, *NA.augment_points(up(src), ALL, count=word(n - 5), paste_points=up(paste), paste_boxes=up(pb),
                                     paste_first=bool(k % 2), point_cloud_range=RANGE,
                                     shuffle=up(np.arange(n_in, dtype=np.int32)[::-1]) if k % 2 else None))
        say(name + " plain", *NA.augment_points(up(src[:, :3]), dict(angle=-0.6)))
    for n in (0, 1, 64, 65, 300):
        for D in (7, 9):
            name = f"augment_boxes n {n} D {D}"
            g = gen(name)
            say(name, *NA.augment_boxes(up(boxes_of(g, n, D, 45.0)), up(g.randint(-1, 5, n).astype(np.int64)), ALL,
                                        point_cloud_range=RANGE, num_classes=4, gravity=D == 9))

    # ---- cmt_gtdb_extract, cmt_gtdb_gather, cmt_gtdb_collide
    for n in (T - 1, T + 1, 2 * T + 1):
        for m in (1, 64, 65, 300):
            name = f"extract_objects N {n} M {m}"
            g = gen(name)
            rows = torch.zeros((4 * n, 5), dtype=torch.float32, device=dev)
            rows, offsets = NG.extract_objects(up(cloud(g, n, 5)), up(boxes_of(g, m, 7, 45.0)), count=word(n - 9 if m % 2 else None),
                                               out=rows)
            say(name, rows, offsets)
            if m == 65:
                off = offsets.cpu().numpy().astype(np.int64)
                lens = np.minimum(np.diff(off), 50)[:65]
                starts = np.concatenate([[0], np.cumsum(lens)])
                out = torch.zeros((int(starts[-1]) + 3, 5), dtype=torch.float32, device=dev)
                say(name + " gather", NG.gather_objects(rows, up(off[:65].astype(np.int32)), up(lens.astype(np.int32)),
                                                        up(starts[:-1].astype(np.int32)), up(g.uniform(-9, 9, (65, 3)).astype(np.float32)),
                                                        int(starts[-1]) + 3, out=out))
    for n_gt, n_s in ((0, 1), (10, 54), (10, 55), (100, 200), (212, 300)):
        name = f"collide n_gt {n_gt} n_s {n_s}"
        g = gen(name)
        group = np.sort(g.randint(0, 5, n_s))
        say(name, *NG.collide(up(boxes_of(g, n_gt + n_s, 7, 60.0)), n_gt, group))

    # ---- cmt_track_predict, cmt_track_update
    for Tn, D in ((65, 63), (65, 65), (512, 1024)):
        for pose in (False, True):
            name = f"tracker T {Tn} D {D}{' pose' if pose else ''}"
            g = gen(name)
            trk = NT.Tracker(["car", "bus", "bike"], dev, max_tracks=Tn, max_dets=D, use_velocity=pose)
            b = boxes_of(g, D, 9, 45.0)
            hashes = []
            for f in range(4):
                b[:, :2] += b[:, 7:9] * np.float32(0.1) + g.normal(0, 0.05, (D, 2)).astype(np.float32)
                order = g.permutation(D)
                ids = trk.step(up(b[order]), up(g.uniform(0, 1, D).astype(np.float32)), up((order % 3).astype(np.int32)),
                               word(D - 3 if f % 2 else None), dt=0.1, pose=rigid(g, 3.0) if pose else None)
                hashes.append(ids.clone())
            st, wk = trk.state, trk.work
            say(name, *hashes, st["trk_f"], st["trk_i"], st["hist"], st["counters"], wk["det_w"], wk["det_ok"], wk["live"],
                wk["cost"], wk["lsap_desc"], trk.det_slot)

    # ---- cmt_box_iou, cmt_box_nms, cmt_box_concat
    for n, m in ((1, 1), (64, 64), (65, 65), (300, 130)):
        name = f"box_iou {n} x {m}"
        g = gen(name)
        a, b = up(boxes_of(g, n, 9, 12.0)), up(boxes_of(g, m, 7, 12.0))
        say(name, *NI.box_iou(a, b, mode="both"))
        say(name + " counts z0", *NI.box_iou(a, b, mode="both", z_origin=0.0, n_a=word(n - 1), n_b=word(m + 5)))
        if n == m:
            say(name + " aligned", *NI.box_iou(a, b, mode="both", aligned=True))
    for n in (0, 1, 64, 65, 300, 2048):
        name = f"nms_rotated n {n}"
        g = gen(name)
        b, s = up(boxes_of(g, n, 7, 20.0 + n / 20)), up(g.uniform(-0.2, 1, n).astype(np.float32))
        lab = up(g.randint(0, 3, n).astype(np.int32))
        keep = torch.zeros(n, dtype=torch.uint8, device=dev)
        say(name, *NI.nms_rotated(b, s, 0.2, labels=lab, count=word(n - 2 if n > 2 else None), score_thr=0.05, keep=keep), keep)
        say(name + " agnostic 3d", *NI.nms_rotated(b, s, 0.1, use_3d=True))
    for cols in (7, 9):
        for tf in (False, True):
            name = f"concat_detections cols {cols}{' poses' if tf else ''}"
            g = gen(name)
            srcs = []
            for k, n in enumerate((5, 64, 65)):
                srcs.append((up(boxes_of(g, n, 9, 40.0))[:, :cols + (k % 2)], up(g.uniform(0, 1, n).astype(np.float32)),
                             up(g.randint(0, 3, n).astype(np.int32)), word(n - 2 if k else None)))
            poses = [None, rigid(g, 20.0), rigid(g, 20.0)] if tf else None
            say(name, *NI.concat_detections(srcs, poses, cols=cols))

    # ---- cmt_det_eval_*
    S_, M, G, C, ths = 4, 40, 10, 3, [0.5, 1.0, 2.0, 4.0]
    for counts in (False, True):
        name = f"det_eval{' counts' if counts else ''}"
        g = gen(name)
        gb = boxes_of(g, S_ * G, 9, 40.0)
        gl = g.randint(0, C, S_ * G).astype(np.int32)
        gs = np.repeat(np.arange(S_), G).astype(np.int32)
        src = g.randint(0, G, S_ * M) + np.repeat(np.arange(S_), M) * G
        pb = gb[src].copy()
        pb[:, :2] += g.normal(0, 0.8, (S_ * M, 2)).astype(np.float32)
        pb[:, 3:6] *= g.uniform(0.8, 1.25, (S_ * M, 3)).astype(np.float32)
        pl = np.where(g.rand(S_ * M) < 0.8, gl[src], g.randint(0, C, S_ * M)).astype(np.int32)
        ps = np.round(g.uniform(0, 1, S_ * M), 2).astype(np.float32)        # ties in the scores
        N_, G_ = S_ * M, S_ * G
        shapes = dict(tp=((4, N_), torch.uint8), match_gt=((4, N_), torch.int32), err=((4, 4, N_), torch.float64),
                      npos=((C,), torch.int32), md=((C, 4, 7, 101), torch.float64), ap=((C, 4), torch.float64),
                      tp_err=((C, 4), torch.float64))
        out = {k: torch.zeros(shape, dtype=dt, device=dev) for k, (shape, dt) in shapes.items()}
        NE.det_eval(up(pb), up(ps), up(pl), up(np.repeat(np.arange(S_), M).astype(np.int32)), up(gb), up(gl), up(gs),
                    up(g.randint(0, 3, G_).astype(np.int32)), num_samples=S_, class_range=[50.0, 40.0, 30.0],
                    yaw_period=[2 * np.pi, np.pi, 2 * np.pi], dist_ths=ths, dist_th_tp=2.0,
                    n_pred=word(N_ - 7) if counts else None, n_gt=word(G_ - 3) if counts else None, out=out)
        say(name, *(out[k] for k in shapes))

    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
