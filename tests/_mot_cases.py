"""Seeded inputs for the tracking evaluation (tests/test_mot_host.py checks on the CPU that the restatement's
uniqueness assertion holds for every one of them, tests/test_gpu_mot.py runs them on the device).

A case is a set of scenes; a class has a fixed population of objects per scene, on a grid ``spacing`` metres apart (a
small spacing leaves several admissible pairs per object).  Per frame an object is detected with probability 1 - p_drop
at a noisy position, under its track id, which changes now and then (id switches); false boxes are added.  Scores are
multiples of 1 / 64 (ties, also at thresholds).  ``junk`` adds rows the contract ignores: NaN boxes, a NaN score, labels
-1 and C, track -1, inst -1 and max_gt_tracks, a frame outside the table, a box outside the class range.  The rows
are shuffled over frames, the boxes have a row stride of 11.
"""
from functools import lru_cache

import numpy as np

import _mot_ref as R

LD = 11
MAX_GT_TRACKS = 700
RANGE = 500.0

#          scene lengths, R, per class (objects, false boxes, p_drop), junk
CASES = dict(
    tiny=dict(lengths=(1,), R=1, classes=[(1, 0, 0.0)], junk=False, seed=1),
    exact64=dict(lengths=(2,), R=1, classes=[(64, 0, 0.0)], junk=False, seed=2),
    edge64=dict(lengths=(2,), R=5, classes=[(63, 1, 0.0), (64, 1, 0.0), (0, 3, 0.0)], junk=True, seed=3),
    big300=dict(lengths=(2,), R=5, classes=[(65, 235, 0.0), (1, 0, 0.5), (0, 0, 0.0)], junk=False, seed=4),
    split=dict(lengths=(1, 2, 5), R=5, classes=[(5, 2, 0.2), (0, 1, 0.0), (3, 1, 0.3)], junk=True, seed=5),
    sweep=dict(lengths=(1, 2, 30), R=40,
               classes=[(6, 2, 0.15), (1, 1, 0.3), (0, 0, 0.0), (4, 0, 0.1), (2, 3, 0.2), (3, 1, 0.0), (5, 1, 0.25),
                        (1, 0, 0.0), (2, 2, 0.5), (3, 0, 0.1)], junk=True, seed=6),
)


def build(name):
    """-> dict of numpy inputs (the arguments of _mot_ref.evaluate) for the case"""
    spec = CASES[name]
    rng = np.random.RandomState(spec["seed"])
    C, lengths = len(spec["classes"]), spec["lengths"]
    table, pred, gt = [], [], []   # pred rows: (x, y, score, label, track, frame); gt rows: (x, y, label, frame, inst)
    next_track = 0
    for scene, length in enumerate(lengths):
        first = len(table)
        table += [(scene, t) for t in range(length)]
        inst0 = 0
        for c, (n_obj, n_false, p_drop) in enumerate(spec["classes"]):
            cols = max(1, int(np.ceil(np.sqrt(max(n_obj, 1)))))
            idx = np.arange(n_obj)
            pos = np.stack([(idx % cols) * 3.0 + 40.0 * c, (idx // cols) * 3.0 - 60.0 * scene], 1) + rng.uniform(-0.4, 0.4, (n_obj, 2))
            vel = rng.uniform(-1.0, 1.0, (n_obj, 2))
            tid = np.arange(next_track, next_track + n_obj)
            next_track += n_obj
            for t in range(length):
                f = first + t
                truth = pos + vel * (0.1 * t)
                switch = rng.uniform(size=n_obj) < 0.05
                tid = np.where(switch, np.arange(next_track, next_track + n_obj), tid)
                next_track += n_obj
                for o in range(n_obj):
                    gt.append((truth[o, 0], truth[o, 1], c, f, inst0 + o))
                    if rng.uniform() >= p_drop:
                        x, y = truth[o] + rng.uniform(-0.5, 0.5, 2)
                        pred.append((x, y, rng.randint(8, 60) / 64.0, c, tid[o], f))
                for _ in range(n_false):
                    x, y = rng.uniform(-20, 20, 2) + (40.0 * c, -60.0 * scene)
                    pred.append((x, y, rng.randint(4, 40) / 64.0, c, next_track, f))
                    next_track += 1
            inst0 += n_obj
    F = len(table)
    if spec["junk"]:
        nan = float("nan")
        pred += [(nan, 0.0, 0.5, 0, 1, 0), (0.0, nan, 0.5, 0, 1, 0), (1.0, 1.0, nan, 0, 1, 0), (1.0, 1.0, 0.5, -1, 1, 0),
                 (1.0, 1.0, 0.5, C, 1, 0), (1.0, 1.0, 0.9, 0, -1, 0), (1.0, 1.0, 0.9, 0, 1, F), (1.0, 1.0, 0.9, 0, 1, -1),
                 (RANGE, 1.0, 0.9, 0, 1, 0), (float("inf"), 1.0, 0.9, 0, 1, 0)]
        gt += [(nan, 0.0, 0, 0, 0), (1.0, 1.0, -1, 0, 0), (1.0, 1.0, C, 0, 0), (1.0, 1.0, 0, 0, -1),
               (1.0, 1.0, 0, 0, MAX_GT_TRACKS), (1.0, 1.0, 0, F, 0), (1.0, RANGE, 0, 0, 0)]
    pred = [pred[i] for i in rng.permutation(len(pred))]
    # the ground truth of one frame stays in annotation order; the frames interleave
    order = sorted(range(len(gt)), key=lambda i: (rng.randint(0, 3), i))
    gt = [gt[i] for i in order]
    pred, gt = np.array(pred, dtype=np.float64).reshape(-1, 6), np.array(gt, dtype=np.float64).reshape(-1, 5)
    pbox = rng.uniform(-1, 1, (len(pred), LD)).astype(np.float32)
    gbox = rng.uniform(-1, 1, (len(gt), LD)).astype(np.float32)
    pbox[:, :2], gbox[:, :2] = pred[:, :2], gt[:, :2]
    return dict(pred_box=pbox, pred_score=pred[:, 2].astype(np.float32), pred_label=pred[:, 3].astype(np.int32),
                pred_track=pred[:, 4].astype(np.int32), pred_frame=pred[:, 5].astype(np.int32), gt_box=gbox,
                gt_label=gt[:, 2].astype(np.int32), gt_frame=gt[:, 3].astype(np.int32), gt_inst=gt[:, 4].astype(np.int32),
                frame_tab=np.array(table, dtype=np.int32), num_scenes=len(lengths), max_steps=max(lengths),
                class_range=[RANGE] * C, dist_th=[2.0] * C, recall=R.recall_levels(spec["R"], 0.1),
                max_gt_tracks=MAX_GT_TRACKS)


@lru_cache(maxsize=None)
def case(name):
    """-> (inputs, the restatement's result); computed once and shared, not to be modified"""
    inp = build(name)
    return inp, R.evaluate(**inp)
