"""Tracking evaluation on the device (cmt_mot_eval_*, csrc/moteval.hip) against tests/_mot_ref.py, the numpy
restatement of the contract in include/cmt_hip.h.  Counters, npos, tp_score, thresholds and the best slot are compared
exactly, every float64 metric within 1e-9 * max(1, |v|) (the bar of tests/test_gpu_eval.py).  The seeded cases are those
of tests/_mot_cases.py; tests/test_mot_host.py holds the restatement to hand-worked answers and checks its uniqueness
assertion for the same cases on the CPU."""
import importlib.util
import json
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _mot_cases as MC  # noqa: E402
import _mot_ref as R  # noqa: E402

from conftest import PKG  # noqa: E402

pytestmark = pytest.mark.gpu
EXACT = ("npos", "run_max", "counters", "counters1")
FLOAT64 = ("dist_sum", "dist_sum1", "metrics", "class_sum")
TENSORS = ("pred_box", "pred_score", "pred_label", "pred_track", "pred_frame", "gt_box", "gt_label", "gt_frame", "gt_inst",
           "frame_tab")


@pytest.fixture(scope="module")
def NE(dev):
    from projects.mmdet3d_plugin import native_eval
    native_eval.mot_lib()
    return native_eval


def run_device(NE, inp, dev, **kw):
    t = [torch.from_numpy(np.ascontiguousarray(inp[k])).to(dev) for k in TENSORS]
    cfg = {k: inp[k] for k in ("num_scenes", "max_steps", "class_range", "dist_th", "recall", "max_gt_tracks")}
    out = NE.mot_eval(*t, **cfg, **kw)
    torch.cuda.synchronize()
    return {k: v.cpu().numpy() for k, v in out.items()}


def same_bits(a, b, what):
    assert a.dtype == b.dtype and a.shape == b.shape, what
    assert a.tobytes() == b.tobytes(), what


def compare(got, ref, what):
    for k in EXACT:
        assert np.array_equal(got[k], ref[k]), f"{what}: {k}\n{got[k]}\n{ref[k]}"
    for k in ("tp_score", "thr"):   # float32 values and NaN places
        assert np.array_equal(got[k], ref[k], equal_nan=True), f"{what}: {k}"
    best = ref["class_sum"][:, 2]
    assert np.array_equal(got["class_sum"][:, 2], best), f"{what}: best slot"
    worst = 0.0
    for k in FLOAT64:
        g, r = got[k].astype(np.float64), ref[k].astype(np.float64)
        assert np.array_equal(np.isnan(g), np.isnan(r)), f"{what}: NaN places of {k}"
        ok = ~np.isnan(r)
        err = np.abs(g[ok] - r[ok]) / np.maximum(1.0, np.abs(r[ok]))
        worst = max(worst, float(err.max()) if err.size else 0.0)
        assert (err <= 1e-9).all(), f"{what}: {k} off by {err.max():.3e} (bound 1e-9)"
    return worst


@pytest.mark.parametrize("name", list(MC.CASES))
def test_device_equals_the_restatement(NE, dev, name, parity_log):
    """scenes 1 and 3 of lengths 1, 2, 30; 1, 3 and 10 classes with an empty one; 0, 1, 63, 64, 65 ground-truth boxes and
    0, 1, 64, 65, 300 predictions per (frame, class); 1, 5 and 40 recall levels; row stride 11, shuffled rows, ignored
    rows of every kind (tests/_mot_cases.py)"""
    inp, ref = MC.case(name)
    got = run_device(NE, inp, dev)
    worst = compare(got, ref, name)
    parity_log.append(f"mot_eval {name}: worst float64 metric error {worst:.2e} (bound 1e-9), counters exact")


@pytest.mark.parametrize("name", ["edge64", "split"])
def test_one_chain_per_block_equals_one_block_bitwise(NE, dev, name):
    """a workspace budget of one byte forces one chain per block; the default holds every chain in one"""
    inp, ref = MC.case(name)
    one = run_device(NE, inp, dev)
    many = run_device(NE, inp, dev, workspace_bytes=1)
    for k in one:
        same_bits(one[k], many[k], f"{name}: {k} depends on the split")
    compare(many, ref, name + " (one chain per block)")


class RedZones:
    """every buffer of mot_eval between two guard zones"""
    PAD, FILL = 256, 0xA5

    def __init__(self, dev):
        self.dev, self.bufs = dev, []

    def __call__(self, name, shape, dtype):
        n = int(np.prod(shape)) * torch.empty((), dtype=dtype).element_size()
        raw = torch.full((n + 2 * self.PAD,), self.FILL, dtype=torch.uint8, device=self.dev)
        self.bufs.append((name, raw, n))
        return raw[self.PAD:self.PAD + n].view(dtype).reshape(shape)

    def check(self):
        assert len(self.bufs) >= 20
        for name, raw, n in self.bufs:
            assert bool((raw[:self.PAD] == self.FILL).all()), f"{name}: written below the buffer"
            assert bool((raw[self.PAD + n:] == self.FILL).all()), f"{name}: written beyond the buffer"


@pytest.mark.parametrize("name", ["edge64", "big300", "sweep"])
def test_red_zones_and_two_runs_bitwise(NE, dev, name):
    """guard zones around every output and workspace buffer stay untouched, the buffers' initial bytes (0xA5 here,
    whatever torch.empty leaves in the first run) do not matter, and two runs agree bit for bit"""
    inp, ref = MC.case(name)
    first = run_device(NE, inp, dev)
    zones = RedZones(dev)
    second = run_device(NE, inp, dev, alloc=zones)
    zones.check()
    for k in first:
        same_bits(first[k], second[k], f"{name}: {k} differs between two runs")


def _device_frame(f, dev):
    return (torch.from_numpy(f["boxes"]).to(dev), torch.from_numpy(f["scores"]).to(dev), torch.from_numpy(f["labels"]).to(dev),
            torch.tensor([f["count"]], dtype=torch.int32, device=dev))


def test_tracker_into_evaluator_end_to_end(dev, parity_log):
    """moving_scene seeds 0-7 (one scene each) through Tracker.step into TrackingEvaluator.add, nothing read back on
    the way: no id switch for any class at any achieved recall level, and the same numbers as the restatement fed with
    the tracker's ids"""
    from projects.mmdet3d_plugin import native_track as NT
    from projects.mmdet3d_plugin import synthetic as S
    from projects.mmdet3d_plugin.core import evaluation as E
    D, names = 32, ["a", "b", "c"]
    cfg = E.MotEvalConfig(class_names=names, max_gt_tracks=16, max_boxes_per_frame=D)
    ev = E.TrackingEvaluator(cfg, 8 * 30, dev)
    trk = NT.Tracker(names, dev, max_dets=D, gate=2.0, max_age=3)
    rows, tracks = [], []
    for seed in range(8):
        trk.reset()
        for t, f in enumerate(S.moving_scene(seed, pad_to=D, with_truth=True)):
            b, s, lab, count = _device_frame(f, dev)
            det_track = trk.step(b, s, lab, count, timestamp=f["timestamp"])
            ev.add(b, s, lab, det_track, count, gt_boxes=torch.from_numpy(f["gt_boxes"]).to(dev),
                   gt_labels=torch.from_numpy(f["gt_labels"]).to(dev), gt_ids=torch.from_numpy(f["gt_ids"]).to(dev), scene=seed)
            tracks.append(det_track.clone())
            rows.append((f, seed, t))
    res = {k: v.cpu().numpy() for k, v in ev.run().items()}
    tracks = torch.stack(tracks).cpu().numpy()
    achieved = ~np.isnan(res["thr"])
    assert achieved.any(axis=1).all() and (res["npos"] == [8 * 30 * 4] * 3).all()
    assert (res["counters"][:, :, 3][achieved] == 0).all(), "an id switch in a scene the tracker keeps pure"
    assert (res["counters1"][:, 3] == 0).all() and (res["counters1"][:, 0] > 0).all()
    # the restatement on the same rows
    live = np.arange(D)
    inp = dict(pred_box=np.concatenate([f["boxes"] for f, _, _ in rows]),
               pred_score=np.concatenate([f["scores"] for f, _, _ in rows]),
               pred_label=np.concatenate([np.where(live < f["count"], f["labels"], -1) for f, _, _ in rows]).astype(np.int32),
               pred_track=tracks.reshape(-1), pred_frame=np.repeat(np.arange(len(rows)), D).astype(np.int32),
               gt_box=np.concatenate([f["gt_boxes"] for f, _, _ in rows]),
               gt_label=np.concatenate([f["gt_labels"] for f, _, _ in rows]),
               gt_frame=np.repeat(np.arange(len(rows)), 12).astype(np.int32),
               gt_inst=np.concatenate([f["gt_ids"] for f, _, _ in rows]),
               frame_tab=np.array([(s, t) for _, s, t in rows], dtype=np.int32), num_scenes=8, max_steps=30,
               class_range=cfg.class_range, dist_th=cfg.dist_th, recall=cfg.recall_levels(), max_gt_tracks=16)
    worst = compare(res, R.evaluate(**inp), "tracker -> evaluator")
    m = ev.compute()
    assert m["ids"] == 0 and 0.0 < m["amota"] <= 1.0 and 0.0 <= m["amotp"] < 2.0
    parity_log.append(f"mot_eval tracker end to end: AMOTA {m['amota']:.4f} AMOTP {m['amotp']:.4f} IDS {m['ids']}, "
                      f"worst float64 metric error {worst:.2e} (bound 1e-9)")


def test_cli_eval_track(dev, capsys):
    """tools/test.py --track --eval track prints one JSON line metric="mot" """
    spec = importlib.util.spec_from_file_location("cmt_test_cli_mot", os.path.join(PKG, "tools", "test.py"))
    cli = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(cli)
    rc = cli.main(["cmt_lidar_nus", "--synthetic", "--track", "--frames", "3", "--num-query", "32", "--num-layers", "1",
                   "--points", "1000", "--eval", "track"])
    assert rc == 0
    lines = [json.loads(ln) for ln in capsys.readouterr().out.splitlines() if ln.startswith("{")]
    mot = [d for d in lines if d.get("metric") == "mot"]
    assert len(mot) == 1
    d = mot[0]
    assert d["frames"] == 3 and "amota" in d and "amotp" in d
    assert len(d["label_metrics"]) == 10
    for m in d["label_metrics"].values():
        assert set(m) >= {"mota", "motp", "recall", "ids", "frag", "fp", "fn"}
