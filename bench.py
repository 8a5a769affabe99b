#!/usr/bin/env python3
"""Decoder-frame throughput of the MI355X-native CMT head (BASELINE.json metric:
"decoder frames/sec at 900 queries x (BEV+6-cam) tokens").

Default workload (BASELINE.json configs[2], the metric's own shape): CMT
camera+LiDAR nuScenes-shape synthetic frame -- BEV [1, 512, 180, 180] plus
6 views x [256, 40, 100] pre-extracted image features (32 400 + 24 000 =
56 400 memory tokens), 900 queries, 6-layer decoder, the whole CmtHead forward
per step: shared_conv, BEV / RV / query coordinate encodings, decoder, task
heads, box epilogue, at the reference's numerics ('ref' policy: every fp32
GEMM of the reference as a three-pass split-f16 MFMA product, each operand kept
to max(2^-22 |x|, 2^-25) (include/cmt_hip.h CMT_F16P); fp32 self-attention; fp16 flash cross-attention core with fp16 P
and output, flash-attn 0.2.2).
The ~30k-point voxel scatter-mean is timed separately.
Inputs and weights are resident in HBM before the timed region; one step = one
frame per rank, captured as a HIP graph.  The bf16 speed policy (bf16 GEMM operands, bf16
attention core: ~2.5 % of each output's scale from the fp32 reference, outside
north_star's 1e-3) is timed on the same frame and reported beside the headline
as ``bf16_policy``.

Other workloads (--workload): lidar (configs[1], 32 400 tokens), coop
(configs[3] forward: vehicle 36 400 + infrastructure 44 400 tokens), stress4
(configs[4]: 4 agents x 48 400 tokens, 1500 queries, fp16 policy).

Usage: python bench.py [--gpus N] [--steps K] [--warmup W] [--dump-outputs DIR] [--full]
A plain run sets up, warms up, times the K steps and prints the headline line
(metric, value, unit, ms_per_step, dtype, config).  --dump-outputs DIR then
writes what the last timed step returned (every tensor of the head's output,
float32) as DIR/<name>.npy; the inputs and weights are seeded, so two builds
can be compared output for output.  --full adds everything else to the line:
the dominant kernel's roofline and PMC traffic, the weight-only-recomputed
and bf16-policy frames, the voxel scatter-mean, the other configs' side keys
and the CPU baseline (each with its own --no-* switch).
With --gpus N > 1 and no torch.distributed environment, this process starts
the N ranks itself (python -m torch.distributed.run, before any GPU call
here) and exits with their status.  Frames are independent, so ranks share
nothing on the data path (weak scaling); the only collectives are the
barrier and the max-over-ranks of the elapsed time.  Prints ONE JSON line on
rank 0.
"""
import argparse
import glob
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(ROOT, "cmt-cooperative-perception_amd"))
sys.path.insert(0, ROOT)

import torch  # noqa: E402  (importing torch does not initialise the GPU)
import torch.distributed as dist  # noqa: E402

from projects.mmdet3d_plugin import dp, native, set_precision  # noqa: E402
from projects.mmdet3d_plugin import synthetic as S  # noqa: E402
from projects.mmdet3d_plugin.mmcv_custom.ops.voxel import SPConvVoxelization  # noqa: E402
from projects.mmdet3d_plugin.profiling import region_timer  # noqa: E402
from projects.mmdet3d_plugin.runtime import OPTIONS, options  # noqa: E402

PEAK_TFLOPS = {"bf16": 2500.0, "fp16": 2500.0}   # dense MFMA, MI355X_MICROARCH.md (no sparsity)
DTYPE_LABEL = {"bf16": "bf16", "fp16": "fp16",
               "ref": "fp32 (GEMMs as 3-pass split-f16 MFMA) + fp16 flash attention core: reference numerics",
               "exact": "fp32 (exact-f32 MFMA GEMMs) + fp16 flash attention core: reference numerics"}
C, NQ, NK, L, H = 256, 900, 32400, 6, 8
METRIC = "decoder frames/sec at 900 queries x (BEV+6-cam) tokens; 1/2/4/8 MI355X"
STRESS_YAWS = (0.0, 90.0, 180.0, -90.0)
# what the headline keeps like a weight pack (a function of the weights and the BEV grid only;
# the reference recomputes each per forward): engine._bev_pos_hidden / _bev_pos_rows / _query_bev_pos
WEIGHT_ONLY_KEPT = [
    "bev_embedding[0] (pos2embed of the 180x180 BEV grid, Linear 512->256, ReLU), cmt_head.py:436",
    "bev_embedding[2] over the same grid (the BEV position rows added to the memory rows), cmt_head.py:436",
    "bev_embedding(pos2embed(reference_points)) (the BEV half of query_pos), cmt_head.py:489",
]


def cross_attn_flops(nq=NQ, nk=NK, c=C):
    """Algorithmic FLOPs of one cross-attention core launch (QK^T + PV), SURVEY 8(d)."""
    return 4.0 * nq * nk * c


def decoder_frame_flops(nq=NQ, nk=NK, c=C, layers=L, ffn=1024):
    """F_layer = 12 Nq C^2 + 4 Nq^2 C + 4 Nk C^2 + 4 Nq Nk C + 4 Nq C F_ffn."""
    return layers * (12 * nq * c * c + 4 * nq * nq * c + 4 * nk * c * c + 4 * nq * nk * c + 4 * nq * c * ffn)


WORKLOADS = {
    # cfg: head config; agents: (meta prefix, camera yaws or None); nq: queries; precision: compute policy
    "fusion": dict(cfg="cmt_fusion_nus", agents=[("", S.NUS_YAWS)], nq=900, precision="ref", head="CmtHead",
                   desc="CMT camera+LiDAR nuScenes-shape (BASELINE configs[2]): BEV 512x180x180 + 6 views x "
                        "256x40x100 image feats (56400 tokens), 900 queries, 6-layer decoder, CmtHead forward "
                        "(shared_conv + BEV/RV/query encodings + decoder + task heads), batch 1 frame per GPU"),
    "lidar": dict(cfg="cmt_lidar_nus", agents=[("", None)], nq=900, precision="ref", head="CmtLidarHead",
                  desc="CMT-L (LiDAR-only) nuScenes-shape (BASELINE configs[1]): BEV 512x180x180 (32400 tokens), "
                       "900 queries, 6-layer decoder, CmtLidarHead forward, batch 1 frame per GPU"),
    "coop": dict(cfg="cmtcoop_fusion_tumtraf", agents=[("vehicle_", S.VEHICLE_YAWS), ("infrastructure_", S.INFRA_YAWS)],
                 nq=900, precision="ref", head="CmtHeadCoop",
                 desc="CMTCoop TUMTraf-shape forward (BASELINE configs[3] forward leg): vehicle BEV 180x180 + 1 cam, "
                      "infrastructure BEV 180x180 + 3 cams (36400 + 44400 tokens), 900 queries, 6-layer decoder per "
                      "agent, max fusion, CmtHeadCoop forward, batch 1 frame per GPU"),
    "stress4": dict(cfg="cmtcoop_fusion_tumtraf", agents=[(f"agent{i}_", STRESS_YAWS) for i in range(4)], nq=1500,
                    precision="fp16", head="CmtHeadCoop",
                    desc="CMTCoop 4-agent stress (BASELINE configs[4]): 4 x (BEV 180x180 + 4 cams) = 4 x 48400 "
                         "tokens, 1500 queries, 6-layer decoder per agent, max fusion over 4 agents, fp16, "
                         "batch 1 frame per GPU"),
}


def make_workload(name, seed, device=None, batch=1):
    """(head, head cfg, forward closure, per-agent memory lengths, oracle closure)
    for one synthetic frame of ``name`` (``batch`` frames per forward); tensors on
    ``device`` (CPU if None)."""
    w = WORKLOADS[name]
    head, cfg, _ = S.build_synthetic_head(w["cfg"], seed=0, num_query=w["nq"], device=device)
    inputs, nks, metas = [], [], [dict() for _ in range(batch)]
    for i, (prefix, yaws) in enumerate(w["agents"]):
        x = S.synthetic_bev(batch, 180, 180, seed=seed + 1 + 10 * i, device=device)
        xi = None
        if yaws is not None:
            xi = S.synthetic_img(batch * len(yaws), 40, 100, seed=seed + 2 + 10 * i, device=device)
            for b, m in enumerate(S.synthetic_metas(batch, yaws=yaws, prefix=prefix, seed=seed + 3 + 10 * i)):
                metas[b].update(m)
        inputs.append((prefix, x, xi))
        nks.append(180 * 180 + (0 if yaws is None else len(yaws) * 40 * 100))
    if len(inputs) == 1:
        _, x, xi = inputs[0]

        def fwd():
            return head([x], [xi] if xi is not None else None, metas)
    elif len(inputs) == 2:
        (_, xv, iv), (_, xi_, ii) = inputs

        def fwd():
            return head([xv], [xi_], [iv], [ii], metas)
    else:
        def fwd():
            return head.forward_agents(inputs, metas)
    fwd.metas = metas

    def oracle_fwd():
        from oracle import cmt_oracle as O
        oc = O.cfg_from_head_cfg(cfg)
        sd = S.head_state_dict(head)
        cpu = [(p, x.cpu(), None if xi is None else xi.cpu()) for p, x, xi in inputs]
        variant = "lidar" if name == "lidar" else "fusion"
        if len(cpu) == 1:
            return lambda: O.head_forward(oc, sd, cpu[0][1], cpu[0][2], metas, variant)
        return lambda: O.head_coop_forward(oc, sd, cpu, metas, variant)

    return head, cfg, fwd, nks, oracle_fwd


def cpu_threads():
    """Host threads for the CPU baseline: every CPU this process may run on,
    capped by OMP_NUM_THREADS when the launcher sets it (the GPU box sets it to
    its 16-CPU share; os.cpu_count() there reports the whole machine)."""
    n = len(os.sched_getaffinity(0)) if hasattr(os, "sched_getaffinity") else (os.cpu_count() or 1)
    omp = os.environ.get("OMP_NUM_THREADS")
    return max(1, min(n, int(omp))) if omp and omp.isdigit() else n


def cpu_baseline(workload, seconds, seed):
    """The oracle (CPU restatement, fp32 exact math, PyTorch CPU) on the same
    workload: one untimed warm-up frame, then the median of up
    to 20 timed frames within about ``seconds`` of host time (at least one)."""
    _, _, _, nks, oracle_fwd = make_workload(workload, seed)
    threads = cpu_threads()
    torch.set_num_threads(threads)
    run = oracle_fwd()
    times = []
    with torch.no_grad():
        run()   # warm-up (allocator, thread pool)
        t0 = time.perf_counter()
        while len(times) < 20 and (not times or time.perf_counter() - t0 < seconds):
            t = time.perf_counter()
            run()
            times.append(time.perf_counter() - t)
    times.sort()
    med = times[len(times) // 2]
    return {"value": round(1.0 / med, 4), "unit": "frames/s", "cores": threads, "kind": "port",
            "sample": f"1 warm-up + {len(times)} timed full {workload} frames (median; memory tokens "
                      f"{'+'.join(map(str, nks))}, {WORKLOADS[workload]['nq']} queries, 6 layers, shared_conv + "
                      f"coordinate encodings + decoder + task heads) through oracle/cmt_oracle.py in fp32 on "
                      f"{threads} host threads (torch.set_num_threads); median frame {med:.3f} s"}


def load_traffic(workload, nk):
    """HBM bytes per launch of the dominant kernel (the cross-attention core as
    the frame runs it) for THIS workload's shape, from the committed rocprofv3 PMC
    summary profiles/*_<workload>_attn_pmc_summary.json (FETCH_SIZE x2 gfx950
    correction + WRITE_SIZE, separate passes; dev/traffic_summary.py).
    Raises when no summary matches the workload and key length."""
    cands = sorted(glob.glob(os.path.join(ROOT, "profiles", f"*_{workload}_attn_pmc_summary.json")))
    for path in reversed(cands):
        with open(path) as f:
            s = json.load(f)
        if s.get("workload") == workload and int(s.get("nk", -1)) == int(nk):
            return s["hbm_bytes_per_launch"], os.path.relpath(path, ROOT)
    raise RuntimeError(f"no committed PMC traffic summary for workload {workload!r} at Nk={nk} under profiles/ "
                       "(collect one with dev/gpu_check.sh ... prof; or pass --no-traffic)")


def spawn_ranks(args):
    """--gpus N without a torch.distributed environment: start the N ranks as
    children (this process has not touched the GPU) and return their status."""
    return dp.spawn(os.path.abspath(__file__), sys.argv[1:], args.gpus)


def train_bench(workload, steps, warmup, env, dev, last=None):
    """BASELINE configs[3]: CMTCoop head DDP training step on TUMTraf-shape
    synthetic frames (vehicle BEV 180x180 + 1 cam, infrastructure BEV 180x180
    + 3 cams, 900 queries + DN groups from 20 GT boxes, 6 layers), one frame
    per rank: training forward, Hungarian-matched losses, backward on the
    native kernels, bucketed RCCL gradient all-reduce, clip + AdamW.  Returns
    (elapsed_max_s, steps_per_s_whole_job, last loss, memory lengths, params);
    ``last`` (a list) receives the latest step's predictions and loss."""
    from projects.mmdet3d_plugin.trainer import Trainer
    head, cfg, _, nks, _ = make_workload(workload, seed=dp.frame_seed(0, env), device=dev)
    w = WORKLOADS[workload]
    head.train()
    seed = dp.frame_seed(0, env)
    B = 1
    agents = []
    metas = [dict()]
    for i, (prefix, yaws) in enumerate(w["agents"]):
        x = S.synthetic_bev(B, 180, 180, seed=seed + 1 + 10 * i, device=dev)
        xi = None
        m = [dict()]
        if yaws is not None:
            xi = S.synthetic_img(len(yaws), 40, 100, seed=seed + 2 + 10 * i, device=dev)
            m = S.synthetic_metas(1, yaws=yaws, seed=seed + 3 + 10 * i)
        agents.append((x, xi, m))
    gtb, gtl = S.synthetic_gt(B, list(head.pc_range), head.num_classes[0], n=20, seed=seed, device=dev)
    loss = [None]
    # freeze_gc: while the steps run, the long-lived objects stay out of the cyclic collector's
    # scans (process-wide gc.freeze, trainer.py), undone when the Trainer closes
    with Trainer(head, lr=1e-4, weight_decay=0.01, max_norm=35.0, freeze_gc=True) as tr:
        def step():
            preds = head.forward_train(agents, metas, gtb, gtl)
            loss[0] = tr.step(head.loss(gtb, gtl, [[p] for p in preds]))
            if last is not None:
                last[:] = [dict(preds=preds, loss=loss[0])]
        elapsed, value = dp.timed_frames(step, steps=steps, warmup=warmup, env=env,
                                         sync=torch.cuda.synchronize, device=dev)
        nparam = sum(p.numel() for p in tr.fp.params)
    return elapsed, value, float(loss[0].item()), nks, nparam


def capture(step, last=None):
    """Warm the step eagerly, then capture it as a HIP graph; returns the graph.
    ``last`` (a list) receives what the captured step returned: the tensors every
    replay writes, i.e. what a caller of the replayed frame reads."""
    for _ in range(2):
        step()
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        step()
        torch.cuda.synchronize()
        with torch.cuda.graph(graph):
            out = step()
    torch.cuda.current_stream().wait_stream(s)
    if last is not None:
        last[:] = [out]
    return graph


def keep_last(step, last):
    """``step`` as a callable that leaves its latest return value in ``last[0]``."""
    def run():
        last[:] = [step()]
    return run


DUMP_LIMIT_BYTES = 64 << 20


def named_arrays(out, prefix="out"):
    """Flatten nested tuples / lists / dicts of tensors into (name, tensor) pairs;
    the name is the path of indices and keys."""
    if torch.is_tensor(out):
        return [(prefix, out)]
    if isinstance(out, dict):
        return [p for k in out for p in named_arrays(out[k], f"{prefix}_{k}")]
    if isinstance(out, (list, tuple)):
        return [p for i, v in enumerate(out) for p in named_arrays(v, f"{prefix}_{i}")]
    return []


def dump_outputs(out, path, limit=DUMP_LIMIT_BYTES):
    """Write every tensor of ``out`` as ``path/<name>.npy``: float32 (float64 for
    fp64 and integer tensors), at most ``limit`` bytes in all.  An array over its
    equal share of the limit is cut to a fixed, seeded sample of its flattened
    elements (ascending positions), the same from run to run."""
    import numpy as np
    os.makedirs(path, exist_ok=True)
    arrays = []
    for name, t in named_arrays(out):
        t = t.detach()
        wide = t.dtype == torch.float64 or not (t.is_floating_point() or t.dtype == torch.bool)
        arrays.append((name, t.to(torch.float64 if wide else torch.float32).cpu().numpy()))
    if not arrays:
        raise RuntimeError("--dump-outputs: the timed step returned no tensor")
    share = limit // len(arrays)
    written = {}
    for name, a in arrays:
        if a.nbytes > share:
            keep = np.sort(np.random.default_rng(0).choice(a.size, size=share // a.itemsize, replace=False))
            a = a.reshape(-1)[keep]
        np.save(os.path.join(path, name + ".npy"), a)
        written[name] = list(a.shape)
    return written


def with_metas(head, metas, replay, graph=True):
    """One timed step: the host fp64 inverse of every camera matrix + its staging into the
    pinned buffers the captured graph's copy nodes read (cmt_head.py:428, 441-444, as the
    reference does per forward), then the replay.  The same frame's metas are staged every
    step, so a staging that overlaps the previous replay's copy writes identical values."""
    if not graph or not getattr(head, "_meta_plan", None):
        return replay

    def run():
        head.stage_metas(metas)
        replay()
    return run


def side_frames(name, steps, env, dev, graph=True):
    """GPU frames/s of another BASELINE config's forward on this run's line (no CPU leg):
    the workload's own policy, captured and replayed like the headline."""
    w = WORKLOADS[name]
    set_precision(w["precision"])
    head, _, step, nks, _ = make_workload(name, seed=dp.frame_seed(0, env), device=dev)
    with torch.no_grad():
        run = capture(step).replay if graph else step
        e, v = dp.timed_frames(with_metas(head, step.metas, run, graph), steps=steps, warmup=3, env=env,
                               sync=torch.cuda.synchronize, device=dev)
    return {"value": round(v, 3), "unit": "frames/s", "steps": steps, "ms_per_step": round(e / steps * 1e3, 4),
            "dtype": DTYPE_LABEL[w["precision"]], "seq_len": sum(nks), "num_query": w["nq"],
            "decoder_gflop_per_frame": round(sum(decoder_frame_flops(nq=w["nq"], nk=nk) for nk in nks) / 1e9, 2),
            "workload": w["desc"]}


def side_train(steps, warmup, env, dev):
    """configs[3]: the coop head's DDP training step (RCCL gradient all-reduce at world > 1)."""
    set_precision(WORKLOADS["coop"]["precision"])
    e, v, loss, nks, nparam = train_bench("coop", steps, warmup, env, dev)
    return {"value": round(v, 3), "unit": "steps/s (whole job, one frame per GPU per step)", "steps": steps,
            "warmup": warmup, "ms_per_step": round(e / steps * 1e3, 3), "last_loss": round(loss, 4),
            "dtype": "fp32 (bf16x3 GEMMs) + fp16 cross-attention core", "seq_len": sum(nks),
            "trainable_params": nparam,
            "workload": WORKLOADS["coop"]["desc"] + " -- TRAINING step: DN queries, Hungarian-matched focal/L1 "
                        "losses, native backward, bucketed RCCL gradient all-reduce, clip 35 + AdamW"}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--workload", default="fusion", choices=sorted(WORKLOADS),
                    help="fusion = BASELINE configs[2] (the headline line); lidar / coop / stress4 = configs[1] / "
                         "[3] forward / [4]")
    ap.add_argument("--precision", default=None, choices=["bf16", "fp16", "ref", "exact"],
                    help="compute policy of the headline value (default: the workload's: ref, fp16 for stress4)")
    ap.add_argument("--dump-outputs", metavar="DIR", default=None,
                    help="after the timed steps, write what the last one returned as DIR/<name>.npy")
    ap.add_argument("--full", action="store_true",
                    help="also measure everything beside the headline: roofline + PMC traffic of the dominant "
                         "kernel, recomputed / bf16 frames, voxel scatter-mean, the other configs, the CPU "
                         "baseline (each has its own --no-* switch below)")
    ap.add_argument("--no-graph", action="store_true")
    ap.add_argument("--no-recompute", action="store_true",
                    help="skip the side key timing the frame with the weight-only encodings recomputed")
    ap.add_argument("--batch", type=int, default=1,
                    help="frames per head forward (the headline is 1: one frame per GPU per step)")
    ap.add_argument("--no-ref", action="store_true", help="skip the bf16-policy frames/s side key")
    ap.add_argument("--cpu-seconds", type=float, default=25.0)
    ap.add_argument("--no-cpu-baseline", action="store_true")
    ap.add_argument("--no-traffic", action="store_true", help="profiling runs: do not read the committed PMC summary")
    ap.add_argument("--no-side", action="store_true",
                    help="skip the other configs' side keys (lidar, stress4 frames/s; coop training steps/s)")
    ap.add_argument("--side-steps", type=int, default=20)
    ap.add_argument("--train", action="store_true",
                    help="time the head TRAINING step instead (configs[3]: use --workload coop)")
    args = ap.parse_args()

    env = dp.dp_env()
    if args.gpus > 1 and env.world == 1 and "RANK" not in os.environ:
        sys.exit(spawn_ranks(args))
    if args.gpus != env.world:
        raise SystemExit(f"--gpus {args.gpus} but WORLD_SIZE={env.world}: launch one process per GPU")
    world, rank, local = env.world, env.rank, env.local_rank
    dev = torch.device("cuda", local)
    torch.cuda.set_device(dev)
    if world > 1:
        dp.init(env, backend="nccl", device=dev)
    native.lib()
    w = WORKLOADS[args.workload]
    prec = args.precision or w["precision"]
    set_precision(prec)
    last = [] if args.dump_outputs else None   # what the latest timed step returned
    if args.train:
        elapsed, value, loss, nks, nparam = train_bench(args.workload, args.steps, args.warmup, env, dev, last)
        if rank == 0:
            if last is not None:
                dump_outputs(last[0], args.dump_outputs)
            print(json.dumps({
                "metric": "head training steps/sec (DDP, one frame per GPU per step)", "value": round(value, 3),
                "unit": "steps/s", "n_gpus": world, "steps": args.steps, "warmup": args.warmup,
                "ms_per_step": round(elapsed / args.steps * 1e3, 3), "higher_is_better": True, "scaling": "weak",
                "vs_baseline": None, "dtype": "fp32 (+fp16 cross-attention core)",
                "data": "synthetic frames and 20 synthetic GT boxes per frame, random-init head weights",
                "config": {"workload": w["desc"] + " -- TRAINING step: DN queries, Hungarian-matched focal/L1 "
                           "losses, native backward, bucketed RCCL gradient all-reduce, clip 35 + AdamW",
                           "global_batch": world, "seq_len": sum(nks), "parallelism": f"dp{world}",
                           "trainable_params": nparam},
                "last_loss": round(loss, 4)}), flush=True)
        if world > 1:
            dist.barrier()
            dist.destroy_process_group()
        return

    head, cfg, step, nks, _ = make_workload(args.workload, seed=dp.frame_seed(0, env), device=dev, batch=args.batch)
    metas = step.metas

    with torch.no_grad():
        if not args.no_graph:
            run = capture(step, last).replay
        else:
            run = step if last is None else keep_last(step, last)
        elapsed, value = dp.timed_frames(with_metas(head, metas, run, not args.no_graph), steps=args.steps, warmup=args.warmup, env=env,
                                         sync=torch.cuda.synchronize, device=dev)
        value *= args.batch   # frames per forward
        if last is not None:
            if rank == 0:
                dump_outputs(last[0], args.dump_outputs)
            last.clear()

        # --- everything below is beside the headline and runs under --full only ---

        # --- dominant kernel: the cross-attention core as the timed frame runs it (its 8 split
        # partials stay in the workspace for chain B1, which combines them in its prologue, ABI 19),
        # HIP events on its launch stream; PMC traffic from the same form
        attn_ms = None
        if args.full:
            with region_timer() as rt:
                for _ in range(3):
                    step()
            attn_ms_all = rt.durations_ms("cross_attn")
            attn_ms = sum(attn_ms_all) / len(attn_ms_all)

        # --- the same frame with the weight-only encodings recomputed per frame (the reference
        # recomputes them on every forward, cmt_head.py:436, 489; the headline keeps them like weight
        # packs: WEIGHT_ONLY_KEPT)
        recompute = None
        if args.full and not args.no_recompute and OPTIONS.bev_pos_cache:
            with options(bev_pos_cache=False):
                run_r = capture(step).replay if not args.no_graph else step
                st_r = max(10, args.steps // 2)
                e_r, v_r = dp.timed_frames(with_metas(head, metas, run_r, not args.no_graph), steps=st_r, warmup=3, env=env,
                                           sync=torch.cuda.synchronize, device=dev)
            recompute = {"value": round(v_r * args.batch, 3), "unit": "frames/s", "steps": st_r,
                         "ms_per_step": round(e_r / st_r * 1e3, 4),
                         "recomputed_per_frame": WEIGHT_ONLY_KEPT}
            del run_r
            torch.cuda.empty_cache()

        # --- the bf16 speed policy on the same frame (bf16 operands everywhere; NOT held to
        # north_star's 1e-3 -- reported beside the headline, never as it)
        side = None
        if args.full and not args.no_ref and prec == "ref":
            set_precision("bf16")
            run_b = capture(step).replay if not args.no_graph else step
            st_b = max(10, args.steps // 2)
            e_b, v_b = dp.timed_frames(with_metas(head, metas, run_b, not args.no_graph), steps=st_b, warmup=3, env=env, sync=torch.cuda.synchronize, device=dev)
            side = {"value": round(v_b, 3), "unit": "frames/s", "steps": st_b, "ms_per_step": round(e_b / st_b * 1e3, 4),
                    "dtype": "bf16 GEMM and attention operands (fp32 accumulate): ~2.5 % of scale from the "
                             "reference, outside north_star's 1e-3"}
            del run_b
            set_precision(prec)

        # --- voxel scatter-mean of ~30k points (timed separately)
        vox_ms = None
        if args.full:
            vl = SPConvVoxelization(voxel_size=[0.075, 0.075, 0.2], point_cloud_range=[-54.0, -54.0, -5.0, 54.0, 54.0, 3.0],
                                    max_num_points=10, max_voxels=(120000, 160000), num_point_features=5).eval()
            pts = S.synthetic_points(30000, [-54.0, -54.0, -5.0, 54.0, 54.0, 3.0], seed=rank, device=dev)
            # three launches, voxel count kept on the device: captured as a graph like the frame
            vstep = lambda: vl.forward_padded(pts, 5)  # noqa: E731
            for _ in range(3):
                vstep()
            torch.cuda.synchronize()
            vrun = capture(vstep).replay if not args.no_graph else vstep
            nvox = 50
            tv = time.perf_counter()
            for _ in range(nvox):
                vrun()
            torch.cuda.synchronize()
            vox_ms = (time.perf_counter() - tv) / nvox * 1e3

    # --- every other BASELINE config's number on the same line (GPU only): configs[1] lidar and
    # configs[4] stress4 forward frames/s, configs[3] coop training steps/s (tools/benchmark.py:110-138
    # timing pattern: warm-up, synchronize, timed loop)
    sides = {}
    if args.full and not args.no_side and args.workload == "fusion" and args.batch == 1:
        del run
        torch.cuda.empty_cache()
        for key, fn in (("lidar", lambda: side_frames("lidar", args.side_steps, env, dev, not args.no_graph)),
                        ("stress4", lambda: side_frames("stress4", args.side_steps, env, dev, not args.no_graph)),
                        ("train_coop", lambda: side_train(args.side_steps, 5, env, dev))):
            sides[key] = fn()
            torch.cuda.empty_cache()
        set_precision(prec)

    ms_per_step = elapsed / args.steps * 1e3
    # mean algorithmic FLOPs of one cross-attention launch (agents may differ in Nk)
    nq = w["nq"]
    roofline = None
    if args.full:
        flop_launch = args.batch * sum(cross_attn_flops(nq=nq, nk=nk) for nk in nks) / len(nks)
        achieved = flop_launch / (attn_ms * 1e-3) / 1e12
        peak = PEAK_TFLOPS.get(prec, PEAK_TFLOPS["bf16"])
        traffic, traffic_src = (None, None)
        if not args.no_traffic:
            traffic, traffic_src = load_traffic(args.workload, sum(nks) // len(nks))
        roofline = {"kernel": "cmt_attn_fwd (cross-attention core attn_pb2_kernel; its split partials are "
                              "combined by the next kernel, chain B1, as in the timed frame)", "bound": "mfma",
                    "achieved": round(achieved, 2), "peak": peak, "unit": "TFLOP/s",
                    "frac": round(achieved / peak, 4), "traffic": traffic, "traffic_source": traffic_src,
                    "avg_launch_ms": round(attn_ms, 5), "flop_per_launch": flop_launch}
    result = {
        "metric": METRIC,
        "value": round(value, 3),
        "unit": "frames/s",
        "n_gpus": world,
        "steps": args.steps,
        "warmup": args.warmup,
        "ms_per_step": round(ms_per_step, 4),
        "higher_is_better": True,
        "scaling": "weak",
        "vs_baseline": None,
        "dtype": DTYPE_LABEL[prec],
        "data": "synthetic (seeded BEV features relu(N(0,1)), image feats N(0,1), nuScenes/TUMTraf-like camera "
                "matrices, random-init weights of the head)",
        "config": {"workload": w["desc"] + ("" if args.batch == 1 else f" -- {args.batch} frames per forward"),
                   "global_batch": world * args.batch, "seq_len": sum(nks), "num_query": nq,
                   "parallelism": f"dp{world}", "graph": not args.no_graph,
                   # functions of the weights (and the BEV grid) only: built once per weight version
                   # like the packed weights; the per-frame cost of recomputing them is the
                   # "weight_only_recomputed" side key
                   "weight_only_kept": WEIGHT_ONLY_KEPT if OPTIONS.bev_pos_cache else [],
                   "camera_metas_staged_per_step": bool(getattr(head, "_meta_plan", None)) and not args.no_graph,
                   "decoder_gflop_per_frame": round(sum(decoder_frame_flops(nq=nq, nk=nk) for nk in nks) / 1e9, 2)},
    }
    if args.full:
        result.update({
            "roofline": roofline,
            "bf16_policy": side,
            "weight_only_recomputed": recompute,
            "voxel_scatter_mean_ms": round(vox_ms, 4),
            **sides,
            "cpu_baseline": None,
        })
    if args.full and rank == 0 and world == 1 and not args.no_cpu_baseline:
        result["cpu_baseline"] = cpu_baseline(args.workload, args.cpu_seconds, seed=dp.frame_seed(0, env))
    if rank == 0:
        print(json.dumps(result), flush=True)
    if world > 1:
        dist.barrier()
        dist.destroy_process_group()


if __name__ == "__main__":
    main()
