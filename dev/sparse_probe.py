"""Per-layer timing of the native SparseEncoder on the full 41 x 1440 x 1440 grid.

A seeded LiDAR-like cloud (rings of a spinning sensor on a ground plane plus upright surfaces, ~120 k
voxels at 0.075 m x 0.075 m x 0.2 m) runs through the reference configuration's encoder.  Every
cmt_sparse_conv call of one forward is recorded and then timed alone with device events over --iters
launches after --warmup; the index / rulebook builds and the whole forward are timed the same way.
Printed per layer: kernel time, rows, active taps per 32-row wave tile after skipping (of K), and the
achieved gather rate (bytes of neighbour rows read, nbr >= 0 entries x Cin x 4, over kernel time).

    python dev/sparse_probe.py [--iters 50] [--warmup 10] [--seed 0] [--out FILE]

Needs a HIP device and the built library; there is no CPU path.
"""
import argparse
import math
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (os.path.join(ROOT, "cmt-cooperative-perception_amd"), ROOT):
    if p not in sys.path:
        sys.path.insert(0, p)

GRID = (41, 1440, 1440)
ENCODER = dict(type="SparseEncoder", in_channels=5, sparse_shape=list(GRID), output_channels=128,
               order=("conv", "norm", "act"), encoder_channels=((16, 16, 32), (32, 32, 64), (64, 64, 128), (128, 128)),
               encoder_paddings=((0, 0, 1), (0, 0, 1), (0, 0, [0, 1, 1]), (0, 0)), block_type="basicblock")


def lidar_voxels(seed, rings=64, azimuths=4700):
    """(features [N, 5], coors [N, 4]) of a synthetic spinning-LiDAR sweep, in first-appearance order"""
    g = torch.Generator().manual_seed(seed)
    elev = torch.linspace(math.radians(-25.0), math.radians(6.0), rings)
    az = torch.linspace(0.0, 2.0 * math.pi, azimuths + 1)[:-1]
    e, a = torch.meshgrid(elev, az, indexing="ij")
    height = 1.8
    ground = torch.where(e < -0.01, height / torch.tan(-e).clamp_min(1e-3), torch.full_like(e, 1e9))
    # upright surfaces: a seeded horizontal distance per 2-degree azimuth sector
    wall = 6.0 + 46.0 * torch.rand(180, generator=g)
    d = torch.minimum(ground, wall[(a / (2.0 * math.pi) * 180).long().clamp_max(179)])
    d = d * (1.0 + 0.002 * torch.randn(e.shape, generator=g))
    x, y, z = d * torch.cos(a), d * torch.sin(a), d * torch.tan(e)      # sensor at z = 0, ground at -height
    keep = (x.abs() < 54.0) & (y.abs() < 54.0) & (z > -5.0) & (z < 3.0)
    x, y, z = x[keep], y[keep], z[keep]
    c = torch.stack([torch.zeros_like(x), (z + 5.0) / 0.2, (y + 54.0) / 0.075, (x + 54.0) / 0.075], 1).floor().long()
    site = (c[:, 1] * GRID[1] + c[:, 2]) * GRID[2] + c[:, 3]
    _, first = torch.unique(site, return_inverse=True)
    order = torch.full((int(first.max()) + 1,), site.numel(), dtype=torch.long).scatter_reduce(
        0, first, torch.arange(site.numel()), reduce="amin")
    order, _ = torch.sort(order)                                  # voxels by their first point
    coors = c[order].to(torch.int32).contiguous()
    feats = torch.cat([x[order, None], y[order, None], z[order, None], torch.rand(order.numel(), 2, generator=g)], 1)
    return feats.float().contiguous(), coors


def timed(fn, iters, warmup):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    t0.record()
    for _ in range(iters):
        fn()
    t1.record()
    torch.cuda.synchronize()
    return t0.elapsed_time(t1) / iters * 1e-3     # seconds per call


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--capacity-factor", type=float, default=8.0)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("sparse_probe needs a HIP device (timings are never taken on the CPU)")
    from projects.mmdet3d_plugin import build_middle_encoder
    from projects.mmdet3d_plugin import native_sparse as S
    dev = torch.device("cuda:0")
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    torch.manual_seed(args.seed)
    enc = build_middle_encoder(dict(ENCODER, capacity_factor=args.capacity_factor)).eval().to(dev)
    feats, coors = lidar_voxels(args.seed)
    feats, coors = feats.to(dev), coors.to(dev)
    say(f"device {torch.cuda.get_device_name(0)}; seed {args.seed}; grid {GRID}; {coors.shape[0]} voxels; "
        f"{args.iters} timed launches after {args.warmup} warm-up, device events")

    calls, builds = [], []
    real = {n: getattr(S, n) for n in ("conv", "build_index", "rulebook_subm", "rulebook_down")}

    def rec_conv(X, nbr, count, Wp, scale, shift, **kw):
        calls.append((X, nbr, count, Wp, scale, shift, kw))
        return real["conv"](X, nbr, count, Wp, scale, shift, **kw)

    def rec_build(name):
        def f(*a, **kw):
            builds.append((name, a, kw))
            return real[name](*a, **kw)
        return f

    S.conv = rec_conv
    for n in ("build_index", "rulebook_subm", "rulebook_down"):
        setattr(S, n, rec_build(n))
    try:
        with torch.no_grad():
            out = enc(feats, coors, 1)
    finally:
        for n, f in real.items():
            setattr(S, n, f)
    torch.cuda.synchronize()
    say(f"output {tuple(out.shape)}, {int((out != 0).any(1).sum())} active BEV cells")

    say(f"{'layer':>5} {'Cin':>4} {'Cout':>4} {'K':>3} {'rows':>8} {'taps/tile':>9} {'time us':>9} {'gather GB/s':>11} {'GFLOP/s':>9}")
    total = 0.0
    for i, (X, nbr, count, Wp, scale, shift, kw) in enumerate(calls):
        n = int(count.item())
        K = nbr.shape[1]
        live = nbr[:n] >= 0
        pad = (-n) % 32
        tiles = torch.cat([live, live.new_zeros((pad, K))]).view(-1, 32, K).any(1)
        taps = tiles.sum().item() / tiles.shape[0]
        pairs = int(live.sum())
        t = timed(lambda: real["conv"](X, nbr, count, Wp, scale, shift, **kw), args.iters, args.warmup)
        total += t
        say(f"{i:>5} {kw['Cin']:>4} {kw['Cout']:>4} {K:>3} {n:>8} {taps:>9.2f} {t * 1e6:>9.1f} "
            f"{pairs * kw['Cin'] * 4 / t * 1e-9:>11.1f} {2.0 * pairs * kw['Cin'] * kw['Cout'] / t * 1e-9:>9.1f}")
    say(f"sum of the {len(calls)} convolution kernels: {total * 1e3:.3f} ms")
    tb = 0.0
    for name, a, kw in builds:
        t = timed(lambda: real[name](*a, **kw), args.iters, args.warmup)
        tb += t
        grid = a[2] if name == "build_index" else a[3]
        say(f"{name:>14} rows {a[0].shape[0]:>8} grid {tuple(grid)}: {t * 1e6:9.1f} us (with its buffer allocations)")
    say(f"sum of the {len(builds)} index / rulebook builds: {tb * 1e3:.3f} ms")

    def fwd():
        with torch.no_grad():
            enc(feats, coors, 1)
    t = timed(fwd, args.iters, args.warmup)
    say(f"whole forward (5 host reads of a row count included): {t * 1e3:.3f} ms")
    say(f"peak device memory {torch.cuda.max_memory_allocated() / 2 ** 20:.0f} MiB")
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
