"""Per-launch timing of the native CPFPN at the reference geometry: [6, 768, 40, 100] + [6, 1024, 20, 50] -> 256.

Every kernel launch of one forward (the two cmt_fpn_lateral, the 3 x 3 output conv on cmt_gemm, the two
cmt_rows_to_nchw) is recorded and then timed alone with device events: --repeats windows of --iters launches
after --warmup, reported as the median window with the min .. max spread.  Each launch stands beside two
yardsticks measured in the same session, in alternating windows:
  * the same step on torch's fp32 conv2d / interpolate / add, the chain users ran before (torch's outputs are
    already NCHW, so the layout launches have no torch counterpart and count fully against the native side);
  * for the laterals, the composition of the kernels the library had: cmt_nchw_to_rows + cmt_gemm on pair rows
    (which still leaves the top-down add and the NCHW output to torch).
Then the sums, the whole forward of both chains, and the full-size max error of native against the torch fp32
chain (a sanity figure, not a bound; the bound is tests/test_gpu_fpn.py's, against float64).

    python dev/img_neck_probe.py [--iters 20] [--warmup 5] [--repeats 5] [--seed 0] [--out FILE]

Needs a HIP device and the built library; there is no CPU path.
"""
import argparse
import os
import statistics
import sys

import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (os.path.join(ROOT, "cmt-cooperative-perception_amd"), ROOT):
    if p not in sys.path:
        sys.path.insert(0, p)

NECK = dict(type="CPFPN", in_channels=[768, 1024], out_channels=256, num_outs=2)
SHAPES = [(6, 768, 40, 100), (6, 1024, 20, 50)]


def window(fn, iters):
    t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    t0.record()
    for _ in range(iters):
        fn()
    t1.record()
    torch.cuda.synchronize()
    return t0.elapsed_time(t1) / iters * 1e-3     # seconds per call


def timed(fns, iters, warmup, repeats):
    """[(median, min, max)] per function; the functions' windows alternate, so drift hits them alike"""
    for fn in fns:
        for _ in range(warmup):
            fn()
    torch.cuda.synchronize()
    ts = [[] for _ in fns]
    for _ in range(repeats):
        for i, fn in enumerate(fns):
            ts[i].append(window(fn, iters))
    return [(statistics.median(t), min(t), max(t)) for t in ts]


def us(t):
    return f"{t[0] * 1e6:8.1f} ({t[1] * 1e6:.1f} .. {t[2] * 1e6:.1f})"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("img_neck_probe needs a HIP device (timings are never taken on the CPU)")
    from projects.mmdet3d_plugin import build_neck, native
    from projects.mmdet3d_plugin import native_bev as NB
    from projects.mmdet3d_plugin import native_fpn as NF
    dev = torch.device("cuda:0")
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    def T(*fns):
        return timed(fns, args.iters, args.warmup, args.repeats)

    neck = build_neck(NECK).eval()
    g = torch.Generator().manual_seed(args.seed)
    with torch.no_grad():
        for m in neck.modules():
            if isinstance(m, torch.nn.Conv2d):
                fan = m.in_channels * m.kernel_size[0] * m.kernel_size[1]
                m.weight.copy_(torch.randn(m.weight.shape, generator=g) / fan ** 0.5)
                m.bias.copy_(0.5 * torch.randn(m.bias.shape, generator=g))
    neck.to(dev)
    xs = [torch.randn(s, generator=g).to(dev) for s in SHAPES]
    say(f"device {torch.cuda.get_device_name(0)}; seed {args.seed}; inputs {SHAPES} -> 256; median of {args.repeats} "
        f"windows of {args.iters} launches after {args.warmup} warm-up (min .. max), device events")

    real = {"lateral": NF.lateral, "rows_to_nchw": NF.rows_to_nchw, "conv3x3_gemm": NB.conv3x3_gemm}
    calls = []

    def rec(name):
        def f(*a, **kw):
            y = real[name](*a, **kw)
            calls.append((name, a, dict(kw, out=y)))      # timed launches write the buffer of the recorded one
            return y
        return f

    NF.lateral, NF.rows_to_nchw, NB.conv3x3_gemm = rec("lateral"), rec("rows_to_nchw"), rec("conv3x3_gemm")
    try:
        with torch.no_grad():
            outs = neck(xs)
    finally:
        NF.lateral, NF.rows_to_nchw, NB.conv3x3_gemm = real["lateral"], real["rows_to_nchw"], real["conv3x3_gemm"]
    torch.cuda.synchronize()
    neck.check_input_range()
    assert [c[0] for c in calls] == ["lateral", "lateral", "conv3x3_gemm", "rows_to_nchw", "rows_to_nchw"]

    # the torch fp32 chain
    w1, b1 = neck.lateral_convs[1].conv.weight.detach(), neck.lateral_convs[1].conv.bias.detach()
    w0, b0 = neck.lateral_convs[0].conv.weight.detach(), neck.lateral_convs[0].conv.bias.detach()
    wf, bf = neck.fpn_convs[0].conv.weight.detach(), neck.fpn_convs[0].conv.bias.detach()
    with torch.no_grad():
        t_l1 = F.conv2d(xs[1], w1, b1)
        t_l0 = F.conv2d(xs[0], w0, b0) + F.interpolate(t_l1, size=xs[0].shape[2:], mode="nearest")
        t_o0 = F.conv2d(t_l0, wf, bf, 1, 1)
    torch.cuda.synchronize()
    for name, o, r in (("outs[0]", outs[0], t_o0), ("outs[1]", outs[1], t_l1)):
        d, top = (o - r).abs().max().item(), r.abs().max().item()
        say(f"{name} {tuple(o.shape)}: native against the torch fp32 chain: max abs difference {d:.3e} over max abs "
            f"{top:.3f} = {d / top:.2e} (sanity figure, both sides carry rounding)")

    # the composition the library had for a lateral: nchw_to_rows, then cmt_gemm on pair rows
    def composed(x, wp, shift, y):
        rows = NB.to_rows(x).rows
        M, K = rows.shape[0], rows.shape[2]
        native.gemm(rows, wp, y, M=M, N=256, K=K, lda=K, ldw=K, ldc=256, bias=shift)
        return y

    steps = [
        ("lateral 1", 0, lambda: F.conv2d(xs[1], w1, b1), 1, 2.0 * 6 * 1000 * 1024 * 256),
        ("lateral 0 + top-down", 1,
         lambda: F.conv2d(xs[0], w0, b0) + F.interpolate(t_l1, size=xs[0].shape[2:], mode="nearest"), 0,
         2.0 * 6 * 4000 * 768 * 256),
        ("output conv 3x3", 2, lambda: F.conv2d(t_l0, wf, bf, 1, 1), None, 2.0 * 6 * 4000 * 9 * 256 * 256),
        ("rows -> NCHW, level 0", 3, None, None, 0.0),
        ("rows -> NCHW, level 1", 4, None, None, 0.0),
    ]
    say(f"{'launch':>22} {'kernel':>14} {'GFLOP':>6} {'native us (min .. max)':>30} {'TFLOP/s':>8} "
        f"{'torch fp32 us (min .. max)':>30} {'native/torch':>12} {'nchw_to_rows + cmt_gemm us':>30} {'native/composed':>15}")
    tot_n = tot_t = tot_lat_n = tot_lat_c = 0.0
    notes = []
    with torch.no_grad():
        for label, ci, tfn, level, flop in steps:
            name, a, kw = calls[ci]
            fns = [lambda: real[name](*a, **kw)]
            if tfn is not None:
                fns.append(tfn)
            if level is not None:
                wp, shift = neck.packed("lateral", level)
                y = torch.empty_like(kw["out"])
                check = composed(xs[level], wp, shift, y)
                if level == 1:       # no top-down term: the composition computes the same map
                    v, c = kw["out"].view(torch.float16).float(), check.view(torch.float16).float()
                    d = ((v[:, 0] + v[:, 1]) - (c[:, 0] + c[:, 1])).abs().max().item()
                    say(f"lateral 1: cmt_fpn_lateral against nchw_to_rows + cmt_gemm: max abs difference {d:.3e}")
                fns.append(lambda x=xs[level], wp=wp, shift=shift, y=y: composed(x, wp, shift, y))
            res = T(*fns)
            tn = res[0]
            tt = res[1] if tfn is not None else None
            tc = res[-1] if level is not None else None
            tot_n += tn[0]
            tot_t += tt[0] if tt else 0.0
            if tc:
                tot_lat_n += tn[0]
                tot_lat_c += tc[0]
            rate = f"{flop / tn[0] * 1e-12:8.1f}" if flop else f"{'-':>8}"
            say(f"{label:>22} {name:>14} {flop * 1e-9:>6.1f} {us(tn):>30} {rate} "
                f"{us(tt) if tt else '-':>30} {f'{tn[0] / tt[0]:.2f}' if tt else '-':>12} "
                f"{us(tc) if tc else '-':>30} {f'{tn[0] / tc[0]:.2f}' if tc else '-':>15}")
            if tt and tn[0] > tt[0]:
                notes.append(f"{label} ({tn[0] / tt[0]:.2f} x torch)")
            if tc and tn[0] > tc[0]:
                notes.append(f"{label} ({tn[0] / tc[0]:.2f} x nchw_to_rows + cmt_gemm)")
    say(f"sum of the 5 native launches {tot_n * 1e6:.1f} us; the 3 torch steps {tot_t * 1e6:.1f} us; the two laterals "
        f"{tot_lat_n * 1e6:.1f} us native, {tot_lat_c * 1e6:.1f} us as nchw_to_rows + cmt_gemm (without the top-down add)")
    say("launches slower than a yardstick: " + (", ".join(notes) if notes else "none"))
    # what the epilogue's top-down term costs: the level-0 launch with and without T, alternating
    name, a, kw = calls[1]
    plain = dict(kw, top=None, top_hw=None, out=torch.empty_like(kw["out"]))
    with torch.no_grad():
        tw, tp = T(lambda: real[name](*a, **kw), lambda: real[name](*a, **plain))
    say(f"lateral 0 with the top-down term {us(tw)} us, without it {us(tp)} us")
    nbytes = [(1024 * 4 + 256 * 4) * 6000, (768 * 4 + 256 * 4) * 24000 + 256 * 4 * 6000, None, 256 * 8 * 24000, 256 * 8 * 6000]
    say("bytes each launch must move at least (inputs once, outputs once): " +
        ", ".join(f"{s[0]} {b * 1e-6:.1f} MB" for s, b in zip(steps, nbytes) if b))

    def fwd():
        with torch.no_grad():
            neck(xs)

    def fwd_torch():
        with torch.no_grad():
            l1 = F.conv2d(xs[1], w1, b1)
            l0 = F.conv2d(xs[0], w0, b0) + F.interpolate(l1, size=xs[0].shape[2:], mode="nearest")
            F.conv2d(l0, wf, bf, 1, 1)

    tn, tt = T(fwd, fwd_torch)
    say(f"whole forward (launches and allocations included): native {us(tn)} us, torch fp32 {us(tt)} us, "
        f"native/torch {tn[0] / tt[0]:.2f}")
    say(f"peak device memory {torch.cuda.max_memory_allocated() / 2 ** 20:.0f} MiB")
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
