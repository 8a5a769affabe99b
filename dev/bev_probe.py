"""Per-layer timing of the native SECOND + SECONDFPN at the reference geometry, [1, 256, 180, 180].

Every kernel launch of one forward (the NCHW halo conv, the pair-row convs on cmt_gemm, cmt_bev_conv3x3,
cmt_bev_deblock) is recorded and then timed alone with device events: --repeats windows of --iters launches
after --warmup, reported as the median window with the min .. max spread.  Printed per layer: time, useful
TFLOP/s (2 x output pixels x Cout x K over time), and the same layer on torch's own fp32 conv2d /
conv_transpose2d with BN folded -- what this chain ran on before, the yardstick for time.  Then the chain
totals (sum of kernels and the whole forward), the stride-1 pair-row layers on cmt_bev_conv3x3 against
cmt_gemm (alternating windows; the routing decision of DESIGN), the full-size max error of native against
the torch fp32 chain (a sanity figure, not a bound), and one shared_conv launch (512 -> 256 at 180 x 180)
for the rate comparison.

    python dev/bev_probe.py [--iters 20] [--warmup 5] [--repeats 5] [--seed 0] [--out FILE]

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

BN = dict(type="BN", eps=1e-3, momentum=0.01)
BACKBONE = dict(type="SECOND", in_channels=256, out_channels=[128, 256], layer_nums=[5, 5], layer_strides=[1, 2],
                norm_cfg=BN, conv_cfg=dict(type="Conv2d", bias=False))
NECK = dict(type="SECONDFPN", in_channels=[128, 256], out_channels=[256, 256], upsample_strides=[1, 2], norm_cfg=BN,
            upsample_cfg=dict(type="deconv", bias=False), use_conv_for_no_stride=True)
SHAPE = (1, 256, 180, 180)


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


def seed_modules(mods, seed):
    g = torch.Generator().manual_seed(seed)
    with torch.no_grad():
        for mod in mods:
            for m in mod.modules():
                if isinstance(m, (torch.nn.Conv2d, torch.nn.ConvTranspose2d)):
                    fan = m.in_channels * (9 if m.kernel_size == (3, 3) else 1)
                    m.weight.copy_(torch.randn(m.weight.shape, generator=g) / fan ** 0.5)
                elif isinstance(m, torch.nn.BatchNorm2d):
                    m.weight.copy_(0.5 + torch.rand(m.num_features, generator=g))
                    m.bias.copy_(0.5 * torch.randn(m.num_features, generator=g))
                    m.running_mean.copy_(0.5 * torch.randn(m.num_features, generator=g))
                    m.running_var.copy_(0.5 + 1.5 * torch.rand(m.num_features, generator=g))


def torch_layers(backbone, neck):
    """the chain on torch's fp32 ops with BN folded: [(name, fn(x) -> y)] and which outputs feed the neck"""
    from projects.mmdet3d_plugin import native_bev as NB
    layers = []
    for i, blk in enumerate(backbone.blocks):
        for j in range(0, len(blk), 3):
            conv, bn = blk[j], blk[j + 1]
            scale, shift = NB.fold_bn(bn.weight, bn.bias, bn.running_mean, bn.running_var, bn.eps)
            w = (conv.weight.detach().double() * scale[:, None, None, None]).float().contiguous()
            b, s = shift.float().contiguous(), conv.stride[0]
            layers.append((f"blocks.{i}.{j}", lambda x, w=w, b=b, s=s: F.relu(F.conv2d(x, w, b, s, 1))))
    ups = []
    for i, blk in enumerate(neck.deblocks):
        up, bn = blk[0], blk[1]
        scale, shift = NB.fold_bn(bn.weight, bn.bias, bn.running_mean, bn.running_var, bn.eps)
        b, k = shift.float().contiguous(), neck.upsample_strides[i]
        if isinstance(up, torch.nn.ConvTranspose2d):
            w = (up.weight.detach().double() * scale[None, :, None, None]).float().contiguous()
            ups.append((f"deblocks.{i}", lambda x, w=w, b=b, k=k: F.relu(F.conv_transpose2d(x, w, b, k))))
        else:
            w = (up.weight.detach().double() * scale[:, None, None, None]).float().contiguous()
            ups.append((f"deblocks.{i}", lambda x, w=w, b=b: F.relu(F.conv2d(x, w, b))))
    return layers, ups


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bev_probe needs a HIP device (timings are never taken on the CPU)")
    from projects.mmdet3d_plugin import build_backbone, build_neck, native
    from projects.mmdet3d_plugin import native_bev as NB
    dev = torch.device("cuda:0")
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    def T(*fns):
        return timed(fns, args.iters, args.warmup, args.repeats)

    backbone, neck = build_backbone(BACKBONE).eval(), build_neck(NECK).eval()
    seed_modules((backbone, neck), args.seed)
    backbone.to(dev), neck.to(dev)
    x = torch.randn(SHAPE, generator=torch.Generator().manual_seed(args.seed + 1)).to(dev)
    say(f"device {torch.cuda.get_device_name(0)}; seed {args.seed}; input {SHAPE}; median of {args.repeats} windows of "
        f"{args.iters} launches after {args.warmup} warm-up (min .. max), device events")

    names = ("conv3x3", "conv3x3_gemm", "conv3x3_nchw_gemm", "deblock")
    real = {n: getattr(NB, n) for n in names}
    calls = []

    def rec(name):
        def f(*a, **kw):
            y = real[name](*a, **kw)
            kw = dict(kw)
            if name != "deblock":
                kw["out"] = y       # timed launches write the buffer of the recorded one
            calls.append((name, a, kw))
            return y
        return f

    for n in names:
        setattr(NB, n, rec(n))
    try:
        with torch.no_grad():
            out = neck(backbone(x))[0]
    finally:
        for n, f in real.items():
            setattr(NB, n, f)
    torch.cuda.synchronize()
    backbone.check_input_range(), neck.check_input_range()

    tl, tu = torch_layers(backbone, neck)
    with torch.no_grad():
        acts, h, stage_in = [], x, []
        for (name, fn), nxt in zip(tl, tl[1:] + [None]):
            acts.append(h)
            h = fn(h)
            if nxt is None or nxt[0].endswith(".0"):
                stage_in.append(h)
        ref = torch.cat([fn(s) for (_, fn), s in zip(tu, stage_in)], 1)
    torch.cuda.synchronize()
    top = ref.abs().max().item()
    say(f"output {tuple(out.shape)}; native against the torch fp32 chain: max abs difference {(out - ref).abs().max().item():.3e} "
        f"over max abs {top:.3f} = {(out - ref).abs().max().item() / top:.2e} (sanity figure, both sides carry rounding)")

    say(f"{'layer':>12} {'kernel':>18} {'Cin':>4} {'Cout':>4} {'out px':>7} {'GFLOP':>6} {'native us (min .. max)':>30} "
        f"{'TFLOP/s':>8} {'torch fp32 us (min .. max)':>30} {'native/torch':>12}")
    tnames = [n for n, _ in tl] + [n for n, _ in tu]
    tfns = [(fn, a) for (_, fn), a in zip(tl, acts)] + [(fn, s) for (_, fn), s in zip(tu, stage_in)]
    assert len(calls) == len(tfns), (len(calls), len(tfns))
    tot_n = tot_t = 0.0
    losers = []
    with torch.no_grad():
        for (name, a, kw), lname, (tfn, tin) in zip(calls, tnames, tfns):
            if name == "conv3x3_nchw_gemm":
                cin, cout, px = a[0].shape[1], kw["Cout"], a[0].shape[2] * a[0].shape[3]
                kk = 9
            elif name == "deblock":
                cin, cout, px, kk = kw["Cin"], kw["Cout"], kw["H"] * kw["W"], kw["k"] ** 2
            else:
                ho, wo = NB.out_hw(kw["H"], kw["W"], kw.get("stride", 1))
                cin, cout, px, kk = kw["Cin"], kw["Cout"], ho * wo, 9
            flop = 2.0 * px * cout * kk * cin
            tn, tt = T(lambda: real[name](*a, **kw), lambda: tfn(tin))
            tot_n += tn[0]
            tot_t += tt[0]
            if tn[0] > tt[0]:
                losers.append(f"{lname} ({tn[0] / tt[0]:.2f} x torch)")
            say(f"{lname:>12} {name:>18} {cin:>4} {cout:>4} {px:>7} {flop * 1e-9:>6.1f} {us(tn):>30} "
                f"{flop / tn[0] * 1e-12:>8.1f} {us(tt):>30} {tn[0] / tt[0]:>12.2f}")
    say(f"sum of the {len(calls)} kernels: native {tot_n * 1e3:.3f} ms, torch fp32 {tot_t * 1e3:.3f} ms")
    say("layers slower than torch fp32: " + (", ".join(losers) if losers else "none"))

    def fwd():
        with torch.no_grad():
            neck(backbone(x))

    def fwd_torch():
        with torch.no_grad():
            h, feats = x, []
            for (name, fn), nxt in zip(tl, tl[1:] + [None]):
                h = fn(h)
                if nxt is None or nxt[0].endswith(".0"):
                    feats.append(h)
            torch.cat([fn(s) for (_, fn), s in zip(tu, feats)], 1)

    tn, tt = T(fwd, fwd_torch)
    say(f"whole forward (launches, allocations and the torch.cat of the torch chain included): native {us(tn)} us, "
        f"torch fp32 {us(tt)} us")

    say("stride-1 pair-row layers, cmt_gemm CONV3X3 against cmt_bev_conv3x3 (alternating windows):")
    seen = set()
    for name, a, kw in calls:
        if name != "conv3x3_gemm" or (kw["Cin"], kw["H"]) in seen:
            continue
        seen.add((kw["Cin"], kw["H"]))
        tg, tb = T(lambda: real["conv3x3_gemm"](*a, **kw), lambda: real["conv3x3"](*a, stride=1, **kw))
        say(f"  {kw['Cin']} -> {kw['Cout']} at {kw['H']} x {kw['W']}: cmt_gemm {us(tg)} us, cmt_bev_conv3x3 {us(tb)} us")

    # one shared_conv launch as the head runs it: 512 -> 256 at 180 x 180, fp32 rows out
    g = torch.Generator().manual_seed(args.seed + 2)
    xs = torch.randn(1, 512, 180, 180, generator=g).to(dev)
    ws = NB.split_pair((torch.randn(256, 9 * 512, generator=g) / (9 * 512) ** 0.5).double()).to(dev)
    bs = torch.randn(256, generator=g).to(dev)
    cs = torch.empty(180 * 180, 256, device=dev)

    def shared():
        native.gemm(xs, ws, cs, M=180 * 180, N=256, K=9 * 512, lda=180 * 180, ldw=9 * 512, ldc=256, bias=bs, relu=True,
                    a_mode=native.A_CONV3X3_NCHW, conv=(180, 180, 512), batch=1, a_bstride=512 * 180 * 180,
                    c_bstride=180 * 180 * 256)
    ts, = T(shared)
    fl = 2.0 * 180 * 180 * 256 * 9 * 512
    say(f"shared_conv (CMT_A_CONV3X3_NCHW 512 -> 256 at 180 x 180, {fl * 1e-9:.1f} GFLOP): {us(ts)} us, "
        f"{fl / ts[0] * 1e-12:.1f} TFLOP/s")
    say(f"peak device memory {torch.cuda.max_memory_allocated() / 2 ** 20:.0f} MiB")
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
