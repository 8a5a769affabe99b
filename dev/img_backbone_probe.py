"""Timing of the native VoVNet (V-99-eSE) at the reference geometry: [6, 3, 640, 1600] -> stage4 [6, 768, 40, 100]
and stage5 [6, 1024, 20, 50], what the CPFPN configs read.

Steps (``--step``; run each under its own time limit, e.g. ``timeout -k 10 600 python dev/img_backbone_probe.py
--step forward``):
  kinds     one forward with a device-event pair around every launch, --repeats times after warm-up: the median
            time per kernel kind and per stage, and per distinct 3 x 3 layer shape with its rate (2 * MACs / time,
            the three MFMA passes count once)
  layers    every distinct 3 x 3 layer shape alone: cmt_img_conv3x3 against torch's fp32 conv2d on the same
            operands (NCHW, BN folded into weight and bias, ReLU), alternating windows; the kernel at every
            number of column blocks per workgroup beside the library's own choice; and, for the stride-1 layers
            it takes (Cin, Cout % 64 == 0), cmt_gemm's CMT_A_CONV3X3 pair-row path on the same rows and pack
  forward   the whole forward against the same chain on torch's fp32 conv2d / max_pool2d(ceil_mode=True) / mean /
            hardtanh with BN folded, same device, same session, alternating windows, median and min .. max; then
            the relative difference of the two at this size (a sanity figure, not a bound: the bound is
            tests/test_gpu_vov.py's, against float64)
MIOpen picks its algorithms on first use, so every torch step is warmed before it is timed.

``--precision`` (default ``ref``): the backbone's arithmetic (native_img.set_img_precision).  ``fp16`` runs ``kinds``
under the one-pass policy; ``both`` makes ``forward`` alternate windows of 'ref', 'fp16' and torch in one session, and
``layers`` time cmt_img_conv3x3_f16 (the library's nb and every divisor) beside the three-pass kernel on the same
values rounded to fp16.

    python dev/img_backbone_probe.py --step forward [--precision both] [--iters 2] [--warmup 2] [--repeats 5]
                                     [--seed 0] [--out FILE]

``--out`` appends.  Needs a HIP device and the built library; there is no CPU path.
"""
import argparse
import os
import statistics
import sys
import zlib
from collections import OrderedDict

import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (os.path.join(ROOT, "cmt-cooperative-perception_amd"), ROOT):
    if p not in sys.path:
        sys.path.insert(0, p)

CFG = dict(type="VoVNet", spec_name="V-99-eSE", out_features=("stage4", "stage5"))
SHAPE = (6, 3, 640, 1600)


def seed(mod, seed):
    """every state-dict tensor by key: conv / fc weights N(0, 1) / sqrt(fan_in), BN gamma in [0.5, 1.5], beta and
    mean N(0, 0.25), var in [0.5, 2], fc.bias N(0, 1)"""
    sd = mod.state_dict()
    with torch.no_grad():
        for key, t in sd.items():
            g = torch.Generator().manual_seed(seed * 1_000_003 + zlib.crc32(key.encode()))
            if key.endswith("conv.weight") or key.endswith("fc.weight"):
                t.copy_(torch.randn(t.shape, generator=g) / (t.shape[1] * t.shape[2] * t.shape[3]) ** 0.5)
            elif key.endswith("norm.weight"):
                t.copy_(0.5 + torch.rand(t.shape, generator=g))
            elif key.endswith("norm.bias") or key.endswith("running_mean"):
                t.copy_(0.5 * torch.randn(t.shape, generator=g))
            elif key.endswith("running_var"):
                t.copy_(0.5 + 1.5 * torch.rand(t.shape, generator=g))
            elif key.endswith("fc.bias"):
                t.copy_(torch.randn(t.shape, generator=g))
    return mod


def folded(seq):
    """conv -> BN of a Sequential as (fp32 weight, fp32 bias), folded in float64"""
    conv, bn = seq[0], seq[1]
    scale = bn.weight.double() / torch.sqrt(bn.running_var.double() + bn.eps)
    return ((conv.weight.double() * scale[:, None, None, None]).float().contiguous(),
            (bn.bias.double() - bn.running_mean.double() * scale).float().contiguous())


class TorchChain:
    """the same network on torch's fp32 ops, BN folded"""

    def __init__(self, m):
        with torch.no_grad():
            self.stem = [folded(m.stem[3 * i:3 * i + 2]) + (s,) for i, s in enumerate((2, 1, 2))]
            self.stages = []
            for name in m.stage_names:
                blocks = []
                for _, blk in getattr(m, name).named_children():
                    if not hasattr(blk, "layers"):
                        blocks.append(None)
                        continue
                    blocks.append(dict(layers=[folded(seq) for seq in blk.layers], concat=folded(blk.concat),
                                       fc=(blk.ese.fc.weight.detach(), blk.ese.fc.bias.detach()), identity=blk.identity))
                self.stages.append((name, blocks))
        self.out_features = m._out_features

    def __call__(self, x):
        outs = OrderedDict()
        with torch.no_grad():
            for w, b, s in self.stem:
                x = F.relu(F.conv2d(x, w, b, s, 1))
            for name, blocks in self.stages:
                for blk in blocks:
                    if blk is None:
                        x = F.max_pool2d(x, 3, 2, ceil_mode=True)
                        continue
                    feats, cur = [x], x
                    for w, b in blk["layers"]:
                        cur = F.relu(F.conv2d(cur, w, b, 1, 1))
                        feats.append(cur)
                    y = F.relu(F.conv2d(torch.cat(feats, 1), *blk["concat"]))
                    y = y * (F.hardtanh(F.conv2d(y.mean((2, 3), keepdim=True), *blk["fc"]) + 3.0, 0.0, 6.0) / 6.0)
                    x = y + x if blk["identity"] else y
                if name in self.out_features:
                    outs[name] = x
        return outs


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


def ms(t):
    return f"{t[0] * 1e3:8.3f} ({t[1] * 1e3:.3f} .. {t[2] * 1e3:.3f})"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--step", choices=("kinds", "layers", "forward"), required=True)
    ap.add_argument("--precision", choices=("ref", "fp16", "both"), default="ref")
    ap.add_argument("--iters", type=int, default=2)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("img_backbone_probe needs a HIP device (timings are never taken on the CPU)")
    if args.repeats < 5:
        raise SystemExit("at least 5 windows")
    from projects.mmdet3d_plugin import build_backbone, native
    from projects.mmdet3d_plugin import native_bev as NB
    from projects.mmdet3d_plugin import native_fpn as NF
    from projects.mmdet3d_plugin import native_img as NI
    dev = torch.device("cuda:0")
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    m = seed(build_backbone(CFG), args.seed).eval().to(dev)
    x = torch.randn(SHAPE, generator=torch.Generator().manual_seed(args.seed + 1)).to(dev)
    if args.step == "kinds" and args.precision == "both":
        raise SystemExit("--step kinds takes one arithmetic per run: --precision ref or fp16")
    say(f"[{args.step}, precision {args.precision}] device {torch.cuda.get_device_name(0)}; V-99-eSE, seed {args.seed}; input {SHAPE}; median of "
        f"{args.repeats} windows of {args.iters} after {args.warmup} warm-up (min .. max), device events")

    if args.step == "kinds":
        f16 = args.precision == "fp16"
        NI.set_img_precision(args.precision)
        names = dict(stem_f16=NI, conv3x3_f16=NI, concat1x1_f16=NI, ese_gate=NI, ese_apply_f16=NI, maxpool_f16=NI,
                     rows_to_nchw_f16=NF) if f16 else \
            dict(stem=NI, conv3x3=NI, conv3x3_gemm=NI, concat1x1=NI, ese_gate=NI, ese_apply=NI, maxpool=NI, rows_to_nchw=NF)
        osa_name = "_osa"
        real = {k: getattr(mod, k) for k, mod in names.items()}
        events, stage = [], ["stem"]

        def rec(kind):
            def f(*a, **kw):
                t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                t0.record()
                y = real[kind](*a, **kw)
                t1.record()
                shape = (kw["Cin"], kw["Cout"], kw.get("stride", 1), kw["B"], kw["H"], kw["W"]) \
                    if kind in ("conv3x3", "conv3x3_gemm", "conv3x3_f16") else None
                events.append((kind, stage[0], shape, t0, t1))
                return y
            return f

        real_osa = getattr(m, osa_name)

        def osa(name, *a, **kw):
            stage[0] = "stage" + name[3]
            return real_osa(name, *a, **kw)

        setattr(m, osa_name, osa)
        for k, mod in names.items():
            setattr(mod, k, rec(k))
        runs = []
        try:
            for i in range(args.warmup + args.repeats):
                events.clear()
                stage[0] = "stem"
                m(x)
                torch.cuda.synchronize()
                if i >= args.warmup:
                    runs.append([(k, s, sh, t0.elapsed_time(t1) * 1e-3) for k, s, sh, t0, t1 in events])
        finally:
            for k, mod in names.items():
                setattr(mod, k, real[k])
            setattr(m, osa_name, real_osa)
        m.check_input_range()

        def med(select):
            tot = [sum(t for k, s, sh, t in run if select(k, s, sh)) for run in runs]
            return statistics.median(tot), min(tot), max(tot)

        say(f"{len(runs[0])} launches per forward; sum of the per-launch times {ms(med(lambda *a: True))} ms")
        for kind in names:
            n = sum(1 for k, *_ in runs[0] if k == kind)
            say(f"  kind {kind:>13} x{n:<4} {ms(med(lambda k, s, sh, kind=kind: k == kind))} ms")
        for st in ("stem", "stage2", "stage3", "stage4", "stage5"):
            say(f"  {st:>18}      {ms(med(lambda k, s, sh, st=st: s == st))} ms   (the pool and the output copy count "
                "to the stage before them)")
        shapes = OrderedDict()
        for k, s, sh, t in runs[0]:
            if sh is not None:
                shapes[sh] = shapes.get(sh, 0) + 1
        say(f"  {'3 x 3 layer (Cin, Cout, stride, B, H, W)':>44} {'count':>5} {'ms each (min .. max)':>28} {'GFLOP':>7} {'TFLOP/s':>8}")
        for sh, n in shapes.items():
            t = med(lambda k, s, q, sh=sh: q == sh)
            cin, cout, stride, b, h, w = sh
            ho, wo = NB.out_hw(h, w, stride)
            flop = 2.0 * b * ho * wo * 9 * cin * cout
            each = tuple(v / n for v in t)
            say(f"  {str(sh):>44} {n:>5} {ms(each):>28} {flop * 1e-9:7.1f} {flop / each[0] * 1e-12:8.1f}")

    elif args.step == "layers":
        say(f"  {'3 x 3 layer (Cin, Cout, stride, H, W)':>40} {'GFLOP':>7} {'native ms (min .. max)':>28} {'TFLOP/s':>8} "
            f"{'torch fp32 ms (min .. max)':>28} {'TFLOP/s':>8} {'native/torch':>12}")
        B = SHAPE[0]
        layers = [(64, 64, 1, 320, 800), (64, 128, 2, 320, 800), (128, 128, 1, 160, 400), (256, 160, 1, 80, 200),
                  (160, 160, 1, 80, 200), (512, 160, 1, 80, 200), (512, 192, 1, 40, 100), (192, 192, 1, 40, 100),
                  (768, 192, 1, 40, 100), (768, 224, 1, 20, 50), (224, 224, 1, 20, 50), (1024, 224, 1, 20, 50)]
        g = torch.Generator().manual_seed(args.seed + 2)
        for cin, cout, stride, H, W in layers:
            xs = torch.randn(B, cin, H, W, generator=g).to(dev)
            w = (torch.randn(cout, cin, 3, 3, generator=g) / (9 * cin) ** 0.5).to(dev)
            bias = torch.randn(cout, generator=g).to(dev)
            one = torch.ones(cout, dtype=torch.float64, device=dev)
            wp, shift = NB.pack_conv3x3(w, [one, bias.double(), torch.zeros_like(one), one, 0.0])
            rows = NB.to_rows(xs).rows
            ho, wo = NB.out_hw(H, W, stride)
            out = torch.empty((B * ho * wo, 2, cout), dtype=torch.uint16, device=dev)
            def run(nb=0):
                return NI.conv3x3(rows, wp, shift, B=B, H=H, W=W, Cin=cin, Cout=cout, stride=stride, out=out, nb=nb)

            def run_gemm():
                M = B * H * W
                return native.gemm(rows, wp, out_g, M=M, N=cout, K=9 * cin, lda=cin, ldw=9 * cin, ldc=cout, bias=shift,
                                   relu=True, a_mode=native.A_CONV3X3, conv=(H, W, cin))

            # the library's own choice of column blocks per workgroup (nb = 0) beside every divisor of Cout / 32
            divs = [d for d in range(1, cout // 32 + 1) if (cout // 32) % d == 0]
            if args.precision != "ref":
                # the one-pass kernel on the same values rounded to fp16, in the same alternating windows as the
                # three-pass kernel
                one = torch.ones(cout, dtype=torch.float64, device=dev)
                w16, shift16 = NI.pack_conv3x3_f16(w, [one, bias.double(), torch.zeros_like(one), one, 0.0])
                rows16 = xs.permute(0, 2, 3, 1).reshape(-1, cin).half().contiguous()
                out16 = torch.empty((B * ho * wo, cout), dtype=torch.float16, device=dev)

                def run16(nb=0):
                    return NI.conv3x3_f16(rows16, w16, shift16, B=B, H=H, W=W, Cin=cin, Cout=cout, stride=stride,
                                          out=out16, nb=nb)

                with torch.no_grad():
                    res = timed([run, run16] + [lambda d=d: run16(d) for d in divs], args.iters, args.warmup, args.repeats)
                    ref = F.relu(F.conv2d(xs, w, bias, stride, 1))
                d16 = (NF.rows_to_nchw_f16(out16, (B, cout, ho, wo)) - ref).abs().max().item() / ref.abs().max().item()
                flop = 2.0 * B * ho * wo * 9 * cin * cout
                say(f"  {str((cin, cout, stride, H, W)):>40} {flop * 1e-9:7.1f} three-pass {ms(res[0])} ms {flop / res[0][0] * 1e-12:6.1f} "
                    f"TFLOP/s | one-pass {ms(res[1])} ms {flop / res[1][0] * 1e-12:6.1f} TFLOP/s | one/three "
                    f"{res[1][0] / res[0][0]:.2f} (rel. difference to torch fp32 {d16:.1e}; one-pass by nb: " +
                    ", ".join(f"{q} {t[0] * 1e3:.3f}" for q, t in zip(divs, res[2:])) + ")")
                del xs, rows, out, ref, rows16, out16
                continue
            # cmt_gemm's CMT_A_CONV3X3 pair-row path takes the stride-1 layers with Cout % 64 == 0
            gemm_ok = stride == 1 and cout % 64 == 0 and cin % 64 == 0
            out_g = torch.empty_like(out) if gemm_ok else None
            with torch.no_grad():
                res = timed([run, lambda: F.relu(F.conv2d(xs, w, bias, stride, 1))] + ([run_gemm] if gemm_ok else []) +
                            [lambda d=d: run(d) for d in divs], args.iters, args.warmup, args.repeats)
                tn, tt = res[0], res[1]
                tg = res[2] if gemm_ok else None
                res = res[:2] + res[3 if gemm_ok else 2:]
                run()
                ref = F.relu(F.conv2d(xs, w, bias, stride, 1))
            d = (NF.rows_to_nchw(out, (B, cout, ho, wo)) - ref).abs().max().item() / ref.abs().max().item()
            flop = 2.0 * B * ho * wo * 9 * cin * cout
            say(f"  {str((cin, cout, stride, H, W)):>40} {flop * 1e-9:7.1f} {ms(tn):>28} {flop / tn[0] * 1e-12:8.1f} "
                f"{ms(tt):>28} {flop / tt[0] * 1e-12:8.1f} {tn[0] / tt[0]:12.2f}   (rel. difference {d:.1e}; by nb: " +
                ", ".join(f"{q} {t[0] * 1e3:.3f}" for q, t in zip(divs, res[2:])) +
                (f"; cmt_gemm CMT_A_CONV3X3 {ms(tg).strip()} ms, bit-equal {torch.equal(out_g.view(torch.int16), out.view(torch.int16))}"
                 if gemm_ok else "") + ")")
            del xs, rows, out, ref

    else:
        chain = TorchChain(m)

        def under(mode):
            def f():
                NI.set_img_precision(mode)
                return m(x)
            return f

        if args.precision == "both":
            tr, tn, tt = timed([under("ref"), under("fp16"), lambda: chain(x)], args.iters, args.warmup, args.repeats)
            say(f"whole forward (launches and allocations included), alternating windows: 'ref' {ms(tr)} ms, 'fp16' "
                f"{ms(tn)} ms, torch fp32 {ms(tt)} ms; fp16/ref {tn[0] / tr[0]:.3f}, ref/torch {tr[0] / tt[0]:.2f}, "
                f"fp16/torch {tn[0] / tt[0]:.2f}; windows apart: {tn[2] < tr[1]}")
            say("below: 'fp16' against the torch fp32 chain")
            NI.set_img_precision("fp16")
        else:
            NI.set_img_precision(args.precision)
            tn, tt = timed([lambda: m(x), lambda: chain(x)], args.iters, args.warmup, args.repeats)
        say(f"whole forward (launches and allocations included): native {ms(tn)} ms, torch fp32 {ms(tt)} ms, "
            f"native/torch {tn[0] / tt[0]:.2f}")
        outs, ref = m(x), chain(x)
        torch.cuda.synchronize()
        m.check_input_range()
        for k in ref:
            d, top = (outs[k] - ref[k]).abs().max().item(), ref[k].abs().max().item()
            say(f"{k} {tuple(outs[k].shape)}: native against the torch fp32 chain: max abs difference {d:.3e} over max "
                f"abs {top:.3f} = {d / top:.2e} (sanity figure, both sides carry rounding)")
        say(f"peak device memory {torch.cuda.max_memory_allocated() / 2 ** 20:.0f} MiB")
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "a") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
