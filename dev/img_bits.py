"""Bit-level fingerprint of the image backbone kernels: a fixed list of small seeded cases through the public
wrappers (native_img, native_fpn, VoVNet) in both arithmetics, one line per case with the SHA-256 of the raw output
bytes (and of ``part`` for the concat).  Run it on two builds and compare the outputs line by line: a refactor of
the kernels or wrappers must leave every line equal.

    python dev/img_bits.py [--out FILE]

The shapes are the tests' edge shapes: tiles that straddle image and row ends, a wave past the last row,
all-padding taps, C % 64 == 32 half chunks, column slices, in-place apply.  Inputs come from a CPU generator seeded
by the case's name.  Needs a HIP device and the built library; the whole list runs in seconds.
"""
import argparse
import hashlib
import os
import sys
import zlib

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (os.path.join(ROOT, "cmt-cooperative-perception_amd"), ROOT):
    if p not in sys.path:
        sys.path.insert(0, p)

EPS = 1e-5


def sha(t):
    return hashlib.sha256(t.detach().cpu().contiguous().view(torch.uint8).numpy().tobytes()).hexdigest()


def gen(name):
    return torch.Generator().manual_seed(zlib.crc32(name.encode()))


def bn(n, g):
    return [0.5 + torch.rand(n, generator=g), 0.5 * torch.randn(n, generator=g), 0.5 * torch.randn(n, generator=g),
            0.5 + 1.5 * torch.rand(n, generator=g), EPS]


def to_rows(x, fp16, dev, pad=0):
    """fp32 [rows, C] on the CPU -> the arithmetic's row buffer on the device; ``pad``: as a column slice of a
    buffer that is 2 * pad words wider"""
    hi = x.half()
    flat = hi if fp16 else torch.cat([hi, (x - hi.float()).half()], dim=1)     # a pair row: hi C | lo C
    n = flat.shape[1]
    wide = torch.zeros((flat.shape[0], n + 2 * pad), dtype=torch.float16)
    wide[:, pad:pad + n] = flat
    t = wide.to(dev)[:, pad:pad + n]
    return t if fp16 else t.view(torch.uint16).unflatten(1, (2, x.shape[1]))


def seed_module(mod, name):
    with torch.no_grad():
        for key, t in mod.state_dict().items():
            g = gen(name + key)
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("img_bits needs a HIP device")
    from projects.mmdet3d_plugin import build_backbone
    from projects.mmdet3d_plugin import native_bev as NB
    from projects.mmdet3d_plugin import native_fpn as NF
    from projects.mmdet3d_plugin import native_img as NI
    dev = torch.device("cuda:0")
    lines = []

    def say(mode, name, *tensors):
        torch.cuda.synchronize()
        lines.append(f"{mode:>4} {name} " + " ".join(sha(t) for t in tensors))
        print(lines[-1], flush=True)

    for mode in ("ref", "fp16"):
        f16 = mode == "fp16"
        op = lambda name, mod=NI: getattr(mod, name + "_f16" if f16 else name)   # noqa: E731
        pack3 = NI.pack_conv3x3_f16 if f16 else NB.pack_conv3x3
        B = 2

        for cin in (3, 1):
            for H, W in ((5, 7), (9, 13)):
                name = f"stem {cin}->64 {H}x{W}"
                g = gen(name)
                w, shift = op("pack_stem")(torch.randn(64, cin, 3, 3, generator=g) / (9 * cin) ** 0.5, bn(64, g))
                x = torch.randn(B, cin, H, W, generator=g)
                say(mode, name, op("stem")(x.to(dev), w.to(dev), shift.to(dev), Cout=64))

        def conv(cin, cout, stride, H, W, nb=0):
            name = f"conv3x3 {cin}->{cout} s{stride} {H}x{W}"
            g = gen(name)
            w, shift = pack3(torch.randn(cout, cin, 3, 3, generator=g) / (9 * cin) ** 0.5, bn(cout, g))
            rows = to_rows(torch.randn(B * H * W, cin, generator=g), f16, dev)
            say(mode, f"{name} nb{nb}", op("conv3x3")(rows, w.to(dev), shift.to(dev), B=B, H=H, W=W, Cin=cin, Cout=cout,
                                                      stride=stride, nb=nb))

        for cin, cout in ((32, 64), (96, 32), (160, 160), (224, 224), (64, 128), (32, 256)):
            for stride in (1, 2):
                conv(cin, cout, stride, 13, 17)
        for nb in (1, 2, 4, 8):
            conv(32, 256, 1, 13, 17, nb)
        for nb in (1, 5):
            conv(160, 160, 2, 13, 17, nb)
        conv(96, 64, 1, 1, 45)

        for widths, sliced in (((64,), False), ((128,) * 4, False), ((256,) + (160,) * 5, False), ((32,) * 8, False),
                               ((128,) * 4, True)):
            for cout in (128, 256):
                for HW in (63, 129):
                    name = f"concat1x1 {'+'.join(str(c) for c in widths)}{' sliced' if sliced else ''}->{cout} HW{HW}"
                    g = gen(name)
                    K = sum(widths)
                    w, shift = op("pack_concat")(torch.randn(cout, K, 1, 1, generator=g) / K ** 0.5, bn(cout, g))
                    srcs = []
                    for c in widths:
                        srcs.append(to_rows(torch.randn(B * HW, c, generator=g), f16, dev, pad=16 if sliced else 0))
                    y, part = op("concat1x1")(srcs, w.to(dev), shift.to(dev), B=B, HW=HW, Cout=cout, part=True)
                    say(mode, name, y, part)

        for HW in (1, 63):
            for ident in (False, True):
                for inplace in (False, True):
                    name = f"ese_apply C128 HW{HW}{' identity' if ident else ''}{' in place' if inplace else ''}"
                    g = gen(name)
                    x = to_rows(torch.randn(B * HW, 128, generator=g), f16, dev)
                    r = to_rows(torch.randn(B * HW, 128, generator=g), f16, dev) if ident else None
                    gate = torch.rand(B, 128, generator=g).to(dev)
                    say(mode, name, op("ese_apply")(x, gate, B=B, HW=HW, C=128, identity=r, out=x if inplace else None))

        for H, W in ((2, 2), (3, 3), (4, 5), (5, 7), (10, 14)):
            for C in (128, 160):
                name = f"maxpool C{C} {H}x{W}"
                x = to_rows(torch.randn(B * H * W, C, generator=gen(name)), f16, dev)
                say(mode, name, op("maxpool")(x, B=B, H=H, W=W, C=C))

        for C in (72, 128):
            for H, W in ((1, 1), (7, 9), (8, 8)):
                name = f"rows_to_nchw C{C} HW{H * W}"
                x = to_rows(torch.randn(B * H * W, C, generator=gen(name)), f16, dev)
                say(mode, name, op("rows_to_nchw", NF)(x, (B, C, H, W)))

        NI.set_img_precision(mode)
        for spec, (H, W) in (("V-19-eSE", (37, 53)), ("V-99-eSE", (64, 96))):
            name = f"VoVNet {spec} {H}x{W}"
            m = seed_module(build_backbone(dict(type="VoVNet", spec_name=spec,
                                                out_features=("stem", "stage2", "stage3", "stage4", "stage5"))),
                            name).eval().to(dev)
            outs = m(torch.randn(B, 3, H, W, generator=gen(name)).to(dev))
            m.check_input_range()
            say(mode, name, *outs.values())
        NI.set_img_precision("ref")

    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
