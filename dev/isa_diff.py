#!/usr/bin/env python3
"""Per-kernel comparison of two device assembly files (hipcc -S --offload-device-only).

    dev/isa_diff.py OLD.s NEW.s [--rename 'REGEX=REPL' ...] [--only REGEX] [--show N]

Kernels are matched on their demangled names; --rename rewrites OLD's names first (for template
arguments a refactor removed, e.g. 'gemm_x3_kernel<256, =gemm_x3_kernel<').  For every kernel:
instruction count old -> new, VGPR / AGPR / scratch / LDS from the kernel descriptor, SGPR and VGPR
spill counts from the metadata, s_barrier count, and
'identical' or the number of differing lines once .LBB label numbers are normalised.  For a kernel
that differs, 'k loop' says whether the ordered sequence of MFMA, ds_read, LDS-DMA and s_waitcnt
instructions (mnemonics and wait counts, no registers) inside its loops that hold MFMAs is the
same.  It only diffs two files.  Names are demangled with c++filt (--cxxfilt PATH for another).
"""
import argparse
import difflib
import re
import subprocess
import sys

PIPE = re.compile(r"^(v_mfma|v_smfmac|ds_read|ds_load|global_load_lds|buffer_load.*\blds\b|s_waitcnt)")


def demangle(names, tool):
    if not names:
        return {}
    # older c++filt builds do not know the _Float16 / __bf16 manglings: spell them as vendor types
    text = "\n".join(names).replace("DF16_", "u8_Float16").replace("DF16b", "u6__bf16")
    out = subprocess.run([tool], input=text, capture_output=True, text=True, check=True).stdout
    return dict(zip(names, out.split("\n")))


def short(name):
    name = name.replace("(anonymous namespace)::", "")
    name = re.sub(r"^void ", "", name)
    return re.sub(r"\(cmt_\w+.*\)$", "", name)     # drop the parameter list


def parse(path):
    """{mangled: {"body": [normalised lines], "desc": {field: int}}} for every kernel of the file"""
    kernels, cur, desc = {}, None, None
    labels = {}
    for raw in open(path, errors="replace"):
        line = raw.split(";")[0].rstrip()
        s = line.strip()
        if desc is not None:                   # inside a kernel descriptor
            if s == ".end_amdhsa_kernel":
                desc = None
            else:
                m = re.match(r"^\.amdhsa_(\w+)\s+(\d+)$", s)
                if m:
                    kernels[desc]["desc"][m.group(1)] = int(m.group(2))
            continue
        m = re.match(r"^\.amdhsa_kernel\s+(\S+)", s)
        if m:
            desc = m.group(1)
            kernels.setdefault(desc, {"body": [], "desc": {}})
            continue
        if cur is None:
            m = re.match(r"^(\w+):$", line)
            if m and "; @" in raw:
                cur, labels = m.group(1), {}
                kernels.setdefault(cur, {"body": [], "desc": {}})
            continue
        if s.startswith(".Lfunc_end"):
            cur = None
            continue
        if not s or s.startswith(".") and not s.startswith(".LBB"):
            continue
        # .LBB<function>_<block> -> numbered in order of first appearance inside the kernel
        s = re.sub(r"\.LBB\d+_\d+", lambda m: labels.setdefault(m.group(0), "L%d" % len(labels)), s)
        kernels[cur]["body"].append(re.sub(r"\s+", " ", s))
    name = None                                # the metadata's spill counts (.name comes before them in an entry)
    for raw in open(path, errors="replace"):
        m = re.match(r"^\s+(?:- )?\.(name|sgpr_spill_count|vgpr_spill_count):\s+(\S+)", raw)
        if m and m.group(1) == "name":
            name = m.group(2)
        elif m and name in kernels:
            kernels[name]["desc"][m.group(1)] = int(m.group(2))
    return {k: v for k, v in kernels.items() if v["desc"]}


def regs(d):
    acc = d.get("accum_offset", d.get("next_free_vgpr", 0))
    return (acc, max(0, d.get("next_free_vgpr", 0) - acc), d.get("private_segment_fixed_size", 0),
            d.get("group_segment_fixed_size", 0))


def insts(body):
    return [l for l in body if not l.endswith(":")]


def barriers(body):
    return sum(1 for l in body if l.split(" ", 1)[0] == "s_barrier")


def pipe(body):
    """the memory / MFMA instruction stream of the innermost loops (backward branches) that contain MFMAs"""
    pos = {l[:-1]: i for i, l in enumerate(body) if l.endswith(":")}
    loops = []
    for i, l in enumerate(body):
        m = re.match(r"^s_c?branch\w* (L\d+)$", l)
        if m and pos.get(m.group(1), i) < i and any(x.startswith("v_mfma") for x in body[pos[m.group(1)]:i]):
            loops.append((pos[m.group(1)], i))
    inside = [False] * len(body)
    for a, b in loops:                         # innermost only: no other MFMA loop inside it
        if not any((c, d) != (a, b) and a <= c and d <= b for c, d in loops):
            inside[a:b] = [True] * (b - a)
    seq = []
    for l in (x for x, k in zip(body, inside) if k and not x.endswith(":")):
        if PIPE.match(l):
            op = l.split(" ", 1)
            seq.append(l if op[0] == "s_waitcnt" else op[0])
    return seq


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("old")
    ap.add_argument("new")
    ap.add_argument("--rename", action="append", default=[], help="REGEX=REPL applied to OLD's demangled names")
    ap.add_argument("--only", default=None, help="only kernels whose name matches this regex")
    ap.add_argument("--show", type=int, default=0, help="print the first N diff lines of a differing kernel")
    ap.add_argument("--cxxfilt", default="c++filt")
    args = ap.parse_args()
    old, new = parse(args.old), parse(args.new)
    dn = demangle(sorted(set(old) | set(new)), args.cxxfilt)

    def names(ks, rename):
        out = {}
        for k in ks:
            n = short(dn[k])
            for r in rename:
                pat, rep = r.split("=", 1)
                n = re.sub(pat, rep, n)
            out[n] = k
        return out

    on, nn = names(old, args.rename), names(new, [])
    rows, same, differ = [], 0, 0
    for n in sorted(set(on) | set(nn)):
        if args.only and not re.search(args.only, n):
            continue
        if n not in nn:
            rows.append((n, "removed (%d instructions)" % len(insts(old[on[n]]["body"]))))
            continue
        if n not in on:
            rows.append((n, "added (%d instructions)" % len(insts(new[nn[n]]["body"]))))
            continue
        o, w = old[on[n]], new[nn[n]]
        ro, rw = regs(o["desc"]), regs(w["desc"])
        head = "%6d -> %6d  vgpr %3d -> %3d  agpr %3d -> %3d  scratch %d -> %d  spills s %d -> %d v %d -> %d  lds %6d -> %6d  barriers %d -> %d" % (
            len(insts(o["body"])), len(insts(w["body"])), ro[0], rw[0], ro[1], rw[1], ro[2], rw[2],
            o["desc"].get("sgpr_spill_count", 0), w["desc"].get("sgpr_spill_count", 0),
            o["desc"].get("vgpr_spill_count", 0), w["desc"].get("vgpr_spill_count", 0), ro[3], rw[3],
            barriers(o["body"]), barriers(w["body"]))
        if o["body"] == w["body"]:
            same += 1
            rows.append((n, head + "  identical"))
            continue
        differ += 1
        d = [l for l in difflib.unified_diff(o["body"], w["body"], lineterm="", n=0)
             if l[:1] in "+-" and l[:3] not in ("+++", "---")]
        verdict = "k loop same" if pipe(o["body"]) == pipe(w["body"]) else "k loop DIFFERS"
        rows.append((n, head + "  %d lines differ, %s" % (len(d), verdict)))
        for l in d[:args.show]:
            rows.append(("", "    " + l))
    width = max([len(n) for n, _ in rows] + [1])
    for n, t in rows:
        print(n.ljust(width), t)
    print("%d kernels identical, %d differ, %d only in one file" % (same, differ, len(rows) - same - differ
                                                                     - sum(1 for n, _ in rows if not n)))
    return 0


if __name__ == "__main__":
    sys.exit(main())
