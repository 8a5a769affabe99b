"""Bits of the training attention kernels of two builds of the library against each other: O, LSE, dQ,
dK and dV for a fixed list of small cases (test_gpu_train_attn_x3.py's CASES without the coop shape)
in the three arithmetics (exact f32, the flash fp16 core, bf16x3), each with p = 0 and with its own p.

    python dev/attn_train_bits.py run OLD_LIB.so NEW_LIB.so [--out DIR] [--timeout S]
        one child process per library (CMT_HIP_LIB selects it, each under its own time limit) dumps
        the outputs; the two dumps are then compared
    python dev/attn_train_bits.py dump OUT.pt        (the child: the library of CMT_HIP_LIB)
    python dev/attn_train_bits.py compare OLD.pt NEW.pt

Required of the comparison (a refactor of csrc/attn_train.hip that moves the exact-f32 kernels'
dropout scale from every P to O / dV):
    f16, bf16x3   bitwise equal where the launch has one split; a gradient summed by f32 atomics over
                  splits within 1e-5 of its max (the re-association figure of
                  test_attention_train_bwd_reuses_forward_copies)
    f32, p = 0    the same
    f32, p > 0    LSE bitwise (the statistics are computed before dropout); O, dQ, dK within 1e-5 of
                  the output's max; dV bitwise where unsplit
Prints the observed maximum of |old - new| / max|old| per output and the verdict; exit status 3 if a
requirement is missed."""
import argparse
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
H, C = 8, 256
SEED = 1234
CASES = [(1, 100, 1000, 0, 0, 0.0), (2, 70, 70, 30, 10, 0.0), (1, 140, 140, 40, 8, 0.25), (1, 33, 65, 0, 0, 0.0),
         (1, 300, 300, 60, 20, 0.1)]
ARITH = ("f32", "f16", "bf16x3")
NAMES = ("O", "LSE", "dQ", "dK", "dV")
ATOMIC_TOL = 1e-5


def cdiv(a, b):
    return -(-a // b)


def splits(arith, B, Nq, Nk):
    """(dQ key splits, dK / dV query splits) of the backward entry points (csrc/attn_train.hip)"""
    ntiles, nqt = cdiv(Nk, 64), cdiv(Nq, 64)
    wq, wk = cdiv(Nq, 128) * B * H, cdiv(Nk, 128) * B * H
    cap_q, cap_k = (432, 288) if arith == "bf16x3" else (768, 512)
    qs = max(1, min(ntiles // 2, cap_q // wq))
    ks = 1 if arith == "f16" else max(1, min(nqt // 2, cap_k // wk))
    return qs, ks


def runs():
    for case in CASES:
        for p in sorted({0.0, case[5]}):
            for arith in ARITH:
                yield case[:5] + (p,), arith


def key(case, arith):
    return "%s B=%d %dx%d dn %d/%d p=%g" % ((arith,) + case)


def dump(path):
    sys.path.insert(0, os.path.join(ROOT, "cmt-cooperative-perception_amd"))
    import torch
    from projects.mmdet3d_plugin import native_train as T
    dev = torch.device("cuda")
    out = {}
    for case, arith in runs():
        B, Nq, Nk, pad, grp, p = case
        g = torch.Generator().manual_seed(Nq * 7 + Nk)
        q, k, v, do = (torch.randn(B, n, C, generator=g).to(dev) for n in (Nq, Nk, Nk, Nq))
        o, lse = torch.empty_like(q), torch.empty(B * H * Nq, device=dev)
        dq, dk, dv = torch.empty_like(q), torch.empty_like(k), torch.empty_like(v)
        kw = dict(B=B, H=H, Nq=Nq, Nk=Nk, q_strides=(Nq * C, 32, C), k_strides=(Nk * C, 32, C),
                  v_strides=(Nk * C, 32, C), o_strides=(Nq * C, 32, C), scale=32 ** -0.5, dn_pad=pad, dn_group=grp,
                  fp16_inputs=arith == "f16", dropout_p=p, seed=SEED, mode="bf16x3" if arith == "bf16x3" else "f32")
        ws = T.attn_train_fwd(q, k, v, o, lse, **kw)
        T.attn_train_bwd(q, k, v, o, lse, do, dq, dk, dv, ws=ws, **kw)
        torch.cuda.synchronize()
        out[key(case, arith)] = [t.cpu() for t in (o, lse, dq, dk, dv)]
    torch.save(out, path)
    print("attn_train_bits: %d runs of %s -> %s" % (len(out), os.environ.get("CMT_HIP_LIB", "the default library"), path))


def compare(old_path, new_path):
    import torch
    old, new = torch.load(old_path), torch.load(new_path)
    missed = 0
    worst = {}
    for case, arith in runs():
        B, Nq, Nk, _, _, p = case
        qs, ks = splits(arith, B, Nq, Nk)
        moved = arith == "f32" and p > 0            # the dropout scale's place: one re-association
        line = []
        for name, a, b in zip(NAMES, old[key(case, arith)], new[key(case, arith)]):
            atomic = (name == "dQ" and qs > 1) or (name in ("dK", "dV") and ks > 1)
            loose = atomic or (moved and name in ("O", "dQ", "dK"))
            same = torch.equal(a, b)
            rel = ((a.double() - b.double()).abs().max() / a.double().abs().max()).item()
            ok = same or (loose and rel <= ATOMIC_TOL)
            missed += not ok
            cls = (arith, "p>0" if p > 0 else "p=0", name, "1e-5" if loose else "bitwise")
            worst[cls] = max(worst.get(cls, 0.0), rel)
            line.append("%s %s" % (name, "=" if same else ("%.1e%s" % (rel, "" if ok else " MISSED (%s)" % cls[3]))))
        print("%-40s dQ x%d dK/dV x%d  %s" % (key(case, arith), qs, ks, "  ".join(line)))
    print("observed maxima of |old - new| / max|old| (requirement):")
    for cls in sorted(worst):
        print("    %-7s %s %-3s  %.2e  (%s)" % (cls[0], cls[1], cls[2], worst[cls], cls[3]))
    print("attn_train_bits: %s" % ("every requirement met" if not missed else "%d MISSED" % missed))
    return 3 if missed else 0


def run(old_lib, new_lib, out, timeout):
    os.makedirs(out, exist_ok=True)
    paths = []
    for tag, lib in (("old", old_lib), ("new", new_lib)):
        path = os.path.join(out, "attn_train_bits_%s.pt" % tag)
        env = dict(os.environ, CMT_HIP_LIB=os.path.abspath(lib))
        rc = subprocess.run([sys.executable, os.path.abspath(__file__), "dump", path], env=env, timeout=timeout).returncode
        if rc != 0:
            print("attn_train_bits: the %s library's run ended with status %d; nothing more is started" % (tag, rc))
            return rc
        paths.append(path)
    return compare(*paths)


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    sub = ap.add_subparsers(dest="cmd", required=True)
    r = sub.add_parser("run")
    r.add_argument("old_lib")
    r.add_argument("new_lib")
    r.add_argument("--out", default=os.path.join(ROOT, "build", "attn_train_bits"))
    r.add_argument("--timeout", type=int, default=240)
    d = sub.add_parser("dump")
    d.add_argument("path")
    c = sub.add_parser("compare")
    c.add_argument("old")
    c.add_argument("new")
    a = ap.parse_args()
    if a.cmd == "dump":
        return dump(a.path) or 0
    if a.cmd == "compare":
        return compare(a.old, a.new)
    return run(a.old_lib, a.new_lib, a.out, a.timeout)


if __name__ == "__main__":
    sys.exit(main())
