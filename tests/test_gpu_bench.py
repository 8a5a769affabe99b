"""bench.py as the driver runs it, in a child process on the GPU: a plain run
times exactly --steps steps and prints the headline line only (no --full leg),
and --dump-outputs writes what the last timed step (a HIP-graph replay of the
CmtHead forward) returned, one float32 .npy per output tensor.  The dumped
class logits are compared with a direct forward of the same seeded frame in
this process: both run the same kernels on the same inputs and each is held to
1e-3 of the oracle (north_star), hence the 2e-3 bound between them."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from conftest import ROOT

pytestmark = pytest.mark.gpu

STEPS, WARMUP = 3, 1
FULL_ONLY = ("roofline", "bf16_policy", "weight_only_recomputed", "voxel_scatter_mean_ms", "lidar", "stress4",
             "train_coop", "cpu_baseline")


def test_plain_run_line_and_dumped_outputs(dev, tmp_path, parity_log):
    out = tmp_path / "dump"
    p = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", str(STEPS),
                        "--warmup", str(WARMUP), "--dump-outputs", str(out)],
                       capture_output=True, text=True, timeout=120)
    assert p.returncode == 0, p.stderr[-2000:]
    lines = [ln for ln in p.stdout.splitlines() if ln.strip()]
    assert len(lines) == 1, p.stdout
    r = json.loads(lines[0])
    assert r["steps"] == STEPS and r["warmup"] == WARMUP and r["n_gpus"] == 1
    assert r["unit"] == "frames/s" and r["higher_is_better"] is True and r["dtype"].startswith("fp32")
    assert r["ms_per_step"] > 0
    # one frame per step: value and ms_per_step are the same measurement (both rounded on the line)
    assert abs(r["value"] * r["ms_per_step"] / 1e3 - 1.0) < 1e-3
    assert not [k for k in FULL_ONLY if k in r]

    import bench
    from projects.mmdet3d_plugin import get_precision, set_precision
    prev = get_precision()
    set_precision(bench.WORKLOADS["fusion"]["precision"])
    try:
        _, _, step, _, _ = bench.make_workload("fusion", seed=0, device=dev)
        with torch.no_grad():
            want = dict(bench.named_arrays(step()))
        torch.cuda.synchronize()
    finally:
        set_precision(prev)
    files = sorted(os.listdir(out))
    assert files == sorted(k + ".npy" for k in want)
    total = 0
    for name, t in want.items():
        a = np.load(out / (name + ".npy"))
        total += a.nbytes
        assert a.dtype == np.float32 and list(a.shape) == list(t.shape), name
        assert np.isfinite(a).all(), name
    assert total <= bench.DUMP_LIMIT_BYTES
    key = "out_0_0_cls_logits"
    err = float(np.abs(np.load(out / (key + ".npy")) - want[key].float().cpu().numpy()).max())
    parity_log.append(f"bench.py --dump-outputs cls_logits (graph replay, child process) vs a direct forward: "
                      f"max abs {err:.2e} bound 2e-3")
    assert err <= 2e-3
