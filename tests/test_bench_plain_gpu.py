"""The plain one-GPU command of bench.py (`--gpus 1 --steps K --warmup W`, no --full): the lean result line, and
`--dump-outputs DIR` = the planned ZMPs of the LAST timed step, which the seeded ring of batches makes reproducible."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_plain_line_and_dumped_outputs(tmp_path):
    import torch

    from centroidalcontrolcollection_amd import LinearMpcZmp
    from centroidalcontrolcollection_amd import fixtures as fx

    n, steps, warmup, ramp = 4096, 3, 1, 2
    out = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", str(steps), "--warmup",
                          str(warmup), "--ramp-steps", str(ramp), "--batch", str(n), "--dump-outputs", str(tmp_path / "dump")],
                         capture_output=True, text=True, timeout=300, cwd=str(tmp_path))
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-2000:]
    lines = [ln for ln in out.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1
    d = json.loads(lines[0])
    assert d["steps"] == steps and d["warmup"] == warmup and d["n_gpus"] == 1 and d["dtype"] == "f64"
    assert d["unit"] == "solves/s" and d["higher_is_better"] is True and d["ms_per_step"] > 0
    assert abs(d["value"] - n / (d["ms_per_step"] * 1e-3)) < 1e-6 * d["value"]
    # what --full measures beside the timed steps is not in a plain line
    assert not set(d) & {"secondary", "cpu_baseline", "history", "roofline", "p50_ms", "strong_scaling", "unsolved"}

    assert sorted(os.listdir(tmp_path / "dump")) == ["zmp.npy"]
    zmp = np.load(tmp_path / "dump" / "zmp.npy")
    assert zmp.dtype == np.float64 and zmp.shape == (n, 2)
    # launch number ramp + warmup + steps solved batch (ramp + warmup + steps - 1) mod 8 of the ring (seed 20250928 + k on
    # rank 0); the answers are the same bits whatever schedule the handle's history gave that launch
    b = fx.make_zmp_batch(n, 32, 0.0625, 1.0, seed=20250928 + (ramp + warmup + steps - 1) % 8)
    dev = torch.device("cuda:0")
    want = torch.empty((n, 2), dtype=torch.float64, device=dev)
    status = torch.empty((n, 2), dtype=torch.int32, device=dev)
    x0, zlim = torch.from_numpy(b["x0"]).to(dev), torch.from_numpy(b["zlim"]).to(dev)
    mpc = LinearMpcZmp(1.0, 2.0, 0.0625, device=0)
    mpc.plan_batch_device(x0, zlim, 0.005, want, None, status)
    torch.cuda.synchronize()
    assert np.all((status.cpu().numpy() & 0xff) == 0)
    assert np.array_equal(zmp, want.cpu().numpy())
