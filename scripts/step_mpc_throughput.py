"""Throughput of the batched StepMpc kernel: 65536 timelines from FootstepManager.makeStepMpcRefData of the reference
scenario at random phases, inputs resident on the device, timed with device events after a warm-up.

    python scripts/step_mpc_throughput.py [--n 65536] [--launches 2000] [--out profiles/step_mpc_throughput.json]

Prints one JSON line: solves/s and ms per launch (median and spread over `--repeats` windows of `--launches` launches).
There is no CPU path: without a gfx950 device the handle's constructor raises.
"""
import argparse
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from centroidalcontrolcollection_amd import StepMpc, fixtures, step_mpc  # noqa: E402


def make_batch(n, seed=20250928, phases=512):
    """n instances drawn from `phases` timelines of the reference scenario at random times in [0, 9) s, each with its own
    random CoM state."""
    rng = np.random.default_rng(seed)
    ref_data, times = [], rng.uniform(0.0, 9.0, phases)
    for t in times:
        fm = fixtures.FootstepManager()
        for fs in fixtures.reference_scenario_footsteps():
            fm.appendFootstep(fs)
        fm.update(t)
        ref_data.append(fm.makeStepMpcRefData(t))
    num, flags, end_time, zmp = step_mpc.pack_ref_data(ref_data)
    pick = rng.integers(0, phases, n)
    x0 = np.concatenate([zmp[pick, 0] + rng.uniform(-0.03, 0.03, (n, 2)), rng.uniform(-0.2, 0.2, (n, 2))], axis=1)
    return num[pick], flags[pick], end_time[pick], zmp[pick], x0, times[pick]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=65536)
    ap.add_argument("--launches", type=int, default=2000)
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2000)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()

    import torch

    mpc = StepMpc(1.0)
    dev = torch.device("cuda", mpc.device)
    host = make_batch(args.n)
    num, flags, end_time, zmp, x0, t = (torch.from_numpy(np.ascontiguousarray(a)).to(dev) for a in host)
    cur, foot = torch.zeros((args.n, 2), dtype=torch.float64, device=dev), torch.zeros((args.n, 2), dtype=torch.float64, device=dev)
    status = torch.zeros(args.n, dtype=torch.int32, device=dev)

    def launch():
        mpc.plan_batch_device(num, flags, end_time, zmp, x0, t, cur, foot, status)

    for _ in range(args.warmup):  # code object load, clock ramp
        launch()
    torch.cuda.synchronize(dev)
    ms = []
    for _ in range(args.repeats):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(args.launches):
            launch()
        b.record()
        b.synchronize()
        ms.append(a.elapsed_time(b) / args.launches)
    solved = int((status.cpu().numpy() & 0xff == 0).sum())
    med = float(np.median(ms))
    line = dict(workload="step_mpc", n=args.n, mean_elements=float(host[0].mean()), launches=args.launches,
                ms_per_launch=med, ms_per_launch_min=float(min(ms)), ms_per_launch_max=float(max(ms)),
                solves_per_s=args.n / (med * 1e-3), solved=solved)
    print(json.dumps(line))
    if args.out:
        with open(args.out, "w") as f:
            f.write(json.dumps(line) + "\n")
    return 0 if solved == args.n else 1


if __name__ == "__main__":
    sys.exit(main())
