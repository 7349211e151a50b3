"""Throughput of the one-launch StepMpc closed loop (ccc_step_closed_loop_device) beside the planner kernel it is built
round (ccc_step_plan_batch_device): 65536 random footstep timelines, 2000 cycles of 5 ms from rest with a push at 4.5 s,
the footstep update on.

    python scripts/step_mpc_loop_throughput.py [--n 65536] [--cycles 2000] [--out FILE]

Prints one JSON line: instance-cycles/s of the loop (device events round one launch each, median over `--repeats` launches
after `--warmup` launches) and solves/s of the planner kernel on element lists of the same timelines at random times
(events round `--plan-launches` launches).  There is no CPU path: without a gfx950 device the handle's constructor raises.
"""
import argparse
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from centroidalcontrolcollection_amd import StepMpc, fixtures, step_mpc  # noqa: E402

H, SIM_DT = 1.0, 0.005


def planner_batch(tl, n, rng, phases=512):
    """n planner instances drawn from the element lists of `phases` of the timelines at random times in [0, 8) s."""
    ref_data, times = [], rng.uniform(0.0, 8.0, phases)
    for k, t in enumerate(times):
        fm = fixtures.FootstepManager({fixtures.LEFT: tl["foot0"][k, 0].copy(), fixtures.RIGHT: tl["foot0"][k, 1].copy()})
        for j in range(tl["foot_id"].shape[1]):
            fm.footstep_list_.append(fixtures.Footstep(int(tl["foot_id"][k, j]), tl["foot_pos"][k, j],
                                                       tl["swing_start"][k, j] - 0.1, 0.2, 0.8))
        fm.update(t)
        ref_data.append(fm.makeStepMpcRefData(t))
    num, flags, end_time, zmp = step_mpc.pack_ref_data(ref_data)
    pick = rng.integers(0, phases, n)
    x0 = np.concatenate([zmp[pick, 0] + rng.uniform(-0.03, 0.03, (n, 2)), rng.uniform(-0.2, 0.2, (n, 2))], axis=1)
    return num[pick], flags[pick], end_time[pick], zmp[pick], x0, times[pick]


def timed(launch, launches, repeats, dev):
    import torch

    ms = []
    for _ in range(repeats):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(launches):
            launch()
        b.record()
        b.synchronize()
        ms.append(a.elapsed_time(b) / launches)
    return float(np.median(ms)), float(min(ms)), float(max(ms))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=65536)
    ap.add_argument("--cycles", type=int, default=2000)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--plan-launches", type=int, default=500)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()

    import torch

    n = args.n
    mpc = StepMpc(H)
    dev = torch.device("cuda", mpc.device)
    up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)  # noqa: E731
    tl = fixtures.make_zmp_timelines(n)
    tl["transit_end"] = tl["swing_end"] + 0.1
    tl_d = {k: up(v) for k, v in tl.items()}
    foot_pos0 = tl_d["foot_pos"].clone()
    com = torch.zeros((n, 2, 2), dtype=torch.float64, device=dev)
    status, updates = (torch.zeros(n, dtype=torch.int32, device=dev) for _ in range(2))

    def loop():
        com.zero_()  # every launch walks the same timelines from rest
        tl_d["foot_pos"].copy_(foot_pos0)
        updates.zero_()
        mpc.closed_loop_device(tl_d, com, 0.0, SIM_DT, args.cycles, (4.5,), 0.05, None, status, updates)

    for _ in range(args.warmup):  # code object load, clock ramp
        loop()
    torch.cuda.synchronize(dev)
    med, lo, hi = timed(loop, 1, args.repeats, dev)
    st = status.cpu().numpy()
    line = dict(workload="step_mpc_closed_loop", n=n, cycles=args.cycles, loop_ms_per_launch=med, loop_ms_min=lo, loop_ms_max=hi,
                loop_instance_cycles_per_s=n * args.cycles / (med * 1e-3), instances_solved=int((st == 0).sum()),
                footstep_updates_per_instance=float(updates.cpu().numpy().mean()))

    host = planner_batch(tl, n, np.random.default_rng(1))
    num, flags, end_time, zmp, x0, t = (up(a) for a in host)
    cur, foot = (torch.zeros((n, 2), dtype=torch.float64, device=dev) for _ in range(2))

    def plan():
        mpc.plan_batch_device(num, flags, end_time, zmp, x0, t, cur, foot, status)

    for _ in range(args.plan_launches):
        plan()
    torch.cuda.synchronize(dev)
    med, lo, hi = timed(plan, args.plan_launches, args.repeats, dev)
    line.update(planner_ms_per_launch=med, planner_ms_min=lo, planner_ms_max=hi, planner_solves_per_s=n / (med * 1e-3),
                planner_mean_elements=float(host[0].mean()))
    line["loop_over_planner"] = line["loop_instance_cycles_per_s"] / line["planner_solves_per_s"]
    print(json.dumps(line))
    if args.out:
        with open(args.out, "w") as f:
            f.write(json.dumps(line) + "\n")
    return 0 if line["instances_solved"] == n else 1


if __name__ == "__main__":
    sys.exit(main())
