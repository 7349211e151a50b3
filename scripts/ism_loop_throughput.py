"""Throughput of the one-launch IntrinsicallyStableMpc closed loop (ccc_ism_closed_loop_device), warm and cold, against
the host-driven loop it replaces: per cycle the references sampled on the CPU, one plan_batch_device, a round trip and the
simulator on the CPU.  Same random footstep timelines, N = 100 (horizon 2 s at 0.02 s), sim_dt = 0.005 s.

    python scripts/ism_loop_throughput.py [--n 16384] [--cycles 200] [--host-cycles 20] [--out FILE]

Prints one JSON line: instance-cycles/s of the three loops and the mean tridiagonal solves per axis and cycle, warm
against cold, from the status words.  The device loops are timed with device events round `--launches` back-to-back
launches after a warm-up (median over `--repeats` windows); the host-driven loop with the wall clock round its cycles,
since most of it is host work.  There is no CPU path: without a gfx950 device the handle's constructor raises.
"""
import argparse
import json
import math
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from centroidalcontrolcollection_amd import IntrinsicallyStableMpc, fixtures  # noqa: E402
from centroidalcontrolcollection_amd.intrinsically_stable_mpc import timeline_knots  # noqa: E402

H, T, DT, SIM_DT, N = 1.0, 2.0, 0.02, 0.005, 100


def host_driven(mpc, tl, knots, n, cycles, dev):
    """plan_batch_device driven from the host, as tests/test_ism_gpu.py drives planOnce: seconds per cycle."""
    import torch

    num, kt, kz = knots
    sim = fixtures.ComZmpSim2d(H, SIM_DT)
    x, y, zmp, t = np.zeros((n, 2)), np.zeros((n, 2)), np.zeros((n, 2)), 0.0
    zd, rows = torch.zeros((n, 2), dtype=torch.float64, device=dev), np.arange(n)[:, None]
    torch.cuda.synchronize(dev)
    t_start = time.perf_counter()
    for _ in range(cycles):
        times = np.tile((t + DT * np.arange(N)) + 2e-6, (n, 1))
        lo, hi = fixtures.zmp_limits_timeline(times=times, **tl)
        live = np.arange(kt.shape[1])[None, None, :] < num[:, None, None]
        j = np.clip(((kt[:, None, :] <= times[:, :, None]) & live).sum(axis=2), 1, num[:, None] - 1)
        r = np.clip((times - kt[rows, j - 1]) / (kt[rows, j] - kt[rows, j - 1]), 0.0, 1.0)[..., None]
        ref = np.stack([(1 - r) * kz[rows, j - 1] + r * kz[rows, j], lo, hi], axis=1).transpose(0, 3, 1, 2)
        cp = np.stack([x[:, 0] + math.sqrt(H / fixtures.G) * x[:, 1], y[:, 0] + math.sqrt(H / fixtures.G) * y[:, 1]], axis=1)
        init = np.stack([cp, zmp], axis=2)
        mpc.plan_batch_device(torch.from_numpy(init).to(dev), torch.from_numpy(np.ascontiguousarray(ref)).to(dev), SIM_DT, zd)
        zmp = zd.cpu().numpy()
        x, y = x @ sim.Ad.T + zmp[:, :1] * sim.Bd, y @ sim.Ad.T + zmp[:, 1:] * sim.Bd
        t += SIM_DT
    return (time.perf_counter() - t_start) / cycles


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=16384)
    ap.add_argument("--cycles", type=int, default=200)
    ap.add_argument("--host-cycles", type=int, default=20)
    ap.add_argument("--launches", type=int, default=5)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()

    import torch

    n = args.n
    mpc = IntrinsicallyStableMpc(H, T, DT)
    dev = torch.device("cuda", mpc.device)
    tl = fixtures.make_zmp_timelines(n)
    knots = timeline_knots(tl)
    up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)  # noqa: E731
    tl_d, knots_d = {k: up(v) for k, v in tl.items()}, tuple(up(a) for a in knots)
    com0, zmp0 = torch.zeros((n, 2, 2), dtype=torch.float64, device=dev), torch.zeros((n, 2), dtype=torch.float64, device=dev)
    com, zmp = com0.clone(), zmp0.clone()
    status = torch.zeros((n, 2), dtype=torch.int32, device=dev)
    line = dict(workload="ism_closed_loop", n=n, horizon_steps=N, cycles=args.cycles)
    for tag, warm in (("warm", True), ("cold", False)):
        def launch():
            com.copy_(com0)  # every launch walks the same 1 s from rest
            zmp.copy_(zmp0)
            mpc.closed_loop_device(tl_d, knots_d, com, zmp, 0.0, SIM_DT, args.cycles, (0.5,), 0.05, warm, status)

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
        st = status.cpu().numpy()
        ok = (st & 0xff) == 0
        line.update({tag + "_ms_per_launch": float(np.median(ms)), tag + "_ms_min": float(min(ms)), tag + "_ms_max": float(max(ms)),
                     tag + "_instance_cycles_per_s": n * args.cycles / (float(np.median(ms)) * 1e-3),
                     tag + "_solves_per_axis_cycle": float((st >> 8)[ok].mean() / args.cycles), tag + "_axes_solved": int(ok.sum())})
    host_driven(mpc, tl, knots, n, 2, dev)  # warm-up
    s = host_driven(mpc, tl, knots, n, args.host_cycles, dev)
    line.update(host_driven_s_per_cycle=s, host_driven_instance_cycles_per_s=n / s,
                speedup_warm_over_host_driven=line["warm_instance_cycles_per_s"] / (n / s))
    print(json.dumps(line))
    if args.out:
        with open(args.out, "w") as f:
            f.write(json.dumps(line) + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
