"""Throughput of the batched PreviewControlZmp / SingularPreviewControlZmp kernels: 65536 instances at N = 200 whose
reference ZMP is FootstepManager's knot list (ref_zmp_list_) of the reference scenario at random phases, inputs resident
on the device, timed with device events after a warm-up.

    python scripts/preview_zmp_throughput.py [--n 65536] [--launches 500] [--out profiles/preview_zmp_throughput.json]

Times, per kind: the sampled entry (ref [n,2,N] already on the device), the knot entry, and for scale the sampled entry
behind what produces ref on the device today (a torch searchsorted + gather interpolation of the same knots).  The
sampled kernel's traffic (16 N + 80 bytes per instance) is set against the rate of a device-to-device copy of the same
buffer measured in the same run (read + write counted).  One ref buffer (210 MB) stays in the 256 MB last-level cache
between launches, so the `_cold` runs rotate through four of them: those are the HBM figures.  Prints one JSON line.  There is no CPU path: without a gfx950
device the constructors raise.
"""
import argparse
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from centroidalcontrolcollection_amd import PreviewControlZmp, SingularPreviewControlZmp, fixtures  # noqa: E402
from centroidalcontrolcollection_amd import preview_control_zmp as pvz  # noqa: E402


def make_batch(n, seed=20250928, phases=512):
    """n instances drawn from `phases` knot lists of the reference scenario at random times in [0, 7.9) s."""
    rng = np.random.default_rng(seed)
    knots, times = [], rng.uniform(0.0, 7.9, phases)
    for t in times:
        fm = fixtures.FootstepManager()
        for fs in fixtures.reference_scenario_footsteps():
            fm.appendFootstep(fs)
        fm.update(t)
        knots.append(list(zip(fm._zmp_times, fm._zmps)))
    num, kt, kz = pvz.pack_knots(knots)
    pick = rng.integers(0, phases, n)
    x0 = rng.uniform(-0.05, 0.05, (n, 2, 3))
    return num[pick], kt[pick], kz[pick], x0, times[pick] + 1e-6


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=65536)
    ap.add_argument("--launches", type=int, default=500)
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=200)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()

    import torch

    n, N, dt = args.n, 200, 0.01
    host = make_batch(n)
    line = dict(workload="preview_zmp", n=n, N=N, mean_knots=float(host[0].mean()), launches=args.launches)
    ok = True
    for name, cls, off in (("preview", PreviewControlZmp, 1), ("singular", SingularPreviewControlZmp, 0)):
        ctl = cls(1.0, 2.0, dt)
        dev = torch.device("cuda", ctl.device)
        num, kt, kz, x0, ct = (torch.from_numpy(np.ascontiguousarray(a)).to(dev) for a in host)
        zmp_s, zmp_k = (torch.zeros((n, 2), dtype=torch.float64, device=dev) for _ in range(2))
        status = torch.zeros(n, dtype=torch.int32, device=dev)
        steps = (torch.arange(N, dtype=torch.float64, device=dev) + off) * dt
        rows = torch.arange(n, device=dev)[:, None]
        unused = torch.arange(pvz.MAX_KNOTS, device=dev)[None, :] >= num[:, None]
        kt_sorted = torch.where(unused, torch.full_like(kt, float("inf")), kt)

        def sample():  # what produces ref on the device today: the comparison rule in torch
            t = ct[:, None] + steps[None, :]
            s = (torch.searchsorted(kt_sorted, t, right=True) - 1).clamp(0, pvz.MAX_KNOTS - 2)
            ta, tb = kt[rows, s], kt[rows, s + 1]
            za, zb = kz[rows, s], kz[rows, s + 1]
            return (za + ((t - ta) / (tb - ta))[..., None] * (zb - za)).permute(0, 2, 1).contiguous()

        ref = sample()
        copy_dst = torch.empty_like(ref)
        refs, turn = [ref] + [ref.clone() for _ in range(3)], [0]

        def cold():
            turn[0] = (turn[0] + 1) % len(refs)
            return refs[turn[0]]

        runs = dict(sampled=lambda: ctl.plan_batch_device(x0, ref, zmp_s, 0.005),
                    knots=lambda: ctl.plan_knots_batch_device(num, kt, kz, x0, ct, zmp_k, 0.005, status=status),
                    sample_then_sampled=lambda: ctl.plan_batch_device(x0, sample(), zmp_s, 0.005),
                    copy=lambda: copy_dst.copy_(ref),
                    sampled_cold=lambda: ctl.plan_batch_device(x0, cold(), zmp_s, 0.005),
                    copy_cold=lambda: copy_dst.copy_(cold()))
        for what, launch in runs.items():
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
            line["%s_%s_ms" % (name, what)] = float(np.median(ms))
            line["%s_%s_ms_minmax" % (name, what)] = [float(min(ms)), float(max(ms))]
        sampled_bytes, copy_bytes = n * (16 * N + 80), 2 * ref.numel() * 8
        gbs = sampled_bytes / line[name + "_sampled_cold_ms"] * 1e-6
        copy_gbs = copy_bytes / line[name + "_copy_cold_ms"] * 1e-6
        line.update({name + "_sampled_plans_per_s": n / line[name + "_sampled_ms"] * 1e3,
                     name + "_sampled_cold_plans_per_s": n / line[name + "_sampled_cold_ms"] * 1e3,
                     name + "_knots_plans_per_s": n / line[name + "_knots_ms"] * 1e3,
                     name + "_sampled_cold_GBps": gbs, name + "_copy_cold_GBps": copy_gbs,
                     name + "_sampled_cold_fraction_of_copy": gbs / copy_gbs,
                     name + "_max_abs_knots_minus_sampled": float((zmp_k - zmp_s).abs().max())})
        ok = ok and int((status != 0).sum()) == 0
    line["all_solved"] = ok
    print(json.dumps(line))
    if args.out:
        with open(args.out, "w") as f:
            f.write(json.dumps(line) + "\n")
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
