"""GPU tests of the one-launch closed loop of IntrinsicallyStableMpc (csrc/ism_loop.hip, ccc_ism_closed_loop_device)
against a float64 host loop: fixtures.zmp_limits_timeline, linear interpolation of the knots, the dense-QP oracle
(oracle.IntrinsicallyStableMpc.plan_batch, independent of the tridiagonal form) and fixtures.ComZmpSim2d."""
import functools
import math

import numpy as np
import pytest

from centroidalcontrolcollection_amd import IntrinsicallyStableMpc, _lib
from centroidalcontrolcollection_amd import fixtures as fx
from centroidalcontrolcollection_amd.intrinsically_stable_mpc import timeline_knots

pytestmark = pytest.mark.gpu

SIM_DT, H = 0.005, 1.0
# horizon_dt per horizon length: 1 s of horizon at N = 20 (tests/test_ism_gpu.py), 2 s and more from N = 64 on.  (N = 20 at
# 0.02 is a horizon of 0.4 s, which cannot walk the 0.8 s swings of the fixture timelines: the oracle finds the y axis
# infeasible at the first swing start.)
DT = {20: 0.05, 64: 0.03125, 100: 0.02, 127: 0.02, 128: 0.02}
# planned ZMP and CoM of every cycle against the host loop [m].  One plan agrees with the oracle to 1e-9
# (tests/test_ism_gpu.py); what 400 cycles of the loop make of that was measured once on the MI355X (DESIGN.md 9d:
# 1.64e-15 at most over N = 20, 64, 100, 127, warm and cold); the bound is ten times that, rounded up to a power of ten.
BOUND = 1e-13


def _mpc(N):
    return IntrinsicallyStableMpc(H, (N - 0.5) * DT[N], DT[N])  # ceil((N - 0.5) dt / dt) = N whatever the rounding


def _ref_zmp(knots, times):
    """FootstepManager::refZmp on packed knots, constant outside them: [n,T,2]."""
    num, kt, kz = knots
    out = np.empty(times.shape + (2,))
    for k in range(len(num)):
        j = np.searchsorted(kt[k, :num[k]], times[k], side="right")
        j0, j1 = np.clip(j - 1, 0, num[k] - 1), np.clip(j, 0, num[k] - 1)
        r = np.where(j1 > j0, (times[k] - kt[k, j0]) / np.where(j1 > j0, kt[k, j1] - kt[k, j0], 1.0), 0.0)
        out[k] = (1 - r)[:, None] * kz[k, j0] + r[:, None] * kz[k, j1]
    return out


def _sample(tl, knots, t, N):
    """(ref [n,2,3,N], limits at t + 1e-6 [2][n,2]) as the loop samples them at time t."""
    n = len(knots[0])
    times = np.tile((t + DT[N] * np.arange(N)) + 2e-6, (n, 1))
    lo, hi = fx.zmp_limits_timeline(times=times, **tl)
    ref = np.stack([_ref_zmp(knots, times), lo, hi], axis=1).transpose(0, 3, 1, 2)  # [n,3,N,2] -> [n,2,3,N]
    now = fx.zmp_limits_timeline(times=np.full((n, 1), t + 1e-6), **tl)
    return np.ascontiguousarray(ref), (now[0][:, 0], now[1][:, 0])


def _host_loop(N, tl, knots, pos, vel, zmp, t, cycles, disturb_times, impulse):
    """The loop of TestIntrinsicallyStableMpc.cpp:55-100 per axis; an axis whose QP the oracle does not solve stops."""
    from oracle import oracle

    o = oracle.IntrinsicallyStableMpc(H, (N - 0.5) * DT[N], DT[N])
    n = len(pos)
    sims = [fx.ComZmpSim2d(H, SIM_DT) for _ in range(n)]
    for k, s in enumerate(sims):
        s.x, s.y = np.array([pos[k, 0], vel[k, 0]]), np.array([pos[k, 1], vel[k, 1]])
    zmp, alive = zmp.copy(), np.ones((n, 2), bool)
    status, viol = np.zeros((n, 2), np.int64), np.zeros(n, np.int64)
    traj_com, traj_zmp = np.full((cycles, n, 2), np.nan), np.full((cycles, n, 2), np.nan)
    for c in range(cycles):
        ref, (vlo, vhi) = _sample(tl, knots, t, N)
        com = np.array([s.pos() for s in sims])
        cp = com + math.sqrt(H / fx.G) * np.array([s.vel() for s in sims])
        # one axis per oracle instance (its status is per instance); the second slot holds a trivial QP
        init, r2 = np.zeros((2 * n, 2, 2)), np.zeros((2 * n, 2, 3, N))
        init[:, 0, 0], init[:, 0, 1], r2[:, 0] = cp.reshape(-1), zmp.reshape(-1), ref.reshape(2 * n, 3, N)
        r2[:, 1, 1], r2[:, 1, 2] = -1.0, 1.0
        r = o.plan_batch(init, r2, SIM_DT, want_vel=False, nthreads=8)
        ok = alive & (r["status"].reshape(n, 2) == 0)
        status[alive & ~ok] = (c << 8) | _lib.CCC_STATUS_INFEASIBLE
        alive = ok
        zmp = np.where(alive, r["zmp"][:, 0].reshape(n, 2), zmp)
        traj_com[c], traj_zmp[c] = np.where(alive, com, np.nan), np.where(alive, zmp, np.nan)
        viol += (alive & ~((zmp - vlo >= 0) & (vhi - zmp >= 0))).sum(axis=1)
        t += SIM_DT
        kick = any(d <= t < d + SIM_DT for d in disturb_times)
        for k, s in enumerate(sims):
            keep = (s.x, s.y)
            s.update(zmp[k])
            if kick:
                s.addDisturb((impulse, impulse))
            s.x, s.y = (s.x if alive[k, 0] else keep[0]), (s.y if alive[k, 1] else keep[1])
    return dict(traj_com=traj_com, traj_zmp=traj_zmp, status=status, viol=viol)


def _device_loop(mpc, tl, knots, pos, vel, zmp, t, cycles, disturb_times=(), impulse=0.0, warm=True):
    import torch

    dev, n = torch.device("cuda:0"), len(pos)
    up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)  # noqa: E731
    com, z = up(np.stack([pos, vel], axis=2)), up(zmp)
    st, vi = torch.zeros((n, 2), dtype=torch.int32, device=dev), torch.zeros(n, dtype=torch.int32, device=dev)
    tc, tz = (torch.zeros((cycles, n, 2), dtype=torch.float64, device=dev) for _ in range(2))
    mpc.closed_loop_device({k: up(v) for k, v in tl.items()}, tuple(up(a) for a in knots), com, z, t, SIM_DT, cycles,
                           disturb_times, impulse, warm, st, vi, tc, tz)
    torch.cuda.synchronize()
    return dict(traj_com=tc.cpu().numpy(), traj_zmp=tz.cpu().numpy(), status=st.cpu().numpy(), viol=vi.cpu().numpy(),
                com=com.cpu().numpy(), zmp=z.cpu().numpy())


def _scenario(n, seed=3):
    """n random timelines, standing at the origin at t = 0; a push of 0.05 m/s at t = 1 (cycle 200 of 400)."""
    tl = fx.make_zmp_timelines(n, seed=seed)
    return tl, timeline_knots(tl), np.zeros((n, 2)), np.zeros((n, 2)), np.zeros((n, 2))


@functools.lru_cache(maxsize=None)
def _host_reference(N):
    tl, knots, pos, vel, zmp = _scenario(4)
    assert tl["swing_start"].min() < 2.0  # a swing boundary lies inside the 400 cycles
    return _host_loop(N, tl, knots, pos, vel, zmp, 0.0, 400, (1.0,), 0.05)


def test_first_cycle_is_plan_batch_device():
    """cycles = 1, cold: the planned ZMP equals plan_batch_device on the host-sampled references of the same instant.
    The limit sampler is restated for the LDS slice, not shared, and the polyline is interpolated on the device, so the
    issue's bound for that case, 1e-12, is what is asserted; measured on the MI355X the two are bit for bit equal."""
    import torch

    n, N, t0 = 8, 100, 0.25
    rng = np.random.default_rng(1)
    tl, knots, _, _, _ = _scenario(n, seed=4)
    pos, vel = rng.uniform(-0.02, 0.02, (n, 2)), rng.uniform(-0.05, 0.05, (n, 2))
    mpc = _mpc(N)
    r = _device_loop(mpc, tl, knots, pos, vel, pos, t0, 1, warm=False)
    ref, _ = _sample(tl, knots, t0, N)
    init = np.stack([pos + math.sqrt(H / fx.G) * vel, pos], axis=2)
    z = torch.zeros((n, 2), dtype=torch.float64, device="cuda:0")
    mpc.plan_batch_device(torch.from_numpy(init).cuda(), torch.from_numpy(ref).cuda(), SIM_DT, z)
    torch.cuda.synchronize()
    diff = np.abs(r["traj_zmp"][0] - z.cpu().numpy()).max()
    print("first cycle against plan_batch_device: max |diff| = %.3e" % diff)
    assert np.all((r["status"] & 0xff) == 0) and diff <= 1e-12
    assert np.array_equal(r["zmp"], r["traj_zmp"][0]) and np.array_equal(r["traj_com"][0], pos)


@pytest.mark.parametrize("warm", [0, 1])
@pytest.mark.parametrize("N", [20, 64, 100, 127])
def test_trajectory_against_host_loop(N, warm):
    """N = 20: first rows only; 64: a full first row, no second; 100: a partial second row; 127: the limit."""
    tl, knots, pos, vel, zmp = _scenario(4)
    h = _host_reference(N)
    r = _device_loop(_mpc(N), tl, knots, pos, vel, zmp, 0.0, 400, (1.0,), 0.05, warm)
    dz, dc = np.abs(r["traj_zmp"] - h["traj_zmp"]).max(), np.abs(r["traj_com"] - h["traj_com"]).max()
    print("N = %d warm = %d: max |zmp diff| = %.3e, max |com diff| = %.3e, solves = %d"
          % (N, warm, dz, dc, (r["status"] >> 8).sum()))
    assert np.all(h["status"] == 0) and np.all((r["status"] & 0xff) == _lib.CCC_STATUS_SOLVED)
    assert dz <= BOUND and dc <= BOUND
    assert np.array_equal(r["viol"], h["viol"])


def test_warm_equals_cold():
    """The QP is strictly convex: the start does not change the minimiser, only the work (printed, not asserted)."""
    tl, knots, pos, vel, zmp = _scenario(4)
    w, c = (_device_loop(_mpc(100), tl, knots, pos, vel, zmp, 0.0, 400, (1.0,), 0.05, warm) for warm in (1, 0))
    print("tridiagonal solves over 400 cycles x 8 axes: warm %d, cold %d" % ((w["status"] >> 8).sum(), (c["status"] >> 8).sum()))
    assert np.all((w["status"] & 0xff) == 0) and np.all((c["status"] & 0xff) == 0)
    assert np.abs(w["traj_zmp"] - c["traj_zmp"]).max() <= BOUND and np.abs(w["traj_com"] - c["traj_com"]).max() <= BOUND


def test_uncatchable_push_stops_one_axis():
    """Instance 3 starts with a sideways push the ZMP cannot catch; the push is the first of a short list at which the
    host loop's oracle gives up at some cycle c (on the CPU: the yardstick alone decides c and the axis)."""
    N, cycles = 100, 40
    tl, knots, pos, vel, zmp = _scenario(4)
    for push in (0.2, 0.4, 0.8, 1.6):
        vel[3] = (0.0, push)
        h = _host_loop(N, tl, knots, pos, vel, zmp, 0.0, cycles, (), 0.0)
        if h["status"][3].any():
            break
    assert h["status"][3, 1] != 0 and not h["status"][:3].any()
    c = int(h["status"][3, 1]) >> 8
    mpc = _mpc(N)
    r = _device_loop(mpc, tl, knots, pos, vel, zmp, 0.0, cycles)
    assert r["status"][3, 1] == (c << 8) | _lib.CCC_STATUS_INFEASIBLE
    assert np.all(np.isnan(r["traj_zmp"][c:, 3, 1])) and np.all(np.isnan(r["traj_com"][c:, 3, 1]))
    assert not np.isnan(r["traj_zmp"][:c, 3, 1]).any() and not np.isnan(r["traj_zmp"][:, 3, 0]).any()
    first3 = {k: v[:3] for k, v in tl.items()}
    g = _device_loop(mpc, first3, tuple(a[:3] for a in knots), pos[:3], vel[:3], zmp[:3], 0.0, cycles)
    for key in ("traj_zmp", "traj_com"):
        assert np.array_equal(r[key][:, :3], g[key])
    assert np.array_equal(r["status"][:3], g["status"]) and np.array_equal(r["com"][:3], g["com"])


def test_refusals():
    tl, knots, pos, vel, zmp = _scenario(2)
    code = lambda e: e.value.code  # noqa: E731
    with pytest.raises(_lib.CccError) as e:  # 128 steps: beyond the tridiagonal kernel
        _device_loop(_mpc(128), tl, knots, pos, vel, zmp, 0.0, 1)
    assert code(e) == _lib.CCC_ERR_UNSUPPORTED
    many = fx.make_zmp_timelines(2, num_footsteps=17)
    with pytest.raises(_lib.CccError) as e:  # 17 footsteps: more than the LDS slice holds
        _device_loop(_mpc(20), many, knots, pos, vel, zmp, 0.0, 1)
    assert code(e) == _lib.CCC_ERR_UNSUPPORTED
    with pytest.raises(_lib.CccError) as e:  # 11 footsteps make 34 knots or more > CCC_PVZ_MAX_KNOTS
        timeline_knots(fx.make_zmp_timelines(2, num_footsteps=11))
    assert code(e) == _lib.CCC_ERR_UNSUPPORTED
    mpc = _mpc(20)
    r = _device_loop(mpc, tl, knots, pos + 0.01, vel, zmp, 0.0, 0)  # cycles = 0: nothing happens
    assert np.array_equal(r["com"][:, :, 0], pos + 0.01) and not r["status"].any()
    for cycles, sim_dt in ((-1, SIM_DT), (1, 0.0), (1, SIM_DT)):  # cycles < 0, sim_dt <= 0, null pointers
        rc = mpc._L.ccc_ism_closed_loop_device(mpc._h, 2, 0, *[None] * 11, 0.0, sim_dt, cycles, 0, None, 0.0, 1, *[None] * 5)
        assert rc == _lib.CCC_ERR_INVALID_ARGUMENT
