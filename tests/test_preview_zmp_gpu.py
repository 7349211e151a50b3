"""CCC::PreviewControlZmp and CCC::SingularPreviewControlZmp on the device (csrc/preview_zmp.hip) against
tests/preview_zmp_ref.py (the reference's planOnce paths in np.longdouble).

The sampled kernel is held to a derived bound: a sum of N products in any order is within (N + 8) 2^-53 (sum |w_i r_i| +
sum |K_j x_j|) |dzmp/du| + 4 2^-53 |zmp| of the exact value for the same K and w.  The knot kernel's prefix differences
have another error constant, so its bound is measured: 8 max(e64, 2^-53 scale), e64 being the error of the float64 numpy
restatement of the same suffix-table formula on the same inputs.  Measured on an MI355X (the printed lines of -s):
sampled, worst error / bound 0.24 (N = 1) falling to 0.006 (N = 512); knots, worst case (32 knots, singular) e64
2.12e-15 m and kernel 2.14e-15 m at a scale of 0.5 m, so 1.0 of the 8 allowed."""
import ctypes

import numpy as np
import pytest

import centroidalcontrolcollection_amd as ccc
from centroidalcontrolcollection_amd import _lib, fixtures, preview_control_zmp as pvz

import preview_zmp_ref as ref

LD, EPS = np.longdouble, 2.0 ** -53
H, DT = 1.0, 0.01
KINDS = {"preview": (ccc.PreviewControlZmp, 0, 1), "singular": (ccc.SingularPreviewControlZmp, 1, 0)}  # class, kind, off


def _make(kind, N):
    return KINDS[kind][0](H, N * DT - 0.5 * DT, DT)  # ceil((N - 1/2) dt / dt) = N


def _exact(ctl, kind, x0, refs, control_dt):
    """Longdouble plans (zmp [n,2], u [n,2]) from the handle's own K and w, and sum |w r| + sum |K x| per plan."""
    K, w, _ = ctl.gains()
    x, r = np.asarray(x0, LD), np.asarray(refs, LD)
    u = r @ w.astype(LD) - x @ K.astype(LD)
    mag = np.abs(r) @ np.abs(w).astype(LD) + np.abs(x) @ np.abs(K).astype(LD)
    return ref.epilogue(KINDS[kind][1], x, u, LD(control_dt), LD(DT), -LD(H) / LD(ref.G)), u, mag


def _dzmp_du(kind, control_dt):
    cd = DT if (control_dt < 0 and kind == "preview") else control_dt
    return abs(cd * H / 9.80665) if kind == "preview" else abs(cd)


@pytest.mark.gpu
@pytest.mark.parametrize("N", [1, 2, 3, 31, 200, 512])
@pytest.mark.parametrize("kind", sorted(KINDS))
def test_gains_against_longdouble(kind, N):
    ctl = _make(kind, N)
    assert ctl.horizon_steps_ == N
    K, w, err = ctl.gains()
    if kind == "preview":
        K_ref, w_ref, _, _ = ref.preview_gains(H, DT, N)
        assert np.isfinite(err) and err < 1e-6  # |P| ~ 1e3: the residual of a converged P
    else:
        omega, K_ref = ref.singular_gain(H, DT)
        w_ref = ref.singular_feedforward(omega, DT, np.eye(N))  # the recursion on unit vectors: its weights
        assert err == 0.0
    eK, ew = np.abs(K - K_ref).max() / np.abs(K_ref).max(), np.abs(w - w_ref).max() / np.abs(w_ref).max()
    print("%s N=%d: K rel %.2e, w rel %.2e, riccati_error %.2e" % (kind, N, eK, ew, err))
    assert eK <= 1e-9 and ew <= 1e-9


@pytest.mark.gpu
@pytest.mark.parametrize("N", [1, 2, 3, 17, 33, 200, 512])
@pytest.mark.parametrize("kind", sorted(KINDS))
def test_sampled_path_against_longdouble(kind, N):
    ctl, rng, worst = _make(kind, N), np.random.default_rng(N), 0.0
    for n in (1, 5, 203):
        refs = rng.uniform(-0.3, 0.3, (n, 2, N))
        x0 = rng.uniform(-0.3, 0.3, (n, 2, 3))
        for control_dt in (-1.0, 0.005):
            out = ctl.planOnceBatch(x0, refs, control_dt)
            exact, u, mag = _exact(ctl, kind, x0, refs, control_dt)
            bound = (N + 8) * EPS * mag * _dzmp_du(kind, control_dt) + 4 * EPS * np.abs(exact)
            worst = max(worst, float((np.abs(out["zmp"] - exact) / bound).max()))
            # (input is u itself, the CoM jerk or the ZMP velocity: the same sum without the epilogue)
            assert (np.abs(out["input"] - u) <= (N + 8) * EPS * mag + 4 * EPS * np.abs(u)).all()
    print("%s N=%d: worst error / bound %.3f" % (kind, N, worst))
    assert worst <= 1.0


def _knot_cases(off, N, rng):
    """(knot list, current_time) per case of the issue; t(i) is the sample time by the kernel's own expression."""
    cases = []
    for name in ("const2", "k16", "k17", "k32", "on_sample", "empty", "wide"):
        for _ in range(6):
            ct = float(rng.uniform(0.0, 9.0))
            t = [ct + (i + off) * DT for i in range(N)]
            if name == "const2":
                times = [t[0] - 1.0, t[-1] + 5.0]
            elif name in ("k16", "k17", "k32"):  # (random widths: at 32 knots some segments hold no sample)
                nk = int(name[1:])
                times = [t[0] - 0.05] + sorted(rng.uniform(t[0], t[-1], nk - 2)) + [t[-1] + 0.1]
            elif name == "on_sample":  # the first knot ON sample 0 (a left end); knot ON sample 37: right end and left end
                times = [t[0], t[20] + 0.3 * DT, t[37], t[90] + 0.5 * DT, t[-1] + 1e-9]
            elif name == "empty":  # three knots between samples 5 and 6
                times = [t[0] - 0.2, t[5] + 0.2 * DT, t[5] + 0.5 * DT, t[5] + 0.7 * DT, t[-1] + 0.3]
            else:  # a segment before every sample, then one wider than the horizon
                times = [t[0] - 0.5, t[0] - 0.1, t[-1] + 10.0]
            z = rng.uniform(-0.3, 0.3, (len(times), 2))
            if name == "const2":
                z[1] = z[0]
            cases.append((name, list(zip(times, z)), ct))
    return cases


@pytest.mark.gpu
@pytest.mark.parametrize("kind", sorted(KINDS))
def test_knot_path_equals_the_sampled_problem(kind):
    N, off, rng = 200, KINDS[kind][2], np.random.default_rng(3)
    ctl = _make(kind, N)
    _, w, _ = ctl.gains()
    cases = _knot_cases(off, N, rng)
    num, kt, kz = pvz.pack_knots([c[1] for c in cases])
    ct = np.array([c[2] for c in cases])
    x0 = rng.uniform(-0.3, 0.3, (len(cases), 2, 3))
    out = ctl.planOnceBatchKnots(num, kt, kz, x0, ct, 0.005)
    assert (out["status"] == _lib.CCC_STATUS_SOLVED).all()
    gain = _dzmp_du(kind, 0.005)
    for k, (name, _, _) in enumerate(cases):
        t = np.array([ct[k] + (i + off) * DT for i in range(N)])
        r, seg = ref.knot_samples(kt[k, :num[k]], kz[k, :num[k]], t)
        exact, _, mag = _exact(ctl, kind, x0[k:k + 1], r[None], 0.005)
        s64 = ref.knot_sum_tables(w, kt[k], kz[k], seg, ct[k], off, DT)
        e64 = float(np.abs(s64 - r @ w.astype(LD)).max()) * gain
        err, scale = float(np.abs(out["zmp"][k] - exact[0]).max()), float(mag.max()) * gain
        print("%s %s: e64 %.2e kernel %.2e scale %.2e" % (kind, name, e64, err, scale))
        assert err <= 8 * max(e64, EPS * scale), (name, k)


@pytest.mark.gpu
@pytest.mark.parametrize("kind", sorted(KINDS))
def test_knot_lists_that_do_not_cover_the_horizon_are_refused(kind):
    N, off = 200, KINDS[kind][2]
    ctl = _make(kind, N)
    t0, t_last = 1.0 + off * DT, 1.0 + (N - 1 + off) * DT
    good = [(t0 - 0.1, (0.0, 0.1)), (t0 + 0.7, (0.2, -0.1)), (t_last + 0.1, (0.3, 0.0))]
    lists = [list(good) for _ in range(12)]
    lists[1][2] = (t_last, (0.3, 0.0))            # ends ON the last sample: [first, last) does not hold it
    lists[4][0] = (t0 + 1e-9, (0.0, 0.1))         # starts after the first sample
    lists[6] = good[:1]                           # num_knots = 1
    lists[9][1] = (t0 - 0.1, (0.2, -0.1))         # two equal knot times
    num, kt, kz = pvz.pack_knots(lists)
    num[10] = 33
    bad = (1, 4, 6, 9, 10)
    out = ctl.planOnceBatchKnots(num, kt, kz, np.full((12, 2, 3), 0.05), np.full(12, 1.0), 0.005)
    for k in range(12):
        if k in bad:
            assert out["status"][k] == _lib.CCC_STATUS_INFEASIBLE, k
            assert np.isnan(out["zmp"][k]).all() and np.isnan(out["input"][k]).all(), k
        else:  # the neighbours in the same wavefront: the plan of the untouched list, bit for bit
            assert out["status"][k] == _lib.CCC_STATUS_SOLVED and (out["zmp"][k] == out["zmp"][0]).all(), k
    assert np.isfinite(out["zmp"][0]).all()


def test_create_refuses_bad_arguments_without_a_device():
    assert "PreviewControlZmp" in ccc.__all__ and "SingularPreviewControlZmp" in ccc.__all__
    L = _lib.load()
    pvz._bind(L)
    h = ctypes.c_void_p()
    for args in ((0, -1.0, 2.0, 0.01), (1, 0.0, 2.0, 0.01), (0, 1.0, 0.0, 0.01), (1, 1.0, 2.0, -0.01), (2, 1.0, 2.0, 0.01)):
        assert L.ccc_pvz_create(*args, 0.0, 0.0, 0, ctypes.byref(h)) == _lib.CCC_ERR_INVALID_ARGUMENT, args
    assert L.ccc_pvz_create(0, 1.0, 5.125, 0.01, 0.0, 0.0, 0, ctypes.byref(h)) == _lib.CCC_ERR_UNSUPPORTED  # N = 513
    assert L.ccc_pvz_horizon_steps(None) == -1


@pytest.mark.gpu
@pytest.mark.parametrize("kind", sorted(KINDS))
def test_closed_loop_reference_scenario(kind):
    """TestPreviewControlZmp.cpp / TestSingularPreviewControlZmp.cpp:55-105, all 10 s with both disturbances, through the
    knot entry with ref_zmp_list_ as the knots (the +1e-6 of FootstepManager::refZmp folded into current_time)."""
    ctl = KINDS[kind][0](1.0, 2.0, 0.01)
    fm = fixtures.FootstepManager()
    for fs in fixtures.reference_scenario_footsteps():
        fm.appendFootstep(fs)
    sim_dt, t = 0.005, 0.0
    sim = fixtures.ComZmpSim2d(1.0, sim_dt)
    planned = sim.pos()
    while t < 10.0:
        fm.update(t)
        if kind == "preview":
            x0 = np.stack([sim.pos(), sim.vel(), fixtures.G / 1.0 * (sim.pos() - planned)], axis=1)
        else:
            x0 = np.stack([planned, sim.pos(), sim.vel()], axis=1)
        num, kt, kz = pvz.pack_knots([list(zip(fm._zmp_times, fm._zmps))])
        out = ctl.planOnceBatchKnots(num, kt, kz, x0[None], [t + 1e-6], sim_dt)
        assert out["status"][0] == _lib.CCC_STATUS_SOLVED, t
        planned = out["zmp"][0].copy()
        assert np.linalg.norm(planned - fm.refZmp(t)) < 0.1, t
        t += sim_dt
        sim.update(planned)
        if any(d <= t < d + sim_dt for d in (4.5, 8.5)):
            sim.addDisturb((0.05, 0.05))
    ref_zmp = fm.refZmp(t)
    assert np.linalg.norm(planned - ref_zmp) < 1e-2
    assert np.linalg.norm(sim.pos() - ref_zmp) < 1e-2
    assert np.linalg.norm(sim.vel()) < 1e-2
