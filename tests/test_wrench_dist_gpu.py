"""ccc_wrench_distribution_device and the fused CCC::PreviewControlCentroidal entry (csrc/wrench_dist.hip) against a
plain np.longdouble reference: a single-change primal active set on the dense H = G' diag(ww) G + rho I from all-at-lo."""
import numpy as np
import pytest

from centroidalcontrolcollection_amd import fixtures_ddp as fx

LD = np.longdouble
N_INST = 67  # the last wavefront and the last group of rows are partial
MASS, INERTIA = 100.0, (40.0, 20.0, 10.0)


def gmat(vertex, ridge, origin, m):
    return np.vstack([np.cross(vertex[:m] - origin, ridge[:m]).T, ridge[:m].T]).astype(LD)


def ref_distribute(G, w, ww, rho, lo, hi):
    """Returns s (longdouble).  Primal active set, one change per step, from s = lo."""
    m = G.shape[1]
    if m == 0:
        return np.zeros(0, LD)
    H = G.T @ (np.asarray(ww, LD)[:, None] * G) + LD(rho) * np.eye(m, dtype=LD)
    q = -G.T @ (np.asarray(ww, LD) * np.asarray(w, LD))
    s, state = np.full(m, LD(lo)), np.ones(m, int)  # 0 free, 1 at lo, 2 at hi
    for _ in range(50 * m + 50):
        F = np.flatnonzero(state == 0)
        t = s.copy()
        if len(F):
            B = np.flatnonzero(state != 0)
            rhs = -(q[F] + H[np.ix_(F, B)] @ s[B])
            t[F] = np.linalg.solve(H[np.ix_(F, F)].astype(np.float64), rhs.astype(np.float64)).astype(LD)
            for _k in range(3):  # refinement in extended precision
                res = rhs - H[np.ix_(F, F)] @ t[F]
                t[F] += np.linalg.solve(H[np.ix_(F, F)].astype(np.float64), res.astype(np.float64)).astype(LD)
        d = t - s
        alpha, blk = LD(1), -1
        for r in F:
            if t[r] < lo and (lo - s[r]) / d[r] < alpha:
                alpha, blk = (lo - s[r]) / d[r], r
            if t[r] > hi and (hi - s[r]) / d[r] < alpha:
                alpha, blk = (hi - s[r]) / d[r], r
        s = s + alpha * d
        if blk >= 0:
            state[blk] = 1 if t[blk] < lo else 2
            s[blk] = lo if t[blk] < lo else hi
            continue
        grad = H @ s + q
        viol = np.where(state == 1, -grad, np.where(state == 2, grad, -1.0))
        r = int(np.argmax(viol))
        if viol[r] <= 1e-13 * (1 + np.abs(q).max()):
            return s
        state[r] = 0
    raise AssertionError("the reference did not terminate")


def foot(x=0.0, y=0.0):
    return fx.contact_from_rect((x - 0.1, y - 0.1), (x + 0.1, y + 0.1))


def contacts(M):
    if M == 16:
        parts = [foot()]
    elif M == 32:
        parts = [foot(0.0, 0.15), foot(0.1, -0.15)]
    else:
        parts = [foot(0.0, 0.15), foot(0.1, -0.15), fx.contact_from_pose((0.4, 0.3, 1.0), (-1, 0, 0.2), (0, 1, 0)),
                 fx.contact_from_pose((0.4, -0.3, 1.1), (-1, 0.1, 0), (0, 0, 1))]
    return np.concatenate([p[0] for p in parts]), np.concatenate([p[1] for p in parts])


def make_batch(M, dim, seed=20251126):
    rng = np.random.default_rng(seed)
    V, R = contacts(M)
    n = N_INST
    vertex, ridge = np.tile(V, (n, 1, 1)), np.tile(R, (n, 1, 1))
    dims = np.full(n, dim, np.int32) if np.isscalar(dim) else np.asarray(dim, np.int32)
    origin = np.array([0.0, 0.0, 1.0]) + 0.05 * rng.standard_normal((n, 3))
    w = np.zeros((n, 6))
    w[:, 5] = MASS * fx.G
    w += rng.standard_normal((n, 6)) * np.array([40.0, 40.0, 40.0, 150.0, 150.0, 100.0])
    return dims, vertex, ridge, origin, w


def check_distribution(dims, vertex, ridge, origin, w, wrench, scales, status, lo, hi, rho, compare_s=False):
    ww = np.ones(6)
    iters = status >> 8
    print("iterations: mean %.2f max %d" % (iters.mean(), iters.max()))
    assert (status & 0xff == 0).all(), status[status & 0xff != 0]
    for k in range(len(dims)):
        m = int(dims[k])
        s = scales[k, :m]
        assert (scales[k, m:] == 0).all() and (s >= lo).all() and (s <= hi).all()
        mom, f = fx.total_wrench(vertex[k], ridge[k], s, origin[k])
        own = np.concatenate([mom, f])
        assert np.abs(wrench[k] - own).max() <= 1e-12 * (1 + np.abs(own).max())
        G = gmat(vertex[k], ridge[k], origin[k], m)
        s_ref = ref_distribute(G, w[k], ww, rho, lo, hi)
        err = np.abs(G @ s.astype(LD) - G @ s_ref).max() if m else np.abs(wrench[k]).max()
        assert err <= 1e-9 * (1 + np.abs(w[k]).max()), (k, float(err))
        if compare_s:
            assert np.abs(s - s_ref).max() <= 1e-9 * hi, k


CASES = [
    pytest.param(16, 16, 3.0, 1000.0, 1e-8, id="M16-base"),
    pytest.param(16, 16, 3.0, 40.0, 1e-8, id="M16-all-at-hi"),
    pytest.param(16, 8, 3.0, 1000.0, 1e-8, id="M16-two-vertices"),
    pytest.param(16, "some-zero", 3.0, 1000.0, 1e-8, id="M16-no-contact-rows"),
    pytest.param(32, 32, 3.0, 1000.0, 1e-8, id="M32-base"),
    pytest.param(32, 32, 3.0, 40.0, 1e-8, id="M32-mixed"),
    pytest.param(64, 64, 3.0, 1000.0, 1e-8, id="M64-base"),
    pytest.param(16, 16, 3.0, 1000.0, 1e-2, id="M16-rho1e-2-compare-s"),
]


@pytest.mark.gpu
@pytest.mark.parametrize("M,dim,lo,hi,rho", CASES)
def test_distribution_against_reference(M, dim, lo, hi, rho):
    import torch

    from centroidalcontrolcollection_amd import wrench as wmod

    if dim == "some-zero":
        dim = np.where(np.arange(N_INST) % 3 == 1, 0, 16)
    dims, vertex, ridge, origin, w = make_batch(M, dim)
    dev = torch.device("cuda")
    t = lambda a: torch.as_tensor(a, device=dev)
    cfg = wmod.WrenchDistConfig(regular_weight=rho, ridge_force_min=lo, ridge_force_max=hi)
    wrench, scales, status = wmod.wrench_distribution_device(t(dims), t(vertex), t(ridge), t(w), t(origin), cfg)
    torch.cuda.synchronize()
    check_distribution(dims, vertex, ridge, origin, w, wrench.cpu().numpy(), scales.cpu().numpy(), status.cpu().numpy(),
                       lo, hi, rho, compare_s=rho == 1e-2)


def ref_gains(inertia, dt, N, q, R):
    """PreviewControl::calcGain (doubling iteration, the reference's stopping rule) in longdouble: K [3], F [2N]."""
    dt, R = LD(dt), LD(R)
    A = np.eye(3, dtype=LD)
    A[0, 1] = A[1, 2] = dt
    A[0, 2] = dt * dt / 2
    B = np.array([[dt ** 3 / 6], [dt * dt / 2], [dt]], LD)
    C = np.array([[1, 0, 0], [0, 0, inertia]], LD)
    Q = np.diag(np.asarray(q, LD))

    def inv(X):
        Y = np.linalg.inv(X.astype(np.float64)).astype(LD)
        for _ in range(3):
            Y = Y + Y @ (np.eye(3, dtype=LD) - X @ Y)
        return Y

    A0, G0, H0 = A, B @ B.T / R, C.T @ Q @ C
    for _ in range(10000):
        Ii = inv(np.eye(3, dtype=LD) + G0 @ H0)
        A1, G1, H1 = A0 @ Ii @ A0, G0 + A0 @ Ii @ G0 @ A0.T, H0 + A0.T @ H0 @ Ii @ A0
        if np.sqrt(((H1 - H0) ** 2).sum()) / np.sqrt((H1 ** 2).sum()) < 1e-8:
            break
        A0, G0, H0 = A1, G1, H1
    P = H1
    rinv = 1 / (R + (B.T @ P @ B)[0, 0])
    K = rinv * (B.T @ P @ A)[0]
    ABKt, fsub, F = (A - B @ K[None]).T, np.eye(3, dtype=LD), np.zeros(2 * N, LD)
    for i in range(N):
        F[2 * i:2 * i + 2] = rinv * (B.T @ fsub @ (C.T @ Q if i < N - 1 else P @ C.T))[0]
        fsub = fsub @ ABKt
    return K, F


@pytest.fixture(scope="module")
def pcc_reference_gains():
    out = {}
    for N in (5, 200):
        K, F = np.zeros((6, 3), LD), np.zeros((6, 2 * N), LD)
        for a in range(6):
            K[a], F[a] = ref_gains(INERTIA[a] if a < 3 else MASS, 0.01, N, (1e2, 5e-3) if a < 3 else (2e2, 5e-4), 1e-8)
        out[N] = (K, F)
    return out


@pytest.mark.gpu
def test_gains_against_longdouble(pcc_reference_gains):
    from centroidalcontrolcollection_amd import PreviewControlCentroidal

    pc = PreviewControlCentroidal(MASS, INERTIA, 2.0, 0.01)
    assert pc.horizon_steps_ == 200
    K, F, err = pc.gains()
    Kr, Fr = pcc_reference_gains[200]
    assert np.isfinite(err).all()
    for a in range(6):
        assert np.abs(K[a] - Kr[a]).max() <= 1e-9 * np.abs(Kr[a]).max()
        assert np.abs(F[a] - Fr[a]).max() <= 1e-9 * np.abs(Fr[a]).max()


@pytest.mark.gpu
@pytest.mark.parametrize("N", [5, 200])
@pytest.mark.parametrize("M", [16, 32])
def test_fused_plan(pcc_reference_gains, N, M):
    from centroidalcontrolcollection_amd import PreviewControlCentroidal

    pc = PreviewControlCentroidal(MASS, INERTIA, N * 0.01, 0.01, max_ridges=M)
    assert pc.horizon_steps_ == N
    dims, vertex, ridge, origin, _ = make_batch(M, M)
    rng = np.random.default_rng(7)
    n = N_INST
    x0 = 0.05 * rng.standard_normal((n, 18))
    x0[:, 3:6] = origin
    ref = np.zeros((n, N, 12))
    ref[:, :, 3:6] = origin[:, None, :] + 0.02 * rng.standard_normal((n, N, 3))
    ref[:, :, 0:3] = 0.02 * rng.standard_normal((n, N, 3))
    ref[:, :, 6:12] = 5.0 * rng.standard_normal((n, N, 6))
    out = pc.planOnceBatch(x0, ref, dims, vertex, ridge, control_dt=0.01)
    again = pc.planOnceBatch(x0, ref, dims, vertex, ridge, control_dt=-1.0)
    assert np.array_equal(out["wrench"], again["wrench"]) and np.array_equal(out["planned_wrench"], again["planned_wrench"])
    K, F = pcc_reference_gains[N]
    planned = np.zeros((n, 6), LD)
    for a in range(6):
        seq = np.stack([ref[:, :, a], ref[:, :, 6 + a]], axis=2).reshape(n, 2 * N).astype(LD)
        x = np.stack([x0[:, a], x0[:, 6 + a], x0[:, 12 + a]], axis=1).astype(LD)
        jerk = -(x @ K[a]) + seq @ F[a]
        planned[:, a] = (INERTIA[a] if a < 3 else MASS) * (x[:, 2] + LD(0.01) * jerk)
    planned[:, 5] += LD(MASS) * LD(fx.G)
    scale = 1 + np.abs(planned).max(axis=1)
    assert (np.abs(out["planned_wrench"] - planned).max(axis=1) <= 1e-9 * scale).all()
    check_distribution(dims, vertex, ridge, origin, out["planned_wrench"], out["wrench"], out["scales"],
                       out["status_raw"], 3.0, 1000.0, 1e-8)


@pytest.mark.gpu
def test_closed_loop_reference_scenario():
    """tests/src/TestPreviewControlCentroidal.cpp as written (three contact phases, the kick at 1 s, 600 cycles at
    sim_dt 0.005), eight instances with perturbed start positions."""
    from centroidalcontrolcollection_amd import PreviewControlCentroidal

    n, N, dt, sim_dt = 8, 200, 0.01, 0.005
    pc = PreviewControlCentroidal(MASS, INERTIA, 2.0, dt)
    rects = [((-0.1, -0.1), (0.1, 0.1)), ((0.15, 0.15), (0.35, 0.35)), ((0.4, -0.1), (0.6, 0.1))]
    ref_pos = np.array([[0.0, 0.0, 1.0], [0.25, 0.0, 1.2], [0.5, 0.0, 1.0]])
    phase = lambda t: np.where(t + 1e-6 < 1.4, 0, np.where(t + 1e-6 < 1.6, 1, 2))
    cont = [fx.contact_from_rect(*r) for r in rects]
    rng = np.random.default_rng(3)
    sims = [fx.CentroidalSim(MASS, INERTIA, sim_dt) for _ in range(n)]
    for sim in sims:
        sim.pos = ref_pos[0] + 0.01 * rng.standard_normal(3)
    planned = np.tile(np.array([0, 0, 0, 0, 0, MASS * fx.G]), (n, 1))
    t, dims = 0.0, np.full(n, 16, np.int32)
    while t < 3.0:
        x0 = np.zeros((n, 18))
        for k, sim in enumerate(sims):
            x0[k, 0:3], x0[k, 3:6], x0[k, 6:9], x0[k, 9:12] = sim.ori, sim.pos, sim.ang_vel, sim.vel
        x0[:, 12:15] = planned[:, 0:3] / np.asarray(INERTIA)
        x0[:, 15:18] = planned[:, 3:6] / MASS - np.array([0, 0, fx.G])
        ref = np.zeros((n, N, 12))
        ref[:, :, 3:6] = ref_pos[phase(t + (np.arange(N) + 1) * dt)]
        V, R = cont[int(phase(np.float64(t)))]
        planned = pc.planOnceBatch(x0, ref, dims, np.tile(V, (n, 1, 1)), np.tile(R, (n, 1, 1)), control_dt=sim_dt)["wrench"]
        now = ref_pos[int(phase(np.float64(t)))]
        for k, sim in enumerate(sims):
            assert np.linalg.norm(np.concatenate([sim.ori, sim.pos - now])) < 2.0
            assert np.linalg.norm(np.concatenate([sim.ang_vel, sim.vel])) < 2.0
            sim.update(planned[k, 3:6], planned[k, 0:3])
        t += sim_dt
        if 1.0 <= t < 1.0 + sim_dt:
            for sim in sims:
                sim.addDisturb((0.05, 0.05, 0.0), (0.0, 0.0, 0.0))
    end = ref_pos[int(phase(np.float64(t)))]
    for sim in sims:
        assert np.linalg.norm(np.concatenate([sim.ori, sim.pos - end])) < 0.1
        assert np.linalg.norm(np.concatenate([sim.ang_vel, sim.vel])) < 0.1
