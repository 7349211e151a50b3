"""CCC::PreviewControlZmp and CCC::SingularPreviewControlZmp restated in numpy as the reference writes them
(include/CCC/PreviewControl.h:93-171, src/PreviewControlZmp.cpp:31-49, src/SingularPreviewControlZmp.cpp:23-57), in
np.longdouble by default (the reference of tests/test_preview_zmp_gpu.py) or, with T=np.float64, in plain double (what
float64 delivers).  Also the suffix-table formula of the knot kernel (csrc/preview_zmp.h), for measuring its error."""
import numpy as np

LD = np.longdouble
G = "9.80665"  # include/CCC/Constants.h:10


def _inv3(m):
    c = np.empty_like(m)
    for i in range(3):
        for j in range(3):  # cofactor of (j, i)
            c[i, j] = (m[(j + 1) % 3, (i + 1) % 3] * m[(j + 2) % 3, (i + 2) % 3]
                       - m[(j + 1) % 3, (i + 2) % 3] * m[(j + 2) % 3, (i + 1) % 3])
    return c / (m[0] @ c[:, 0])


def _fro(m):
    return np.sqrt((m * m).sum())


def preview_gains(com_height, dt, N, w_zmp=1.0, w_jerk=1e-8, T=LD):
    """PreviewControl<3,1,1>::calcGain for ComZmpModelJerkInput: (K [3], F [N], riccati_error, C(0,2))."""
    dt, Q, R = T(dt), T(w_zmp), T(w_jerk)
    A = np.array([[1, dt, dt * dt / 2], [0, 1, dt], [0, 0, 1]], T)
    B = np.array([dt ** 3 / 6, dt * dt / 2, dt], T)
    C = np.array([1, 0, -T(com_height) / T(G)], T)
    eye = np.eye(3, dtype=T)
    A0, G0, H0 = A, np.outer(B, B) / R, np.outer(C, C) * Q
    CtQC = H0
    for _ in range(10000):  # :121-143
        W = _inv3(eye + G0 @ H0)
        A1, G1, H1 = A0 @ W @ A0, G0 + A0 @ W @ G0 @ A0.T, H0 + A0.T @ H0 @ W @ A0
        if _fro(H1 - H0) / _fro(H1) < T("1e-8"):
            break
        A0, G0, H0 = A1, G1, H1
    P = H1
    rinv = 1 / (R + B @ P @ B)
    K = rinv * (B @ P @ A)
    err = _fro(P - (A.T @ P @ A + CtQC - np.outer(A.T @ P @ B, B @ P @ A) * rinv))
    F, fSub, ABKt = np.zeros(N, T), eye, (A - np.outer(B, K)).T
    for i in range(N):
        F[i] = rinv * (B @ fSub @ C) * Q if i < N - 1 else rinv * (B @ fSub @ P @ C)
        fSub = fSub @ ABKt
    return K, F, err, C[2]


def singular_gain(com_height, dt, T=LD):
    """(omega, K [3]) of src/SingularPreviewControlZmp.cpp:32-34."""
    dt, omega = T(dt), np.sqrt(T(G) / T(com_height))
    return omega, np.array([(1 + omega * dt) / dt + omega / (1 + omega * dt), -(2 + omega * dt) / dt,
                            -(2 + omega * dt) / (omega * dt)], T)


def singular_feedforward(omega, dt, ref, T=LD):
    """u_ff of src/SingularPreviewControlZmp.cpp:39-47 by its backward recursion; ref [..., N] (leading axes are batched)."""
    ref, dt = np.asarray(ref, T), T(dt)
    S0 = ref[..., -1] * (1 + omega * dt) / (omega * dt)
    for i in range(ref.shape[-1] - 2, 0, -1):
        S0 = ref[..., i] + S0 / (1 + omega * dt)
    return ref[..., 0] / dt - omega * (2 + omega * dt) * S0 / (1 + omega * dt) ** 2


def epilogue(kind, x, u, control_dt, dt, c02):
    """The planned ZMP from the input u (PreviewControlZmp.cpp:40-46 / SingularPreviewControlZmp.cpp:54); x [..., 3]."""
    if kind == 0:
        cd = dt if control_dt < 0 else control_dt
        return x[..., 0] + cd * x[..., 1] + cd * cd / 2 * x[..., 2] + c02 * (x[..., 2] + cd * u)
    return x[..., 0] + control_dt * u


def knot_samples(knot_time, knot_zmp, t, T=LD):
    """The linear interpolation of the knots at the sample times t [N] (float64, as the caller computed them): sample i
    lies in segment s iff knot_time[s] <= t[i] < knot_time[s + 1].  Returns (ref [2, N] in T, segment index [N])."""
    s = np.searchsorted(knot_time, t, side="right") - 1
    ta, tb, za, zb = (np.asarray(a, T) for a in (knot_time[s], knot_time[s + 1], knot_zmp[s], knot_zmp[s + 1]))
    return (za + ((np.asarray(t, T) - ta) / (tb - ta))[:, None] * (zb - za)).T, s


def knot_sum_tables(w, knot_time, knot_zmp, seg, ct, off, dt):
    """sum_i w_i r_i [2] by the knot kernel's formula in float64: suffix tables (accumulated in longdouble, rounded once)
    and, per segment with samples [lo, hi), alpha (W0[lo] - W0[hi]) + beta (W1[lo] - W1[hi])."""
    N = len(w)
    W0 = np.concatenate([np.cumsum(np.asarray(w, LD)[::-1])[::-1], [0]]).astype(np.float64)
    W1 = np.concatenate([np.cumsum((np.arange(N) * np.asarray(w, LD))[::-1])[::-1], [0]]).astype(np.float64)
    total = np.zeros(2)
    for s in np.unique(seg):
        lo, hi = np.searchsorted(seg, s, "left"), np.searchsorted(seg, s, "right")
        m = (knot_zmp[s + 1] - knot_zmp[s]) * (1.0 / (knot_time[s + 1] - knot_time[s]))
        total += (knot_zmp[s] + (ct + off * dt - knot_time[s]) * m) * (W0[lo] - W0[hi]) + (dt * m) * (W1[lo] - W1[hi])
    return total
