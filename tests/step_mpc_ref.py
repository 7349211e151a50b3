"""References for the StepMpc tests (plain module, not a test).

plan_exact  -- StepMpc1d::planOnce (/root/reference/src/StepMpc.cpp:8-200) restated literally in mpmath at 60 digits from
               the raw float64 inputs: Ad_, Bd_, C_ of StepModel, the sequential extension with outputs, eq_mat, eq_vec,
               an exact solve.  THE reference.
plan_lstsq  -- the same least-squares rows (eq_mat = J'J, eq_vec = -J'r) in numpy float64, solved by numpy.linalg.lstsq:
               what float64 can deliver on the problem, the yardstick of the kernel's error bound.
Both take one axis: flags [n] (is_single_support), zmp [n], end_time [n], (pos, vel), current_time, com_height and the
weights (free_zmp, fixed_zmp, double_support, pos, vel, capture_point_abs, capture_point_rel), and return
(current_zmp, next_foot_zmp or None).
"""
import math

import mpmath
import numpy as np

G = 9.80665
DEFAULT_WEIGHTS = (1e-2, 1e0, 1e0, 0.0, 0.0, 1e1, 1e1)


def _next_foot(flags):
    for i in range(1, len(flags)):
        if flags[i]:
            return i
    return None


def plan_exact(flags, zmp, end_time, x0, current_time, com_height, weights=DEFAULT_WEIGHTS):
    mp = mpmath.mp
    old = mp.dps
    mp.dps = 60
    try:
        f = mpmath.mpf
        n = len(flags)
        w_free, w_fixed, w_ds, w_pos, w_vel, w_cpa, w_cpr = (f(float(v)) for v in weights)
        omega = mpmath.sqrt(f(G) / f(float(com_height)))
        # StepModel (:8-24) and VariantSequentialExtension(model_list, true): output block i = C x_{i+1}
        C = mpmath.matrix([[1, 0], [0, 1], [1, 1 / omega]])
        A_seq = mpmath.zeros(3 * n, 2)
        B_seq = mpmath.zeros(3 * n, n)
        Phi = mpmath.eye(2)
        cols = []  # d x_{i+1} / d u_j
        for i in range(n):
            T = f(float(end_time[i])) - (f(float(current_time)) if i == 0 else f(float(end_time[i - 1])))
            e = mpmath.exp(omega * T)
            ei = 1 / e
            Ad = mpmath.matrix([[(e + ei) / 2, (e - ei) / 2 / omega], [omega * (e - ei) / 2, (e + ei) / 2]])
            Bd = mpmath.matrix([[1 - (e + ei) / 2], [omega * (ei - e) / 2]])
            Phi = Ad * Phi
            cols = [Ad * c for c in cols] + [Bd]
            A_seq[3 * i:3 * i + 3, :] = C * Phi
            for j, c in enumerate(cols):
                B_seq[3 * i:3 * i + 3, j] = C * c
        x0v = mpmath.matrix([f(float(x0[0])), f(float(x0[1]))])
        ref = [f(float(z)) for z in zmp]
        eq_mat = mpmath.zeros(n, n)
        eq_vec = mpmath.zeros(n, 1)

        def add(rows, targets, w):
            # eq_mat += w S'S, eq_vec += w S'(free - target) for the selected output rows S (a list of row vectors)
            for row, free, tgt in zip(rows, targets[0], targets[1]):
                for p in range(n):
                    if row[p] == 0:
                        continue
                    eq_vec[p] += w * row[p] * (free - tgt)
                    for q in range(n):
                        eq_mat[p, q] += w * row[p] * row[q]

        # ZMP (:51-64)
        diag = [w_free] * n
        diag[0] = w_fixed
        if n > 1 and not flags[0]:
            diag[1] = w_fixed
        for i in range(n):
            eq_mat[i, i] += diag[i]
            eq_vec[i] += -diag[i] * ref[i]
        # double support (:66-80)
        ds = [1, -2, 1]
        for i in range(1, n - 1):
            if flags[i - 1] and not flags[i] and flags[i + 1]:
                for p in range(3):
                    for q in range(3):
                        eq_mat[i - 1 + p, i - 1 + q] += w_ds * ds[p] * ds[q]
        free = A_seq * x0v
        brow = lambda r: [B_seq[r, j] for j in range(n)]  # noqa: E731
        # position (:82-95), velocity (:97-109)
        if w_pos > 0:
            add([brow(3 * i) for i in range(n)], ([free[3 * i] for i in range(n)], [ref[min(i + 1, n - 1)] for i in range(n)]),
                w_pos)
        if w_vel > 0:
            add([brow(3 * i + 1) for i in range(n)], ([free[3 * i + 1] for i in range(n)], [0] * n), w_vel)
        future = sum(1 for i in range(1, n) if flags[i])
        # capture point, absolute (:111-150)
        if w_cpa > 0:
            if future == 0:
                sel = [(i, i) for i in range(n) if i >= 1 or not flags[i]]
            else:
                sel = [(i, i - 1) for i in range(1, n) if flags[i]]
            add([brow(3 * k + 2) for _, k in sel], ([free[3 * k + 2] for _, k in sel], [ref[i] for i, _ in sel]), w_cpa)
        # capture point relative to the ZMP (:152-180)
        if w_cpr > 0 and future >= 1:
            rows, frees = [], []
            for i in range(1, n):
                if flags[i]:
                    r = brow(3 * (i - 1) + 2)
                    r[i] -= 1
                    rows.append(r)
                    frees.append(free[3 * (i - 1) + 2])
            add(rows, (frees, [0] * len(rows)), w_cpr)
        sol = mpmath.lu_solve(eq_mat, -eq_vec)
        k = _next_foot(flags)
        return float(sol[0]), (None if k is None else float(sol[k]))
    finally:
        mp.dps = old


def rows_float64(flags, zmp, end_time, x0, current_time, com_height, weights=DEFAULT_WEIGHTS):
    """(J [m,n], r [m]) with eq_mat = J'J and eq_vec = -J'r, in float64, in the modal coordinates xi = x + v / w,
    zeta = x - v / w of the step-to-step map."""
    n = len(flags)
    s_free, s_fixed, s_ds, s_pos, s_vel, s_cpa, s_cpr = (math.sqrt(v) for v in weights)
    omega = math.sqrt(G / com_height)
    J, r = [], []

    def row(coef, rhs):
        J.append(coef)
        r.append(rhs)

    for i in range(n):
        c = np.zeros(n)
        c[i] = s_fixed if i == 0 or (i == 1 and n > 1 and not flags[0]) else s_free
        row(c, c[i] * zmp[i])
    future = any(flags[1:])
    a, b = np.zeros(n), np.zeros(n)
    xi, zeta = x0[0] + x0[1] / omega, x0[0] - x0[1] / omega
    for i in range(n):
        if s_ds > 0 and 2 <= i and flags[i - 2] and not flags[i - 1] and flags[i]:
            c = np.zeros(n)
            c[i - 2:i + 1] = [s_ds, -2 * s_ds, s_ds]
            row(c, 0.0)
        if i >= 1 and flags[i] and future:
            if s_cpa > 0:
                row(s_cpa * a, s_cpa * (zmp[i] - xi))
            if s_cpr > 0:
                c = a.copy()
                c[i] -= 1.0
                row(s_cpr * c, -s_cpr * xi)
        wt = omega * (end_time[i] - (current_time if i == 0 else end_time[i - 1]))
        em, en = math.expm1(wt), math.expm1(-wt)
        a, b = a * (1.0 + em), b * (1.0 + en)
        a[i], b[i] = -em, -en
        xi, zeta = xi * (1.0 + em), zeta * (1.0 + en)
        if s_pos > 0:
            row(s_pos * (0.5 * (a + b)), s_pos * (zmp[min(i + 1, n - 1)] - 0.5 * (xi + zeta)))
        if s_vel > 0:
            row(s_vel * 0.5 * omega * (a - b), -s_vel * 0.5 * omega * (xi - zeta))
        if s_cpa > 0 and not future and (i >= 1 or not flags[0]):
            row(s_cpa * a, s_cpa * (zmp[i] - xi))
    return np.array(J), np.array(r)


def plan_lstsq(flags, zmp, end_time, x0, current_time, com_height, weights=DEFAULT_WEIGHTS):
    J, r = rows_float64(flags, zmp, end_time, x0, current_time, com_height, weights)
    sol = np.linalg.lstsq(J, r, rcond=None)[0]
    k = _next_foot(flags)
    return float(sol[0]), (None if k is None else float(sol[k]))
