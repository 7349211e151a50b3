"""CPU checks of the references behind the wrench-distribution GPU tests (tests/wrench_dist_ref.py): the active-set
reference terminates on every batch of tests/test_wrench_dist_edges_gpu.py and its answer meets the optimality conditions
that the kernel's answers are held to; and the comparisons of those tests can fail -- three slips a kernel could make,
modelled in numpy, exceed their bounds."""
import numpy as np
import pytest
import test_wrench_dist_edges_gpu as edges
from wrench_dist_ref import LD, gmat, optimality_ratio, ref_distribute, ref_gain_table, ref_planned_wrench


@pytest.mark.parametrize("name", sorted(edges.DIST_CASES))
def test_reference_terminates_and_is_optimal(name):
    c = edges.DIST_CASES[name]
    dims, vertex, ridge, origin, w = edges.build_case(c)
    ww = np.ones(6) if c["ww"] is None else np.asarray(c["ww"])
    for k in range(c["n"]):
        m = int(dims[k])
        G = gmat(vertex[k], ridge[k], origin[k], m)
        s = ref_distribute(G, w[k], ww, c["rho"], c["lo"], c["hi"]).astype(np.float64)
        if m:
            assert optimality_ratio(G, w[k], ww, s, c["rho"], c["lo"], c["hi"]).max() <= 1.0
        if c["expect"] in ("all-lo", "box-point"):
            assert (s == c["lo"]).all()
        if c["expect"] == "all-hi":
            assert (s == c["hi"]).all()


def test_optimality_check_refuses_a_point_that_is_off():
    c = edges.DIST_CASES["M16-weights-a"]
    dims, vertex, ridge, origin, w = edges.build_case(c)
    G = gmat(vertex[0], ridge[0], origin[0], 16)
    s = ref_distribute(G, w[0], c["ww"], c["rho"], c["lo"], c["hi"]).astype(np.float64)
    free = np.flatnonzero((s > c["lo"]) & (s < c["hi"]))
    assert len(free) and (s == c["lo"]).any()
    off = s.copy()
    off[free[0]] += 1e-4  # a free ridge 1e-4 N away: the gradient moves by |sw o g_r|^2 1e-4, the tolerance is ~1e-4
    assert optimality_ratio(G, w[0], c["ww"], off, c["rho"], c["lo"], c["hi"]).max() > 2.0
    off = s.copy()
    off[free[0]] = c["lo"]  # a ridge clamped that wants to be free: the multiplier has the wrong sign
    assert optimality_ratio(G, w[0], c["ww"], off, c["rho"], c["lo"], c["hi"]).max() > 2.0


def _fused(N):
    x0, ref, *_ = edges.fused_inputs(19, N, 16, spread=True)
    K, F = ref_gain_table(N, 0.01, edges.AXIS_POS, edges.AXIS_WRENCH, edges.AXIS_JERK)
    return x0, ref, K, F, ref_planned_wrench(x0, ref, K, F, 0.01)


def _exceeds(wrong, planned):
    return (np.abs(wrong - planned).max(axis=1) > 1e-9 * (1 + np.abs(planned).max(axis=1))).all()


def test_a_swap_of_two_linear_axes_exceeds_the_planned_wrench_bound():
    x0, ref, K, F, planned = _fused(7)
    swapped = F.copy()
    swapped[[3, 4]] = F[[4, 3]]
    assert _exceeds(ref_planned_wrench(x0, ref, K, swapped, 0.01), planned)
    # ... which the default weights cannot see: there the linear axes share their gains
    Kd, Fd = ref_gain_table(7, 0.01)
    assert np.array_equal(Fd[3], Fd[4]) and np.array_equal(Fd[4], Fd[5])


def test_a_dropped_tail_of_the_stream_loop_exceeds_the_planned_wrench_bound():
    """L = 12 N = 72 at N = 6 (L mod 48 = 24): the flat dot product without its last 16 elements."""
    N = 6
    x0, ref, K, F, planned = _fused(N)
    short = F.copy()
    flat = np.arange(12 * N).reshape(N, 12)  # flat element -> (step, kind * 6 + axis)
    for f in flat.ravel()[-16:]:
        step, cls = divmod(int(f), 12)
        short[cls % 6, 2 * step + cls // 6] = 0
    assert _exceeds(ref_planned_wrench(x0, ref, K, short, 0.01), planned)


def test_a_projected_wrench_left_in_the_scaled_space_exceeds_the_weighted_bound():
    """wd_instance un-scales its row sums by isw = 1 / sqrt(ww); without it the output is sw o (G s)."""
    c = edges.DIST_CASES["M16-weights-a"]
    dims, vertex, ridge, origin, w = edges.build_case(c)
    sw = np.sqrt(np.asarray(c["ww"], LD))
    for k in range(8):
        G = gmat(vertex[k], ridge[k], origin[k], 16)
        s = ref_distribute(G, w[k], c["ww"], c["rho"], c["lo"], c["hi"])
        own, wrong = G @ s, sw * (G @ s)
        assert np.abs(wrong - own).max() > 1e-12 * (1 + np.abs(own).max())  # (the wrench against the returned scales)
        assert np.abs(sw * (wrong - own)).max() > 1e-9 * (1 + np.abs(sw * w[k]).max())  # (against the reference)
