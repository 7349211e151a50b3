"""The edges of ccc_wrench_distribution_device and of the fused ccc_pcc_* entries (csrc/wrench_dist.hip) that
tests/test_wrench_dist_gpu.py leaves out: per-axis weights, ragged and out-of-range ridge counts, rank-deficient free sets,
degenerate boxes and targets, an offset world frame, small batches and NULL optional outputs; for the fused kernel every
tail of its stream loop, six distinct axes, the control_dt override, the host entry's staging buffer and the executed
header shim.  Every returned point is checked by its optimality conditions alone (wrench_dist_ref.optimality_ratio)
besides the comparison with the active-set reference."""
import ctypes
import os
import subprocess

import numpy as np
import pytest
from wrench_dist_ref import (BLOCK_ITERS, INERTIA, MASS, N_INST, axis_inertia, check_distribution, make_batch,
                             ref_gain_table, ref_planned_wrench)

from centroidalcontrolcollection_amd import fixtures_ddp as fx

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
WW_A, WW_B = (1.0, 1.0, 0.1, 10.0, 10.0, 100.0), (100.0, 10.0, 1.0, 1.0, 0.1, 0.01)
# one count per instance, cycled: the four rows of a wavefront differ, partial slots included
RAGGED = {16: [0, 1, 2, 3, 5, 7, 15, 16], 32: [0, 1, 15, 16, 17, 31, 32], 64: [0, 1, 16, 17, 33, 48, 49, 63, 64]}


def case(M=16, dim=None, ww=None, lo=3.0, hi=1000.0, rho=1e-8, target="noise", w_scale=1.0, shift=None, nanfill=False,
         dup=False, n=N_INST, compare_s=False, expect=None):
    return dict(M=M, dim=M if dim is None else dim, ww=ww, lo=lo, hi=hi, rho=rho, target=target, w_scale=w_scale,
                shift=shift, nanfill=nanfill, dup=dup, n=n, compare_s=compare_s, expect=expect)


DIST_CASES = {
    "M16-weights-a": case(16, ww=WW_A), "M16-weights-b": case(16, ww=WW_B),
    "M32-weights-a": case(32, ww=WW_A), "M32-weights-b": case(32, ww=WW_B),
    "M16-ragged": case(16, dim=RAGGED[16], nanfill=True), "M32-ragged": case(32, dim=RAGGED[32], nanfill=True),
    "M64-ragged": case(64, dim=RAGGED[64], nanfill=True),
    # free sets of rank 1, 2, 3 (ridges of one vertex), 3 (all four of it), and two identical columns
    "rank-m1": case(16, dim=1), "rank-m2": case(16, dim=2), "rank-m3": case(16, dim=3), "rank-m4": case(16, dim=4),
    "rank-duplicate-column": case(16, dup=True),
    "rank-duplicate-column-rho1e-2-compare-s": case(16, dup=True, rho=1e-2, compare_s=True),
    "box-lo-equals-hi": case(16, lo=3.0, hi=3.0, expect="box-point"),
    "box-lo-zero": case(32, lo=0.0, hi=1000.0), "box-lo-negative": case(32, lo=-5.0, hi=50.0),
    "box-hi-1e6": case(16, lo=3.0, hi=1e6),
    "target-pulls-down": case(16, target="down", expect="all-lo"), "target-zero": case(16, target="zero", expect="all-lo"),
    "target-1e4-hi-40": case(16, hi=40.0, w_scale=1e4, expect="all-hi"),
    "offset-world-frame": case(32, shift=(100.0, -50.0, 0.0)),
    "n1": case(16, n=1), "n15": case(16, n=15), "n16": case(16, n=16), "n17": case(16, n=17),
}


def build_case(c):
    """(dims, vertex, ridge, origin, w) of a DIST_CASES entry."""
    M, n = c["M"], c["n"]
    dim = c["dim"] if np.isscalar(c["dim"]) else np.resize(np.asarray(c["dim"], np.int32), n)
    dims, vertex, ridge, origin, w = make_batch(M, dim, n=n)
    if c["dup"]:
        vertex[:, 1], ridge[:, 1] = vertex[:, 0], ridge[:, 0]
    if c["target"] == "down":
        w[:] = (0.0, 0.0, 0.0, 0.0, 0.0, -MASS * fx.G)
    elif c["target"] == "zero":
        w[:] = 0.0
    w *= c["w_scale"]
    if c["shift"] is not None:
        vertex += np.asarray(c["shift"])
        origin += np.asarray(c["shift"])
    if c["nanfill"]:  # the slots at and beyond dim must not be read
        for k in range(n):
            vertex[k, dims[k]:], ridge[k, dims[k]:] = np.nan, np.nan
    return dims, vertex, ridge, origin, w


def _config(c):
    from centroidalcontrolcollection_amd import wrench as wmod

    return wmod.WrenchDistConfig(wrench_weight=c["ww"], regular_weight=c["rho"], ridge_force_min=c["lo"],
                                 ridge_force_max=c["hi"])


def _dev(a):
    import torch

    return torch.as_tensor(np.ascontiguousarray(a), device=torch.device("cuda"))


def run_distribution(inputs, cfg):
    import torch

    from centroidalcontrolcollection_amd import wrench as wmod

    dims, vertex, ridge, origin, w = inputs
    out = wmod.wrench_distribution_device(_dev(dims), _dev(vertex), _dev(ridge), _dev(w), _dev(origin), cfg)
    torch.cuda.synchronize()
    return tuple(t.cpu().numpy() for t in out)


@pytest.mark.gpu
@pytest.mark.parametrize("name", sorted(DIST_CASES))
def test_distribution_edges(name):
    c = DIST_CASES[name]
    inputs = build_case(c)
    dims, vertex, ridge, origin, w = inputs
    wrench, scales, status = run_distribution(inputs, _config(c))
    check_distribution(dims, vertex, ridge, origin, w, wrench, scales, status, c["lo"], c["hi"], c["rho"],
                       compare_s=c["compare_s"], ww=c["ww"], label=name)
    for k in range(c["n"]):
        m = int(dims[k])
        if c["expect"] in ("all-lo", "box-point"):
            assert (scales[k, :m] == c["lo"]).all(), k
        if c["expect"] == "all-hi":
            assert (scales[k, :m] == c["hi"]).all(), k
        if c["expect"] == "box-point":
            own = np.concatenate(fx.total_wrench(vertex[k], ridge[k], np.full(m, c["lo"]), origin[k]))
            assert np.abs(wrench[k] - own).max() <= 1e-12 * (1 + np.abs(own).max())


@pytest.mark.gpu
def test_both_solver_paths_run():
    """Which path the rows take, measured on an MI355X: the share of the 67 instances with more than kWdBlockIters = 24
    iterations (restarted in single-change mode) and the iteration maximum, per case of tests/test_wrench_dist_gpu.py and
    of this file --
      M16-base 0.075 / 34, M16-all-at-hi 0 / 19, M16-two-vertices 0.015 / 29, M16-no-contact-rows 0.060 / 34,
      M32-base 0.269 / 41, M32-mixed 0.836 / 94, M64-base 0.448 / 45, M16-rho1e-2 0 / 6;
      M16-weights-a 0.075 / 39, -b 0.075 / 41, M32-weights-a 0.239 / 43, -b 0.343 / 41, M16-ragged 0.030 / 32,
      M32-ragged 0.134 / 37, M64-ragged 0.313 / 40, rank-m1 ... m4 0 / 3, duplicate column 0.060 / 33 (rho 1e-2: 0 / 8),
      box (3, 3) 0 / 17, (0, 1000) 0.239 / 41, (-5, 50) 0.910 / 89, (3, 1e6) 0.015 / 34, the three targets 0 / 16,
      offset frame 0.269 / 41.
    Both paths occur in most of them; M64-base has the largest minority share (30 of 67 restart), so it is the one held
    to it here: a change that makes every row restart, or none, shows."""
    dims, vertex, ridge, origin, w = make_batch(64, 64)
    _, _, status = run_distribution((dims, vertex, ridge, origin, w), _config(case(64)))
    iters = status >> 8
    print("M64-base: %d of %d rows restarted, iterations max %d" % ((iters > BLOCK_ITERS).sum(), len(iters), iters.max()))
    assert (status & 0xff == 0).all()
    assert (iters > BLOCK_ITERS).any() and (iters <= BLOCK_ITERS).any()


@pytest.mark.gpu
@pytest.mark.parametrize("M", [16, 32, 64])
def test_out_of_range_counts_are_clamped(M):
    """dim = -3 behaves as 0 and dim = M + 5 as M (include/ccc_amd.h): bitwise the outputs of the clamped counts."""
    c = case(M)
    dims, vertex, ridge, origin, w = build_case(c)
    wild = np.resize(np.array([-3, M + 5, M, 0, M + 5, -3, 7], np.int32), c["n"])
    clamped = np.clip(wild, 0, M).astype(np.int32)
    a = run_distribution((wild, vertex, ridge, origin, w), _config(c))
    b = run_distribution((clamped, vertex, ridge, origin, w), _config(c))
    assert all(np.array_equal(x, y) for x, y in zip(a, b))
    assert (a[2] & 0xff == 0).all() and (a[1][clamped == 0] == 0).all() and (a[0][clamped == 0] == 0).all()


def _c_distribution(n, M, inputs, cfg, wrench, scales, status):
    """ccc_wrench_distribution_device itself (device tensors; scales / status may be None)."""
    import torch

    from centroidalcontrolcollection_amd import _lib

    L = _lib.load()
    L.ccc_wrench_distribution_device.restype = ctypes.c_int
    L.ccc_wrench_distribution_device.argtypes = [ctypes.c_int64, ctypes.c_int] + [ctypes.c_void_p] * 10
    p = lambda t: None if t is None else ctypes.c_void_p(t.data_ptr())
    dims, vertex, ridge, origin, w = inputs
    rc = L.ccc_wrench_distribution_device(n, M, p(dims), p(vertex), p(ridge), p(w), p(origin), ctypes.byref(cfg), p(wrench),
                                          p(scales), p(status), ctypes.c_void_p(torch.cuda.current_stream().cuda_stream))
    torch.cuda.synchronize()
    return rc


@pytest.mark.gpu
def test_empty_batch_and_null_optional_outputs():
    import torch

    from centroidalcontrolcollection_amd import _lib

    c = case(16)
    inputs = tuple(_dev(a) for a in build_case(c))
    n, cfg = c["n"], _config(c)
    new = lambda shape, dtype: torch.full(shape, -7, dtype=dtype, device="cuda")
    wrench, scales, status = new((n, 6), torch.float64), new((n, 16), torch.float64), new((n,), torch.int32)
    # n = 0: CCC_OK and nothing written
    assert _c_distribution(0, 16, inputs, cfg, wrench, scales, status) == _lib.CCC_OK
    assert (wrench == -7).all() and (scales == -7).all() and (status == -7).all()
    assert _c_distribution(n, 16, inputs, cfg, wrench, scales, status) == _lib.CCC_OK
    assert (status.cpu().numpy() & 0xff == 0).all()
    alone = new((n, 6), torch.float64)
    assert _c_distribution(n, 16, inputs, cfg, alone, None, None) == _lib.CCC_OK
    assert torch.equal(alone, wrench)


# ------------------------------------------------------------------------------------------------ the fused kernel

def fused_inputs(n, N, M, dim=None, seed=7, spread=False):
    """x0 [n,18], ref [n,N,12] and the contact arrays; spread: every axis draws its reference at its own magnitude."""
    dims, vertex, ridge, origin, _ = make_batch(M, M if dim is None else dim, n=n)
    rng = np.random.default_rng(seed)
    x0 = 0.05 * rng.standard_normal((n, 18))
    x0[:, 3:6] = origin
    mag = 1.0 + 0.5 * np.arange(6) if spread else np.ones(6)
    ref = np.zeros((n, N, 12))
    ref[:, :, 0:6] = 0.02 * mag * rng.standard_normal((n, N, 6))
    ref[:, :, 3:6] += origin[:, None, :]
    ref[:, :, 6:12] = 5.0 * mag[::-1] * rng.standard_normal((n, N, 6))
    return x0, ref, dims, vertex, ridge, origin


def check_planned(out, x0, ref, K, F, control_dt):
    planned = ref_planned_wrench(x0, ref, K, F, control_dt)
    scale = 1 + np.abs(planned).max(axis=1)
    err = np.abs(out["planned_wrench"] - planned).max(axis=1) / scale
    print("planned wrench: worst error / scale %.3g" % err.max())
    assert (err <= 1e-9).all()


HDT = 0.0078125  # 2^-7: N * HDT / HDT is N exactly, up to the 512 steps of CCC_PCC_MAX_STEPS


@pytest.mark.gpu
@pytest.mark.parametrize("N", [1, 2, 3, 4, 6, 7, 512])
def test_fused_horizons(N):
    """L = 12 N elements per instance in a loop unrolled by three over 16 lanes: L mod 48 = 12, 24, 36, 0 (N = 1 / 2 / 3 / 4
    and again 6 / 7 behind a full turn), L < 16 (N = 1) and the 48 KB of LDS at N = 512."""
    from centroidalcontrolcollection_amd import PreviewControlCentroidal

    n = 19
    pc = PreviewControlCentroidal(MASS, INERTIA, N * HDT, HDT)
    assert pc.horizon_steps_ == N
    x0, ref, dims, vertex, ridge, origin = fused_inputs(n, N, 16, spread=True)
    out = pc.planOnceBatch(x0, ref, dims, vertex, ridge)
    K, F = ref_gain_table(N, HDT)
    check_planned(out, x0, ref, K, F, HDT)
    check_distribution(dims, vertex, ridge, origin, out["planned_wrench"], out["wrench"], out["scales"], out["status_raw"],
                       3.0, 1000.0, 1e-8, label="fused-horizon-N%d" % N)


@pytest.mark.gpu
def test_fused_horizon_of_513_steps_is_refused():
    from centroidalcontrolcollection_amd import PreviewControlCentroidal, _lib

    with pytest.raises(_lib.CccError) as err:
        PreviewControlCentroidal(MASS, INERTIA, 513 * HDT, HDT)
    assert err.value.code == _lib.CCC_ERR_UNSUPPORTED


# (not in proportion: an axis whose three weights are all scaled by one factor keeps its gains, the cost only scales)
AXIS_POS = (100.0, 130.0, 170.0, 200.0, 260.0, 340.0)
AXIS_WRENCH = (5e-3, 8e-3, 3e-3, 5e-4, 9e-4, 3e-4)
AXIS_JERK = (1e-8, 2e-8, 5e-9, 1e-8, 4e-9, 3e-8)


@pytest.mark.gpu
@pytest.mark.parametrize("N", [7, 200])
def test_fused_six_distinct_axes(N):
    """With the default weights and one mass the three linear axes share K and F, and a swap between them -- in the permuted
    gain table, the class selection or the three accumulators -- passes.  Here every axis has weights and references of its own."""
    from centroidalcontrolcollection_amd import PreviewControlCentroidal

    wp = PreviewControlCentroidal.WeightParam(pos=AXIS_POS, wrench=AXIS_WRENCH, jerk=AXIS_JERK)
    pc = PreviewControlCentroidal(MASS, INERTIA, N * HDT, HDT, wp)
    assert pc.horizon_steps_ == N
    Kr, Fr = ref_gain_table(N, HDT, AXIS_POS, AXIS_WRENCH, AXIS_JERK)
    K, F, err = pc.gains()
    assert np.isfinite(err).all()
    for a in range(6):
        assert np.abs(K[a] - Kr[a]).max() <= 1e-9 * np.abs(Kr[a]).max()
        assert np.abs(F[a] - Fr[a]).max() <= 1e-9 * np.abs(Fr[a]).max()
    x0, ref, dims, vertex, ridge, origin = fused_inputs(N_INST, N, 16, spread=True)
    out = pc.planOnceBatch(x0, ref, dims, vertex, ridge)
    check_planned(out, x0, ref, Kr, Fr, HDT)
    check_distribution(dims, vertex, ridge, origin, out["planned_wrench"], out["wrench"], out["scales"], out["status_raw"],
                       3.0, 1000.0, 1e-8, label="fused-distinct-axes-N%d" % N)


@pytest.mark.gpu
def test_fused_control_dt_override():
    """src/PreviewControlCentroidal.cpp:38-41: a negative control_dt means horizon_dt, anything else is used, zero included
    -- then the jerk drops out and the planned wrench is inertia x acc (+ m g) to rounding."""
    from centroidalcontrolcollection_amd import PreviewControlCentroidal

    N, hdt = 5, 0.02
    pc = PreviewControlCentroidal(MASS, INERTIA, N * hdt, hdt)
    assert pc.horizon_steps_ == N
    K, F = ref_gain_table(N, hdt)
    x0, ref, dims, vertex, ridge, origin = fused_inputs(N_INST, N, 16, spread=True)
    outs = {}
    for cdt in (-1.0, 0.0, 0.005):
        out = outs[cdt] = pc.planOnceBatch(x0, ref, dims, vertex, ridge, control_dt=cdt)
        check_planned(out, x0, ref, K, F, hdt if cdt < 0 else cdt)
        check_distribution(dims, vertex, ridge, origin, out["planned_wrench"], out["wrench"], out["scales"],
                           out["status_raw"], 3.0, 1000.0, 1e-8, label="fused-control-dt%g" % cdt)
    explicit = pc.planOnceBatch(x0, ref, dims, vertex, ridge, control_dt=hdt)
    assert np.array_equal(outs[-1.0]["planned_wrench"], explicit["planned_wrench"])
    assert not np.array_equal(outs[-1.0]["planned_wrench"], outs[0.005]["planned_wrench"])
    still = axis_inertia() * x0[:, 12:18]
    still[:, 5] += MASS * fx.G
    # two roundings (the product, the sum with m g), each half an ulp of the result's scale
    assert (np.abs(outs[0.0]["planned_wrench"] - still) <= np.finfo(np.float64).eps * (1 + np.abs(still))).all()


@pytest.mark.gpu
def test_fused_config_through_the_class():
    from centroidalcontrolcollection_amd import PreviewControlCentroidal
    from centroidalcontrolcollection_amd.wrench import WrenchDistConfig

    N, M = 5, 32
    cfg = WrenchDistConfig(wrench_weight=WW_A, ridge_force_min=0.0, ridge_force_max=200.0)
    pc = PreviewControlCentroidal(MASS, INERTIA, N * 0.01, 0.01, PreviewControlCentroidal.WeightParam(wrench_dist_config=cfg),
                                  max_ridges=M)
    x0, ref, dims, vertex, ridge, origin = fused_inputs(N_INST, N, M, dim=np.resize(np.asarray(RAGGED[M], np.int32), N_INST))
    for k in range(N_INST):
        vertex[k, dims[k]:], ridge[k, dims[k]:] = np.nan, np.nan
    out = pc.planOnceBatch(x0, ref, dims, vertex, ridge)
    K, F = ref_gain_table(N, 0.01)
    check_planned(out, x0, ref, K, F, 0.01)
    check_distribution(dims, vertex, ridge, origin, out["planned_wrench"], out["wrench"], out["scales"], out["status_raw"],
                       0.0, 200.0, 1e-8, ww=WW_A, label="fused-config-ragged-M32")


OUT_KEYS = ("wrench", "planned_wrench", "scales", "status_raw")


@pytest.mark.gpu
def test_host_entry_regrows_its_staging_buffer():
    """n = 40, then 67 (the buffer is freed and allocated again), then 5 (a larger buffer serves a smaller batch): each
    result bitwise that of a fresh handle."""
    from centroidalcontrolcollection_amd import PreviewControlCentroidal

    N = 5
    make = lambda: PreviewControlCentroidal(MASS, INERTIA, N * 0.01, 0.01)
    x0, ref, dims, vertex, ridge, _ = fused_inputs(N_INST, N, 16)
    pc = make()
    for n in (40, 67, 5):
        args = (x0[:n], ref[:n], dims[:n], vertex[:n], ridge[:n])
        got, fresh = pc.planOnceBatch(*args), make().planOnceBatch(*args)
        assert (got["status"] == 0).all()
        for key in OUT_KEYS:
            assert np.array_equal(got[key], fresh[key]), (n, key)


@pytest.mark.gpu
def test_host_entry_with_null_optional_outputs():
    """ccc_pcc_plan_batch with planned_wrench, scales and status all NULL (the header shim passes the first two NULL)."""
    from centroidalcontrolcollection_amd import PreviewControlCentroidal, _lib
    from centroidalcontrolcollection_amd.preview_control_centroidal import _p

    N, n = 5, N_INST
    pc = PreviewControlCentroidal(MASS, INERTIA, N * 0.01, 0.01)
    x0, ref, dims, vertex, ridge, _ = fused_inputs(n, N, 16)
    full = pc.planOnceBatch(x0, ref, dims, vertex, ridge)
    wrench = np.full((n, 6), -7.0)
    _lib.check(pc._L.ccc_pcc_plan_batch(pc._h, n, _p(x0), _p(ref), _p(dims), _p(vertex), _p(ridge), -1.0, _p(wrench), None,
                                        None, None))
    assert np.array_equal(wrench, full["wrench"])


@pytest.mark.gpu
def test_device_entry_matches_host_entry():
    import torch

    from centroidalcontrolcollection_amd import PreviewControlCentroidal

    N, n, M = 5, N_INST, 32
    pc = PreviewControlCentroidal(MASS, INERTIA, N * 0.01, 0.01, max_ridges=M)
    x0, ref, dims, vertex, ridge, _ = fused_inputs(n, N, M)
    host = pc.planOnceBatch(x0, ref, dims, vertex, ridge, control_dt=0.005)
    f64 = lambda *shape: torch.full(shape, -7.0, dtype=torch.float64, device="cuda")
    dev = dict(wrench=f64(n, 6), planned_wrench=f64(n, 6), scales=f64(n, M),
               status_raw=torch.full((n,), -7, dtype=torch.int32, device="cuda"))
    pc.plan_batch_device(_dev(x0), _dev(ref), _dev(dims), _dev(vertex), _dev(ridge), dev["wrench"], 0.005,
                         dev["planned_wrench"], dev["scales"], dev["status_raw"])
    torch.cuda.synchronize()
    for key in OUT_KEYS:
        assert np.array_equal(dev[key].cpu().numpy(), host[key]), key


@pytest.mark.gpu
def test_cpp_header_shim_matches_python_mirror():
    """Host C++ against include/CCC/PreviewControlCentroidal.h (examples/plan_once_preview_control_centroidal.cpp): same
    kernel, same sampled inputs as the Python mirror -> identical projected wrenches, all 24 numbers."""
    exe = os.path.join(ROOT, "examples", "plan_once_preview_control_centroidal")
    if not os.path.exists(exe):
        import __graft_entry__

        __graft_entry__.build()
    run = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert run.returncode == 0, run.stdout + run.stderr
    lines = run.stdout.strip().splitlines()
    assert len(lines) == 4 and lines[0].startswith("planOnce wrench=")
    numbers = lambda line: [float(x) for x in line.split("wrench=")[1].split("status=")[0].split()]
    from centroidalcontrolcollection_amd import PreviewControlCentroidal

    N, dt = 200, 0.01
    pc = PreviewControlCentroidal(MASS, INERTIA, 2.0, dt)
    V, R = fx.contact_from_rect((-0.1, -0.1), (0.1, 0.1))
    zero = np.zeros(3)

    def ref_data_func(t):
        lin = (0.0, 0.0, 1.0) if t + 1e-6 < 1.4 else (0.25, 0.0, 1.2)
        return np.concatenate([zero, lin]), np.zeros(6)

    start = lambda k: (np.array([0.0, 0.0, 0.0, 0.01 * float(k), 0.0, 1.0]), np.zeros(6), np.zeros(6))
    one = pc.planOnce((V, R), ref_data_func, start(0), 0.0, 0.005)
    assert numbers(lines[0]) == list(one)
    times = (0.0, 0.5, 1.0)
    x0 = np.stack([np.concatenate(start(k)) for k in range(3)])
    ref = np.zeros((3, N, 12))
    for k, t in enumerate(times):
        for i in range(N):
            ref[k, i, :6], ref[k, i, 6:] = ref_data_func(t + (i + 1) * dt)
    out = pc.planOnceBatch(x0, ref, np.full(3, 16, np.int32), np.tile(V, (3, 1, 1)), np.tile(R, (3, 1, 1)), control_dt=0.005)
    for k in range(3):
        assert lines[1 + k].startswith("batch[%d] wrench=" % k) and lines[1 + k].endswith("status=0")
        assert numbers(lines[1 + k]) == list(out["wrench"][k]), k
    assert (out["status"] == 0).all()
