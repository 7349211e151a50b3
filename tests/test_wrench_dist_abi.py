"""CPU checks of the wrench-distribution / PreviewControlCentroidal entries (include/ccc_amd.h): arguments are refused
before any device is touched, and the header shim's example compiles."""
import ctypes
import os
import subprocess

from centroidalcontrolcollection_amd import _lib, build, preview_control_centroidal

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _create(duration, dt, max_ridges):
    L = _lib.load()
    preview_control_centroidal._bind(L)
    inertia = (ctypes.c_double * 3)(40.0, 20.0, 10.0)
    h = ctypes.c_void_p()
    return L.ccc_pcc_create(100.0, inertia, duration, dt, None, None, None, None, max_ridges, 0, ctypes.byref(h))


def test_pcc_create_refuses_bad_arguments_before_the_device():
    assert _create(2.0, 0.0, 16) == _lib.CCC_ERR_INVALID_ARGUMENT
    assert _create(2.0, -0.01, 16) == _lib.CCC_ERR_INVALID_ARGUMENT
    assert _create(2.0, 0.01, 48) == _lib.CCC_ERR_UNSUPPORTED
    assert b"max_ridges = 48" in _lib.load().ccc_last_error_string()
    assert _create(5.13, 0.01, 16) == _lib.CCC_ERR_UNSUPPORTED  # 513 steps
    assert _lib.load().ccc_pcc_horizon_steps(None) == -1


def test_wrench_distribution_refuses_other_ridge_strides():
    L = _lib.load()
    L.ccc_wrench_distribution_device.restype = ctypes.c_int
    L.ccc_wrench_distribution_device.argtypes = [ctypes.c_int64, ctypes.c_int] + [ctypes.c_void_p] * 10
    assert L.ccc_wrench_distribution_device(4, 48, *([None] * 10)) == _lib.CCC_ERR_UNSUPPORTED
    assert L.ccc_wrench_distribution_device(4, 16, *([None] * 10)) == _lib.CCC_ERR_INVALID_ARGUMENT


def test_example_compiles(tmp_path):
    lib_dir = os.path.dirname(build.build_lib())
    cmd = ["g++", "-std=c++17", "-O2", "-Wall", "-Werror", "-I" + os.path.join(ROOT, "include"),
           os.path.join(ROOT, "examples", "plan_once_preview_control_centroidal.cpp"), "-L" + lib_dir, "-lccc_amd",
           "-Wl,-rpath," + lib_dir, "-o", str(tmp_path / "example")]
    out = subprocess.run(cmd, capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stderr[-2000:]
