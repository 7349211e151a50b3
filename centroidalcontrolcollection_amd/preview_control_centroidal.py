"""Host-side mirror of CCC::PreviewControlCentroidal over the C-ABI (include/ccc_amd.h, csrc/wrench_dist.hip).

Same names and argument meaning as the reference (/root/reference/include/CCC/PreviewControlCentroidal.h:137-262):
``PreviewControlCentroidal(mass, moment_of_inertia, horizon_duration, horizon_dt, weight_param)``,
``planOnce(motion_param, ref_data_func, initial_param, current_time, control_dt)`` returning the projected wrench
[moment; force] -- plus the batched entry points.  sva vectors are 6-arrays [angular; linear] / [moment; force]; the
contact list is the flattened (vertex [m,3], ridge [m,3]) pair of fixtures_ddp.contact_from_rect.
"""
import ctypes

import numpy as np

from . import _lib
from .wrench import WrenchDistConfig


def _bind(L):
    if getattr(L, "_pcc_bound", False):
        return
    vp, d = ctypes.c_void_p, ctypes.c_double
    L.ccc_pcc_create.restype = ctypes.c_int
    L.ccc_pcc_create.argtypes = [d, vp, d, d, vp, vp, vp, vp, ctypes.c_int, ctypes.c_int, ctypes.POINTER(vp)]
    L.ccc_pcc_destroy.restype = None
    L.ccc_pcc_destroy.argtypes = [vp]
    L.ccc_pcc_horizon_steps.restype = ctypes.c_int
    L.ccc_pcc_horizon_steps.argtypes = [vp]
    L.ccc_pcc_get_gains.restype = ctypes.c_int
    L.ccc_pcc_get_gains.argtypes = [vp, vp, vp, vp]
    L.ccc_pcc_plan_batch_device.restype = ctypes.c_int
    L.ccc_pcc_plan_batch_device.argtypes = [vp, ctypes.c_int64] + [vp] * 5 + [d] + [vp] * 5
    L.ccc_pcc_plan_batch.restype = ctypes.c_int
    L.ccc_pcc_plan_batch.argtypes = [vp, ctypes.c_int64] + [vp] * 5 + [d] + [vp] * 4
    L._pcc_bound = True


def _p(a):
    return None if a is None else ctypes.c_void_p(a.ctypes.data)


class PreviewControlCentroidal:
    class WeightParam:
        """PreviewControlCentroidal.h:182-218 (same defaults); wrench_dist_config: a WrenchDistConfig or None."""

        def __init__(self, pos=(1e2, 1e2, 1e2, 2e2, 2e2, 2e2), wrench=(5e-3, 5e-3, 5e-3, 5e-4, 5e-4, 5e-4), jerk=(1e-8,) * 6,
                     wrench_dist_config=None):
            self.pos, self.wrench, self.jerk = (np.asarray(v, np.float64).reshape(6) for v in (pos, wrench, jerk))
            self.wrench_dist_config = wrench_dist_config

    def __init__(self, mass, moment_of_inertia, horizon_duration, horizon_dt, weight_param=None, max_ridges=16, device=0):
        L = _lib.load()
        _bind(L)
        self._L = L
        w = weight_param or PreviewControlCentroidal.WeightParam()
        cfg = w.wrench_dist_config
        if cfg is not None and not isinstance(cfg, WrenchDistConfig):
            raise TypeError("wrench_dist_config must be a WrenchDistConfig")
        inertia = np.asarray(moment_of_inertia, np.float64).reshape(3)
        h = ctypes.c_void_p()
        _lib.check(L.ccc_pcc_create(float(mass), _p(inertia), float(horizon_duration), float(horizon_dt), _p(w.pos),
                                    _p(w.wrench), _p(w.jerk), ctypes.byref(cfg) if cfg is not None else None,
                                    int(max_ridges), int(device), ctypes.byref(h)))
        self._h = h
        self.device, self.max_ridges = int(device), int(max_ridges)
        self.mass_, self.horizon_dt_ = float(mass), float(horizon_dt)
        self.horizon_steps_ = L.ccc_pcc_horizon_steps(h)

    def __del__(self):
        h = getattr(self, "_h", None)
        if h:
            self._L.ccc_pcc_destroy(h)
            self._h = None

    def gains(self):
        """(K [6,3], F [6,2N], riccati_error [6]) of the six one-dimensional preview controllers."""
        K, F, err = np.zeros((6, 3)), np.zeros((6, 2 * self.horizon_steps_)), np.zeros(6)
        _lib.check(self._L.ccc_pcc_get_gains(self._h, _p(K), _p(F), _p(err)))
        return K, F, err

    def planOnceBatch(self, x0, ref, dim, vertex, ridge, control_dt=-1.0):
        """Host arrays (ccc_pcc_plan_batch): x0 [n,18] (pos, vel, acc; each angular then linear), ref [n,N,12]
        (RefData pos, wrench at t + (i+1) dt), dim [n], vertex / ridge [n,M,3].  Returns dict(wrench [n,6],
        planned_wrench [n,6], scales [n,M], status [n], iterations [n], status_raw [n])."""
        N, M = self.horizon_steps_, self.max_ridges
        x0 = np.ascontiguousarray(x0, np.float64)
        ref = np.ascontiguousarray(ref, np.float64)
        dim = np.ascontiguousarray(dim, np.int32)
        vertex = np.ascontiguousarray(vertex, np.float64)
        ridge = np.ascontiguousarray(ridge, np.float64)
        n = x0.shape[0]
        if x0.shape != (n, 18) or ref.shape != (n, N, 12) or dim.shape != (n,) or vertex.shape != (n, M, 3) or \
                ridge.shape != (n, M, 3):
            raise ValueError("x0 [n,18], ref [n,%d,12], dim [n], vertex / ridge [n,%d,3]" % (N, M))
        wrench, planned = np.zeros((n, 6)), np.zeros((n, 6))
        scales, status = np.zeros((n, M)), np.zeros(n, np.int32)
        _lib.check(self._L.ccc_pcc_plan_batch(self._h, n, _p(x0), _p(ref), _p(dim), _p(vertex), _p(ridge), float(control_dt),
                                              _p(wrench), _p(planned), _p(scales), _p(status)))
        return dict(wrench=wrench, planned_wrench=planned, scales=scales, status=status & 0xff, iterations=status >> 8,
                    status_raw=status)

    def plan_batch_device(self, x0, ref, dim, vertex, ridge, wrench, control_dt=-1.0, planned_wrench=None, scales=None,
                          status=None, stream=None):
        """Device-resident torch tensors (dim int32), asynchronous on `stream`."""
        import torch

        if stream is None:
            stream = torch.cuda.current_stream(self.device)

        def p(t):
            return None if t is None else ctypes.c_void_p(t.data_ptr())

        _lib.check(self._L.ccc_pcc_plan_batch_device(self._h, x0.shape[0], p(x0), p(ref), p(dim), p(vertex), p(ridge),
                                                     float(control_dt), p(wrench), p(planned_wrench), p(scales), p(status),
                                                     ctypes.c_void_p(stream.cuda_stream)))

    def planOnce(self, motion_param, ref_data_func, initial_param, current_time, control_dt=-1.0):
        """CCC::PreviewControlCentroidal::planOnce (src/PreviewControlCentroidal.cpp:91-130).  motion_param: (vertex [m,3],
        ridge [m,3]); ref_data_func(t) -> (pos [6], wrench [6]); initial_param: (pos [6], vel [6], acc [6])."""
        N, M = self.horizon_steps_, self.max_ridges
        V, R = (np.asarray(a, np.float64).reshape(-1, 3) for a in motion_param)
        if len(V) > M:
            raise ValueError("the contact list has %d ridges, the handle was created for %d" % (len(V), M))
        vertex, ridge = np.zeros((1, M, 3)), np.zeros((1, M, 3))
        vertex[0, :len(V)], ridge[0, :len(R)] = V, R
        ref = np.zeros((1, N, 12))
        for i in range(N):
            pos, wr = ref_data_func(current_time + (i + 1) * self.horizon_dt_)
            ref[0, i, :6], ref[0, i, 6:] = pos, wr
        x0 = np.concatenate([np.asarray(v, np.float64).reshape(6) for v in initial_param])[None]
        return self.planOnceBatch(x0, ref, [len(V)], vertex, ridge, control_dt)["wrench"][0]
