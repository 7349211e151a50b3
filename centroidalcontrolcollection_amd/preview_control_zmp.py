"""Host-side mirror of CCC::PreviewControlZmp over the C-ABI (include/ccc_amd.h, csrc/preview_zmp.hip).

Same names and argument meaning as the reference (/root/reference/include/CCC/PreviewControlZmp.h:92-140):
``PreviewControlZmp(com_height, horizon_duration, horizon_dt, weight_param)``, ``planOnce(ref_zmp_func, initial_param,
current_time, control_dt)`` -- plus the batched entry points, sampled (``planOnceBatch``) and from the knots of a
piecewise-linear reference (``planOnceBatchKnots``).  initial_param is a triple ``(pos [2], vel [2], acc [2])``.
"""
import ctypes

import numpy as np

from . import _lib

PREVIEW, SINGULAR = 0, 1  # CCC_PVZ_PREVIEW, CCC_PVZ_SINGULAR
MAX_STEPS, MAX_KNOTS = 512, 32  # CCC_PVZ_MAX_STEPS, CCC_PVZ_MAX_KNOTS


def _bind(L):
    if getattr(L, "_pvz_bound", False):
        return
    vp, d = ctypes.c_void_p, ctypes.c_double
    L.ccc_pvz_create.restype = ctypes.c_int
    L.ccc_pvz_create.argtypes = [ctypes.c_int, d, d, d, d, d, ctypes.c_int, ctypes.POINTER(vp)]
    L.ccc_pvz_destroy.restype = None
    L.ccc_pvz_destroy.argtypes = [vp]
    L.ccc_pvz_horizon_steps.restype = ctypes.c_int
    L.ccc_pvz_horizon_steps.argtypes = [vp]
    L.ccc_pvz_get_gains.restype = ctypes.c_int
    L.ccc_pvz_get_gains.argtypes = [vp, vp, vp, vp]
    L.ccc_pvz_plan_batch_device.restype = ctypes.c_int
    L.ccc_pvz_plan_batch_device.argtypes = [vp, ctypes.c_int64, vp, vp, d, vp, vp, vp]
    L.ccc_pvz_plan_batch.restype = ctypes.c_int
    L.ccc_pvz_plan_batch.argtypes = [vp, ctypes.c_int64, vp, vp, d, vp, vp]
    L.ccc_pvz_plan_knots_batch_device.restype = ctypes.c_int
    L.ccc_pvz_plan_knots_batch_device.argtypes = [vp, ctypes.c_int64] + [vp] * 5 + [d] + [vp] * 4
    L.ccc_pvz_plan_knots_batch.restype = ctypes.c_int
    L.ccc_pvz_plan_knots_batch.argtypes = [vp, ctypes.c_int64] + [vp] * 5 + [d] + [vp] * 3
    L._pvz_bound = True


def _p(a):
    return ctypes.c_void_p(a.ctypes.data)


def pack_knots(knot_lists):
    """A list of knot lists [(time, zmp [2]), ...] as the arrays of planOnceBatchKnots: (num_knots [n], knot_time [n,32],
    knot_zmp [n,32,2])."""
    n = len(knot_lists)
    num = np.array([len(k) for k in knot_lists], np.int32)
    time, zmp = np.zeros((n, MAX_KNOTS)), np.zeros((n, MAX_KNOTS, 2))
    for k, knots in enumerate(knot_lists):
        for i, (t, z) in enumerate(knots[:MAX_KNOTS]):
            time[k, i], zmp[k, i] = t, z
    return num, time, zmp


class _PreviewZmpHandle:
    """What the two mirrors share: a ccc_pvz_t handle and its batched entry points.  `OFF`: the first sample is at
    current_time + OFF * horizon_dt."""

    KIND, OFF = PREVIEW, 1

    def _create(self, com_height, horizon_duration, horizon_dt, weight_zmp, weight_com_jerk, device):
        L = _lib.load()
        _bind(L)
        self._L = L
        h = ctypes.c_void_p()
        _lib.check(L.ccc_pvz_create(self.KIND, float(com_height), float(horizon_duration), float(horizon_dt), float(weight_zmp),
                                    float(weight_com_jerk), int(device), ctypes.byref(h)))
        self._h = h
        self.device, self.com_height_, self.horizon_dt_ = int(device), float(com_height), float(horizon_dt)
        self.horizon_steps_ = L.ccc_pvz_horizon_steps(h)

    def __del__(self):
        h = getattr(self, "_h", None)
        if h:
            self._L.ccc_pvz_destroy(h)
            self._h = None

    def gains(self):
        """(K [3], w [N], riccati_error) of the handle (ccc_pvz_get_gains)."""
        K, w, err = np.zeros(3), np.zeros(self.horizon_steps_), np.zeros(1)
        _lib.check(self._L.ccc_pvz_get_gains(self._h, _p(K), _p(w), _p(err)))
        return K, w, float(err[0])

    def planOnceBatch(self, x0, ref, control_dt=-1.0):
        """Host arrays (ccc_pvz_plan_batch): x0 [n,2,3] (per axis, in the order of the class's state), ref [n,2,N] (the
        reference ZMP at current_time + (i + OFF) horizon_dt).  Returns dict(zmp [n,2], input [n,2])."""
        x0, ref = np.ascontiguousarray(x0, np.float64), np.ascontiguousarray(ref, np.float64)
        n = x0.shape[0]
        if x0.shape != (n, 2, 3) or ref.shape != (n, 2, self.horizon_steps_):
            raise ValueError("x0 [n,2,3], ref [n,2,%d]" % self.horizon_steps_)
        zmp, u = np.zeros((n, 2)), np.zeros((n, 2))
        _lib.check(self._L.ccc_pvz_plan_batch(self._h, n, _p(x0), _p(ref), float(control_dt), _p(zmp), _p(u)))
        return dict(zmp=zmp, input=u)

    def planOnceBatchKnots(self, num_knots, knot_time, knot_zmp, x0, current_time, control_dt=-1.0):
        """Host arrays (ccc_pvz_plan_knots_batch): the reference of instance k is the linear interpolation of its first
        num_knots[k] knots (knot_time [n,32] strictly increasing, knot_zmp [n,32,2]).  Returns dict(zmp [n,2], input [n,2],
        status [n]); an instance whose knots do not cover every sample is CCC_STATUS_INFEASIBLE with NaN outputs."""
        num_knots = np.ascontiguousarray(num_knots, np.int32)
        knot_time, knot_zmp = np.ascontiguousarray(knot_time, np.float64), np.ascontiguousarray(knot_zmp, np.float64)
        x0, current_time = np.ascontiguousarray(x0, np.float64), np.ascontiguousarray(current_time, np.float64)
        n, M = num_knots.shape[0], MAX_KNOTS
        if knot_time.shape != (n, M) or knot_zmp.shape != (n, M, 2) or x0.shape != (n, 2, 3) or current_time.shape != (n,):
            raise ValueError("num_knots [n], knot_time [n,32], knot_zmp [n,32,2], x0 [n,2,3], current_time [n]")
        zmp, u, status = np.zeros((n, 2)), np.zeros((n, 2)), np.zeros(n, np.int32)
        _lib.check(self._L.ccc_pvz_plan_knots_batch(self._h, n, _p(num_knots), _p(knot_time), _p(knot_zmp), _p(x0),
                                                    _p(current_time), float(control_dt), _p(zmp), _p(u), _p(status)))
        return dict(zmp=zmp, input=u, status=status)

    def plan_batch_device(self, x0, ref, zmp, control_dt=-1.0, input=None, stream=None):
        """Device-resident torch tensors (ccc_pvz_plan_batch_device), asynchronous on `stream`."""
        _lib.check(self._L.ccc_pvz_plan_batch_device(self._h, x0.shape[0], _tp(x0), _tp(ref), float(control_dt), _tp(zmp),
                                                     _tp(input), self._stream(stream)))

    def plan_knots_batch_device(self, num_knots, knot_time, knot_zmp, x0, current_time, zmp, control_dt=-1.0, input=None,
                                status=None, stream=None):
        """Device-resident torch tensors (num_knots / status int32), asynchronous on `stream`."""
        _lib.check(self._L.ccc_pvz_plan_knots_batch_device(self._h, x0.shape[0], _tp(num_knots), _tp(knot_time), _tp(knot_zmp),
                                                           _tp(x0), _tp(current_time), float(control_dt), _tp(zmp), _tp(input),
                                                           _tp(status), self._stream(stream)))

    def _stream(self, stream):
        import torch

        return ctypes.c_void_p((stream or torch.cuda.current_stream(self.device)).cuda_stream)

    def _plan_once(self, ref_zmp_func, x0, current_time, control_dt):
        """planOnce of both classes: ref_zmp_func sampled on the host, n = 1."""
        N = self.horizon_steps_
        ref = np.zeros((1, 2, N))
        for i in range(N):
            ref[0, :, i] = ref_zmp_func(current_time + (i + self.OFF) * self.horizon_dt_)
        return self.planOnceBatch(np.asarray(x0, np.float64)[None], ref, control_dt)["zmp"][0]


def _tp(t):
    return None if t is None else ctypes.c_void_p(t.data_ptr())


class PreviewControlZmp(_PreviewZmpHandle):
    class WeightParam:
        """PreviewControlZmp1d::WeightParam (PreviewControlZmp.h:28-44, same defaults)."""

        def __init__(self, zmp=1.0, com_jerk=1e-8):
            self.zmp, self.com_jerk = float(zmp), float(com_jerk)

    def __init__(self, com_height, horizon_duration, horizon_dt, weight_param=None, device=0):
        self.weight_param_ = weight_param or PreviewControlZmp.WeightParam()
        self._create(com_height, horizon_duration, horizon_dt, self.weight_param_.zmp, self.weight_param_.com_jerk, device)

    def planOnce(self, ref_zmp_func, initial_param, current_time, control_dt=-1.0):
        """CCC::PreviewControlZmp::planOnce (src/PreviewControlZmp.cpp:51-76): the planned ZMP [2]."""
        pos, vel, acc = (np.asarray(v, np.float64).reshape(2) for v in initial_param)
        return self._plan_once(ref_zmp_func, np.stack([pos, vel, acc], axis=1), current_time, control_dt)
