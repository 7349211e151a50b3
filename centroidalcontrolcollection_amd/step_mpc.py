"""Host-side mirror of CCC::StepMpc over the C-ABI (include/ccc_amd.h, csrc/step_mpc.hip).

Same names and argument meaning as the reference (/root/reference/include/CCC/StepMpc.h:163-240):
``StepMpc(com_height, weight_param)``, ``planOnce(ref_data, initial_param, current_time)`` -- plus the batched entry
points.  ref_data is a list of elements ``(is_single_support, zmp [2], end_time)``, initial_param a pair ``(pos [2],
vel [2])``; planOnce returns ``(current_zmp [2], next_foot_zmp [2] or None)``.
"""
import ctypes

import numpy as np

from . import _lib

MAX_ELEMENTS = 16  # CCC_STEP_MAX_ELEMENTS
HAS_NEXT_FOOT = 0x100  # CCC_STEP_HAS_NEXT_FOOT


class _Weights(ctypes.Structure):
    _fields_ = [(k, ctypes.c_double) for k in ("free_zmp", "fixed_zmp", "double_support", "pos", "vel", "capture_point_abs",
                                               "capture_point_rel")]


class LoopParams(ctypes.Structure):
    """ccc_step_loop_params_t: the constants of makeStepMpcRefData (FootstepManager.h:392-393) and of the footstep update
    (TestStepMpc.cpp:100-105)."""
    _fields_ = [("horizon_duration", ctypes.c_double), ("constant_zmp_duration", ctypes.c_double),
                ("pre_duration", ctypes.c_double), ("enable_footstep_update", ctypes.c_int32)]

    def __init__(self, horizon_duration=3.0, constant_zmp_duration=0.2, pre_duration=0.1, enable_footstep_update=True):
        super().__init__(float(horizon_duration), float(constant_zmp_duration), float(pre_duration),
                         int(bool(enable_footstep_update)))


def _bind(L):
    if getattr(L, "_step_bound", False):
        return
    vp = ctypes.c_void_p
    L.ccc_step_create.restype = ctypes.c_int
    L.ccc_step_create.argtypes = [ctypes.c_double, vp, ctypes.c_int, ctypes.POINTER(vp)]
    L.ccc_step_destroy.restype = None
    L.ccc_step_destroy.argtypes = [vp]
    L.ccc_step_plan_batch_device.restype = ctypes.c_int
    L.ccc_step_plan_batch_device.argtypes = [vp, ctypes.c_int64] + [vp] * 10
    L.ccc_step_plan_batch.restype = ctypes.c_int
    L.ccc_step_plan_batch.argtypes = [vp, ctypes.c_int64] + [vp] * 9
    L.ccc_step_closed_loop_device.restype = ctypes.c_int
    L.ccc_step_closed_loop_device.argtypes = [vp, ctypes.c_int64, ctypes.c_int] + [vp] * 7 + [
        ctypes.c_double, ctypes.c_double, ctypes.c_int, ctypes.c_int, vp, ctypes.c_double] + [vp] * 7
    L._step_bound = True


def _p(a):
    return ctypes.c_void_p(a.ctypes.data)


class StepMpc:
    class WeightParam:
        """StepMpc1d::WeightParam (StepMpc.h:80-123, same defaults)."""

        def __init__(self, free_zmp=1e-2, fixed_zmp=1e0, double_support=1e0, pos=0.0, vel=0.0, capture_point_abs=1e1,
                     capture_point_rel=1e1):
            self.free_zmp, self.fixed_zmp, self.double_support = float(free_zmp), float(fixed_zmp), float(double_support)
            self.pos, self.vel = float(pos), float(vel)
            self.capture_point_abs, self.capture_point_rel = float(capture_point_abs), float(capture_point_rel)

        def as_tuple(self):
            return (self.free_zmp, self.fixed_zmp, self.double_support, self.pos, self.vel, self.capture_point_abs,
                    self.capture_point_rel)

    def __init__(self, com_height, weight_param=None, device=0):
        L = _lib.load()
        _bind(L)
        self._L = L
        self.weight_param_ = weight_param or StepMpc.WeightParam()
        w = _Weights(*self.weight_param_.as_tuple())
        h = ctypes.c_void_p()
        _lib.check(L.ccc_step_create(float(com_height), ctypes.byref(w), int(device), ctypes.byref(h)))
        self._h = h
        self.device, self.com_height_ = int(device), float(com_height)

    def __del__(self):
        h = getattr(self, "_h", None)
        if h:
            self._L.ccc_step_destroy(h)
            self._h = None

    def planOnceBatch(self, num_elements, is_single_support, end_time, zmp, x0, current_time):
        """Host arrays (ccc_step_plan_batch): num_elements [n], is_single_support [n,16], end_time [n,16], zmp [n,16,2],
        x0 [n,4] (pos xy, vel xy), current_time [n].  Returns dict(current_zmp [n,2], next_foot_zmp [n,2],
        has_next_foot [n] bool, status [n], status_raw [n])."""
        num_elements = np.ascontiguousarray(num_elements, np.int32)
        is_single_support = np.ascontiguousarray(is_single_support, np.int32)
        end_time = np.ascontiguousarray(end_time, np.float64)
        zmp = np.ascontiguousarray(zmp, np.float64)
        x0 = np.ascontiguousarray(x0, np.float64)
        current_time = np.ascontiguousarray(current_time, np.float64)
        n, M = num_elements.shape[0], MAX_ELEMENTS
        if is_single_support.shape != (n, M) or end_time.shape != (n, M) or zmp.shape != (n, M, 2) or x0.shape != (n, 4) or \
                current_time.shape != (n,):
            raise ValueError("num_elements [n], is_single_support / end_time [n,16], zmp [n,16,2], x0 [n,4], current_time [n]")
        cur, foot, status = np.zeros((n, 2)), np.zeros((n, 2)), np.zeros(n, np.int32)
        _lib.check(self._L.ccc_step_plan_batch(self._h, n, _p(num_elements), _p(is_single_support), _p(end_time), _p(zmp),
                                               _p(x0), _p(current_time), _p(cur), _p(foot), _p(status)))
        return dict(current_zmp=cur, next_foot_zmp=foot, has_next_foot=(status & HAS_NEXT_FOOT) != 0, status=status & 0xff,
                    status_raw=status)

    def plan_batch_device(self, num_elements, is_single_support, end_time, zmp, x0, current_time, current_zmp, next_foot_zmp,
                          status=None, stream=None):
        """Device-resident torch tensors (num_elements / is_single_support / status int32), asynchronous on `stream`."""
        import torch

        if stream is None:
            stream = torch.cuda.current_stream(self.device)

        def p(t):
            return None if t is None else ctypes.c_void_p(t.data_ptr())

        _lib.check(self._L.ccc_step_plan_batch_device(self._h, num_elements.shape[0], p(num_elements), p(is_single_support),
                                                      p(end_time), p(zmp), p(x0), p(current_time), p(current_zmp),
                                                      p(next_foot_zmp), p(status), ctypes.c_void_p(stream.cuda_stream)))

    def closed_loop_device(self, timeline, com_state, t0, sim_dt, cycles, disturb_times=(), impulse=0.0, params=None,
                           status=None, updates=None, traj_com=None, traj_zmp=None, traj_next_foot=None, stream=None):
        """ccc_step_closed_loop_device: `cycles` control cycles of TestStepMpc.cpp:55-116 for every instance in one launch.
        timeline: dict of contiguous CUDA tensors (foot0 [n,2,2], foot_pos [n,K,2], foot_id [n,K] i32, swing_start /
        swing_end / transit_end [n,K]); foot_pos is rewritten where the loop adapts a footstep.  com_state [n,2,2] is
        updated in place; params a LoopParams (None: the reference's constants); status [n] i32, updates [n] i32
        (incremented), traj_com / traj_zmp / traj_next_foot [cycles,n,2] are optional.  Returns the time after the last
        cycle."""
        import torch

        n, K = timeline["foot_id"].shape
        if stream is None:
            stream = torch.cuda.current_stream(self.device)

        def p(t):
            return None if t is None else ctypes.c_void_p(t.data_ptr())

        dts = (ctypes.c_double * max(1, len(disturb_times)))(*disturb_times)
        _lib.check(self._L.ccc_step_closed_loop_device(
            self._h, n, K, *(p(timeline[k]) for k in ("foot0", "foot_pos", "foot_id", "swing_start", "swing_end",
                                                      "transit_end")), p(com_state), float(t0), float(sim_dt), int(cycles),
            len(disturb_times), dts, float(impulse), None if params is None else ctypes.cast(ctypes.byref(params), ctypes.c_void_p),
            p(status), p(updates), p(traj_com), p(traj_zmp), p(traj_next_foot), ctypes.c_void_p(stream.cuda_stream)))
        t = float(t0)
        for _ in range(int(cycles)):
            t += float(sim_dt)
        return t

    def planOnce(self, ref_data, initial_param, current_time):
        """CCC::StepMpc::planOnce (src/StepMpc.cpp:202-247)."""
        n = len(ref_data)
        if not 1 <= n <= MAX_ELEMENTS:
            raise ValueError("ref_data holds %d elements, this library plans 1 .. %d" % (n, MAX_ELEMENTS))
        flags, end_time, zmp = pack_ref_data([ref_data])[1:]
        x0 = np.concatenate([np.asarray(v, np.float64).reshape(2) for v in initial_param])[None]
        out = self.planOnceBatch([n], flags, end_time, zmp, x0, [current_time])
        if out["status"][0] != _lib.CCC_STATUS_SOLVED:
            raise ValueError("ref_data is not a valid timeline (durations > 0, no two double supports in a row)")
        return out["current_zmp"][0], (out["next_foot_zmp"][0] if out["has_next_foot"][0] else None)


def pack_ref_data(ref_data_list):
    """A list of element lists [(is_single_support, zmp [2], end_time), ...] as the arrays of planOnceBatch:
    (num_elements [n], is_single_support [n,16], end_time [n,16], zmp [n,16,2])."""
    n = len(ref_data_list)
    num = np.array([len(r) for r in ref_data_list], np.int32)
    flags, end_time = np.zeros((n, MAX_ELEMENTS), np.int32), np.zeros((n, MAX_ELEMENTS))
    zmp = np.zeros((n, MAX_ELEMENTS, 2))
    for k, ref in enumerate(ref_data_list):
        for i, (ss, z, te) in enumerate(ref[:MAX_ELEMENTS]):
            flags[k, i], end_time[k, i] = int(bool(ss)), te
            zmp[k, i] = z
    return num, flags, end_time, zmp
