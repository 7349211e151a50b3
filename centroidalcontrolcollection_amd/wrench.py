"""ForceColl::calcTotalWrench on the device (include/ccc_amd.h, csrc/wrench.hip): the step after planOnce of the
force-scale planners (LinearMpcXY, DdpCentroidal, DdpSingleRigidBody) -- /root/reference/tests/src/TestLinearMpcXY.cpp:119-120;
and ForceColl::WrenchDistribution::run (csrc/wrench_dist.hip): a planned wrench projected onto the ridge forces."""
import ctypes

from . import _lib


def total_wrench_device(dim, vertex, ridge, scales, origin, wrench=None, stream=None):
    """Device-resident torch tensors: dim [n] i32, vertex / ridge [n,M,3], scales [n,K] (first dim entries of a row used;
    a strided view of a larger tensor is fine as long as the last dimension is contiguous), origin [n,3].
    Returns wrench [n,6] = [moment; force] (asynchronous on `stream`)."""
    import torch

    L = _lib.load()
    if not getattr(L, "_wrench_bound", False):
        vp = ctypes.c_void_p
        L.ccc_total_wrench_device.restype = ctypes.c_int
        L.ccc_total_wrench_device.argtypes = [ctypes.c_int64, ctypes.c_int, vp, vp, vp, vp, ctypes.c_int, vp, vp, vp]
        L._wrench_bound = True
    n, M = vertex.shape[0], vertex.shape[1]
    if scales.stride(-1) != 1 or vertex.shape != ridge.shape or not vertex.is_contiguous() or not ridge.is_contiguous():
        raise ValueError("vertex / ridge must be contiguous [n,M,3] and the rows of scales contiguous")
    if wrench is None:
        wrench = torch.empty((n, 6), dtype=torch.float64, device=vertex.device)
    if stream is None:
        stream = torch.cuda.current_stream(vertex.device)
    _lib.check(L.ccc_total_wrench_device(n, M, ctypes.c_void_p(dim.data_ptr()), ctypes.c_void_p(vertex.data_ptr()),
                                         ctypes.c_void_p(ridge.data_ptr()), ctypes.c_void_p(scales.data_ptr()),
                                         int(scales.stride(0)) if n > 1 else int(scales.shape[-1]),
                                         ctypes.c_void_p(origin.data_ptr()), ctypes.c_void_p(wrench.data_ptr()),
                                         ctypes.c_void_p(stream.cuda_stream)))
    return wrench


class WrenchDistConfig(ctypes.Structure):
    """ccc_wrench_dist_config_t (defaults: ForceColl's WrenchDistribution::Configuration as recalled, include/ccc_amd.h)."""
    _fields_ = [("wrench_weight", ctypes.c_double * 6), ("regular_weight", ctypes.c_double),
                ("ridge_force_min", ctypes.c_double), ("ridge_force_max", ctypes.c_double)]

    def __init__(self, wrench_weight=None, regular_weight=None, ridge_force_min=None, ridge_force_max=None):
        super().__init__()
        L = _lib.load()
        L.ccc_wrench_dist_default_config.restype = None
        L.ccc_wrench_dist_default_config.argtypes = [ctypes.c_void_p]
        L.ccc_wrench_dist_default_config(ctypes.byref(self))
        if wrench_weight is not None:
            self.wrench_weight = (ctypes.c_double * 6)(*[float(x) for x in wrench_weight])
        for name, v in (("regular_weight", regular_weight), ("ridge_force_min", ridge_force_min),
                        ("ridge_force_max", ridge_force_max)):
            if v is not None:
                setattr(self, name, float(v))


def wrench_distribution_device(dim, vertex, ridge, desired_wrench, origin, config=None, stream=None):
    """Device-resident torch tensors: dim [n] i32, vertex / ridge [n,M,3] (M = 16, 32 or 64), desired_wrench [n,6]
    ([moment; force] about origin), origin [n,3].  Returns (wrench [n,6], scales [n,M], status [n] i32 =
    (iterations << 8) | CCC_STATUS_*), asynchronous on `stream`."""
    import torch

    L = _lib.load()
    if not getattr(L, "_wrench_dist_bound", False):
        vp = ctypes.c_void_p
        L.ccc_wrench_distribution_device.restype = ctypes.c_int
        L.ccc_wrench_distribution_device.argtypes = [ctypes.c_int64, ctypes.c_int] + [vp] * 10
        L._wrench_dist_bound = True
    n, M = vertex.shape[0], vertex.shape[1]
    for t in (dim, vertex, ridge, desired_wrench, origin):
        if not t.is_contiguous():
            raise ValueError("wrench_distribution_device takes contiguous tensors")
    if vertex.shape != ridge.shape or desired_wrench.shape != (n, 6) or origin.shape != (n, 3) or dim.dtype != torch.int32:
        raise ValueError("vertex / ridge [n,M,3], desired_wrench [n,6], origin [n,3], dim int32 [n]")
    wrench = torch.empty((n, 6), dtype=torch.float64, device=vertex.device)
    scales = torch.empty((n, M), dtype=torch.float64, device=vertex.device)
    status = torch.empty((n,), dtype=torch.int32, device=vertex.device)
    if stream is None:
        stream = torch.cuda.current_stream(vertex.device)
    p = lambda t: ctypes.c_void_p(t.data_ptr())
    _lib.check(L.ccc_wrench_distribution_device(n, M, p(dim), p(vertex), p(ridge), p(desired_wrench), p(origin),
                                                ctypes.byref(config) if config is not None else None, p(wrench),
                                                p(scales), p(status), ctypes.c_void_p(stream.cuda_stream)))
    return wrench, scales, status
