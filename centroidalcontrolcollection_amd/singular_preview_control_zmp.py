"""Host-side mirror of CCC::SingularPreviewControlZmp over the C-ABI (include/ccc_amd.h, csrc/preview_zmp.hip).

Same names and argument meaning as the reference (/root/reference/include/CCC/SingularPreviewControlZmp.h:86-130):
``SingularPreviewControlZmp(com_height, horizon_duration, horizon_dt)``, ``planOnce(ref_zmp_func, initial_param,
current_time, control_dt)`` with initial_param a triple ``(pos [2], vel [2], planned_zmp [2])`` -- plus the batched entry
points of preview_control_zmp, whose x0 is per axis (planned_zmp, pos, vel) here and whose samples start at
current_time itself.  control_dt is used as passed (src/SingularPreviewControlZmp.cpp:54): give it explicitly.
"""
import numpy as np

from .preview_control_zmp import SINGULAR, _PreviewZmpHandle


class SingularPreviewControlZmp(_PreviewZmpHandle):
    KIND, OFF = SINGULAR, 0

    def __init__(self, com_height, horizon_duration, horizon_dt, device=0):
        self._create(com_height, horizon_duration, horizon_dt, 0.0, 0.0, device)

    def planOnce(self, ref_zmp_func, initial_param, current_time, control_dt=-1.0):
        """CCC::SingularPreviewControlZmp::planOnce (src/SingularPreviewControlZmp.cpp:59-88): the planned ZMP [2]."""
        pos, vel, planned_zmp = (np.asarray(v, np.float64).reshape(2) for v in initial_param)
        return self._plan_once(ref_zmp_func, np.stack([planned_zmp, pos, vel], axis=1), current_time, control_dt)
