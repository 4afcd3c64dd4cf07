"""racing-lmpc-ros2_amd -- MI355X-native batched LMPC solve path (host-side Python mirror).

Thin ctypes layer over the C ABI in include/lmpc_hip.h (lib/liblmpc_hip.so, hand-written HIP
for gfx950).  PyTorch is used only for device memory, streams and torch.distributed; all
compute happens in the HIP kernels.  There is no CPU fallback: importing `capi` without the
built library raises.
"""
from . import closed_loop, presets, racing_trajectory, ros_params, safe_set, workloads  # noqa: F401
from .capi import (LmpcError, Solver, SplineTrack, SOLVE_INFEASIBLE, SOLVE_MAX_ITER, SOLVE_OPTIMAL,  # noqa: F401
                   TRACK_BAD_INPUT, TRACK_NOT_CONVERGED, TRACK_OK, EKF_FALLBACK, EKF_NOT_FINITE, EKF_R_REPAIRED, LQR_NOT_FINITE, CLqrConfig, VANILLA_NOT_FINITE, CVanillaConfig, library_path, load_library)

__all__ = ["presets", "ros_params", "workloads", "closed_loop", "safe_set", "racing_trajectory", "Solver", "SplineTrack", "LmpcError", "load_library", "library_path",
           "SOLVE_OPTIMAL", "SOLVE_MAX_ITER", "SOLVE_INFEASIBLE", "TRACK_OK", "TRACK_NOT_CONVERGED", "TRACK_BAD_INPUT",
           "EKF_FALLBACK", "EKF_R_REPAIRED", "EKF_NOT_FINITE", "LQR_NOT_FINITE", "CLqrConfig", "VANILLA_NOT_FINITE", "CVanillaConfig"]
