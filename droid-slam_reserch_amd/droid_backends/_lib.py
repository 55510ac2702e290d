"""ctypes binding of the C-ABI library (include/droid_backends_hip.h).

The HIP library is the product: if it cannot be loaded this module raises -- there is no CPU
fallback and nothing here imports the test oracle.
"""
from __future__ import annotations

import ctypes
import os

_HERE = os.path.dirname(os.path.abspath(__file__))
# DROID_HIP_LIB selects another build of the same library (diagnostic builds, tools/README.md)
LIB_PATH = os.environ.get("DROID_HIP_LIB") or os.path.join(_HERE, "libdroid_backends_hip.so")

# every symbol include/droid_backends_hip.h declares (tests check the library exports them all)
SYMBOLS = [
    "droid_abi_version", "droid_last_error",
    "droid_corr_index_forward", "droid_corr_index_backward", "droid_corr_pyramid_forward",
    "droid_corr_volume_pyramid", "droid_corr_pyramid_forward_slots", "droid_corr_volume_pyramid_slots",
    "droid_altcorr_forward", "droid_altcorr_backward", "droid_altcorr_pyramid_forward",
    "droid_altcorr_pyramid_forward_f16",
    "droid_ba_workspace_bytes", "droid_ba", "droid_ba_prepare", "droid_ba_build", "droid_ba_build_packed",
    "droid_ba_packed_system", "droid_ba_unpack_system",
    "droid_ba_overlap_available", "droid_ba_overlap_plan", "droid_ba_unpack_chunk", "droid_ba_solve_update_overlap",
    "droid_ba_solve_update", "droid_ba_profile_iteration", "droid_ba_system", "droid_ba_status",
    "droid_ba_attach_status_mirror", "droid_ba_attach_launch_hints", "droid_chol_solve", "droid_chol_scratch_doubles", "droid_reproject_motion",
    "droid_frame_distance", "droid_frame_distance_matrix", "droid_projmap", "droid_iproj", "droid_depth_filter",
    "droid_proximity_workspace_bytes", "droid_proximity_edges",
    "droid_cvx_upsample",
    "droid_graph_mean_workspace_bytes", "droid_graph_mean",
    "droid_se3_unary", "droid_se3_mul", "droid_pose_interpolate",
    "droid_point_cloud_workspace_bytes", "droid_point_cloud",
    "droid_test_wave_reduce32",
]

DROID_F16, DROID_F32, DROID_F64 = 0, 1, 2

_lib = None


class DroidBackendError(RuntimeError):
    pass


def load() -> ctypes.CDLL:
    """Load libdroid_backends_hip.so (built by csrc/build.sh or __graft_entry__.build())."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise DroidBackendError(
            f"{LIB_PATH} is missing: build the HIP extension first "
            "(python -c 'import __graft_entry__ as g; g.build()' or droid-slam_reserch_amd/csrc/build.sh). "
            "There is no CPU fallback.")
    lib = ctypes.CDLL(LIB_PATH)
    for s in SYMBOLS:
        if not hasattr(lib, s):
            raise DroidBackendError(f"{LIB_PATH} does not export {s}")
    c_int, c_float, vp, sz = ctypes.c_int, ctypes.c_float, ctypes.c_void_p, ctypes.c_size_t
    lib.droid_abi_version.restype = c_int
    lib.droid_last_error.restype = ctypes.c_char_p
    lib.droid_corr_index_forward.argtypes = [vp, vp, vp] + [c_int] * 7 + [vp]
    lib.droid_corr_index_backward.argtypes = [vp, vp, vp] + [c_int] * 7 + [vp]
    lib.droid_corr_pyramid_forward.argtypes = [ctypes.POINTER(vp), vp, vp] + [c_int] * 6 + [vp]
    lib.droid_corr_volume_pyramid.argtypes = ([vp, vp, vp, ctypes.POINTER(vp)] + [c_int] * 7
                                              + [ctypes.c_int64, ctypes.c_int64, c_int, vp])
    lib.droid_corr_pyramid_forward_slots.argtypes = ([ctypes.POINTER(vp), vp, vp, vp, c_int, ctypes.c_int64]
                                                     + [c_int] * 5 + [vp])
    lib.droid_corr_volume_pyramid_slots.argtypes = ([vp, vp, vp, ctypes.POINTER(vp), vp] + [c_int] * 7
                                                    + [ctypes.c_int64, c_int, vp])
    lib.droid_altcorr_forward.argtypes = [vp, vp, vp, vp] + [c_int] * 9 + [vp]
    lib.droid_altcorr_backward.argtypes = [vp] * 6 + [c_int] * 8 + [vp]
    lib.droid_altcorr_pyramid_forward.argtypes = [ctypes.POINTER(vp), vp, vp, vp, vp] + [c_int] * 7 + [vp]
    lib.droid_altcorr_pyramid_forward_f16.argtypes = [ctypes.POINTER(vp), vp, vp, vp, vp] + [c_int] * 7 + [vp]
    lib.droid_ba_workspace_bytes.argtypes = [c_int] * 7
    lib.droid_ba_workspace_bytes.restype = sz
    lib.droid_ba.argtypes = [vp] * 9 + [c_int] * 8 + [c_float, c_float, c_int, vp, vp, vp, sz, vp]
    lib.droid_ba_prepare.argtypes = [vp, vp] + [c_int] * 10 + [vp, sz, vp]
    lib.droid_ba_build.argtypes = [vp] * 9 + [c_int] * 8 + [vp, sz, vp]
    lib.droid_ba_build_packed.argtypes = [vp] * 9 + [c_int] * 8 + [vp, sz, vp]
    lib.droid_ba_packed_system.argtypes = [vp] + [c_int] * 7 + [ctypes.POINTER(sz)]
    lib.droid_ba_packed_system.restype = vp
    lib.droid_ba_unpack_system.argtypes = [c_int] * 8 + [vp, sz, vp]
    lib.droid_ba_solve_update.argtypes = [vp] * 6 + [c_int] * 7 + [c_float, c_float, c_int, vp, vp, vp, sz, vp]
    lib.droid_ba_overlap_available.argtypes = [c_int, c_int]
    lib.droid_ba_overlap_plan.argtypes = [c_int, c_int, c_int, ctypes.POINTER(c_int), ctypes.POINTER(sz)]
    lib.droid_ba_unpack_chunk.argtypes = [c_int] * 9 + [c_float, c_float, c_int, vp, sz, vp]
    lib.droid_ba_solve_update_overlap.argtypes = [vp] * 6 + [c_int] * 9 + [vp, vp, vp, sz, vp]
    lib.droid_ba_profile_iteration.argtypes = [vp] * 9 + [c_int] * 7 + [c_float, c_float, c_int, vp, sz, vp, vp]
    lib.droid_ba_system.argtypes = [vp] + [c_int] * 7 + [ctypes.POINTER(sz)]
    lib.droid_ba_system.restype = vp
    lib.droid_ba_status.argtypes = [vp, vp, ctypes.POINTER(c_int), ctypes.POINTER(c_int)]
    lib.droid_ba_attach_status_mirror.argtypes = [vp, vp]
    lib.droid_ba_attach_launch_hints.argtypes = [vp, vp]
    lib.droid_chol_solve.argtypes = [vp, vp, vp, c_int, vp, vp, vp]
    lib.droid_reproject_motion.argtypes = [vp, vp, vp, c_int, vp, vp, vp, c_int, c_int, c_int, c_int, vp, vp, vp, vp]
    lib.droid_chol_scratch_doubles.argtypes = [c_int]
    lib.droid_chol_scratch_doubles.restype = ctypes.c_size_t
    lib.droid_frame_distance.argtypes = [vp] * 5 + [c_int] * 4 + [c_float, vp, vp]
    lib.droid_frame_distance_matrix.argtypes = [vp] * 3 + [c_int] * 4 + [c_float, vp, vp]
    lib.droid_projmap.argtypes = [vp] * 5 + [c_int] * 4 + [vp, vp, vp]
    lib.droid_iproj.argtypes = [vp] * 3 + [c_int] * 3 + [vp, vp]
    lib.droid_depth_filter.argtypes = [vp] * 5 + [c_int] * 4 + [vp, vp]
    lib.droid_proximity_workspace_bytes.argtypes = [c_int] * 5
    lib.droid_proximity_workspace_bytes.restype = sz
    lib.droid_proximity_edges.argtypes = ([vp] + [c_int] * 7 + [c_float, c_int, c_int, vp, vp, c_int, vp, vp, c_int,
                                                                vp, c_int, vp, vp, sz, vp])
    lib.droid_cvx_upsample.argtypes = [vp] * 4 + [c_int] * 6 + [vp]
    lib.droid_graph_mean_workspace_bytes.argtypes = [c_int, c_int]
    lib.droid_graph_mean_workspace_bytes.restype = sz
    lib.droid_graph_mean.argtypes = [vp, vp, vp, c_int, ctypes.c_int64] + [c_int] * 4 + [vp, vp, sz, vp]
    lib.droid_se3_unary.argtypes = [vp, vp, ctypes.c_int64, c_int, vp]
    lib.droid_se3_mul.argtypes = [vp, c_int, vp, c_int, vp, ctypes.c_int64, vp]
    lib.droid_pose_interpolate.argtypes = [vp, vp, c_int, vp, c_int, vp, vp, vp, vp]
    lib.droid_point_cloud_workspace_bytes.argtypes = [c_int] * 3
    lib.droid_point_cloud_workspace_bytes.restype = sz
    lib.droid_point_cloud.argtypes = [vp] * 6 + [c_int] * 5 + [ctypes.c_double] + [vp] * 6 + [sz, vp]
    lib.droid_test_wave_reduce32.argtypes = [vp, vp, vp]
    for s in SYMBOLS[2:]:
        if s not in ("droid_ba_workspace_bytes", "droid_ba_system", "droid_ba_packed_system", "droid_chol_scratch_doubles",
                     "droid_proximity_workspace_bytes", "droid_graph_mean_workspace_bytes",
                     "droid_point_cloud_workspace_bytes"):
            getattr(lib, s).restype = c_int
    if lib.droid_abi_version() != 1:
        raise DroidBackendError("ABI version mismatch")
    _lib = lib
    return lib


def check(rc: int, what: str):
    if rc != 0:
        msg = load().droid_last_error().decode("utf-8", "replace")
        raise RuntimeError(f"droid_backends.{what} failed (rc={rc}): {msg}")
