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

# One entry per function of include/droid_backends_hip.h, in the header's argument order: (result, arguments).  A run of
# equal arguments is written with its count ("3p 7i p" = three pointers, seven ints, one pointer).
#   i int   l int64_t   z size_t   f float   d double   p pointer to data (or an opaque handle: workspace, stream)
#   P array of pointers (pyramid levels)   I int* result   Z size_t* result   s const char*
# tests/test_abi.py holds every entry against the header's prototype.
ABI = {
    "droid_abi_version": ("i", ""),
    "droid_last_error": ("s", ""),
    "droid_corr_index_forward": ("i", "3p 7i p"),
    "droid_corr_index_backward": ("i", "3p 7i p"),
    "droid_corr_pyramid_forward": ("i", "P 2p 6i p"),
    "droid_corr_volume_pyramid": ("i", "3p P 7i 2l i p"),
    "droid_corr_pyramid_forward_slots": ("i", "P 3p i l 5i p"),
    "droid_corr_volume_pyramid_slots": ("i", "3p P p 7i l i p"),
    "droid_altcorr_forward": ("i", "4p 9i p"),
    "droid_altcorr_backward": ("i", "6p 8i p"),
    "droid_altcorr_pyramid_forward": ("i", "P 4p 7i p"),
    "droid_altcorr_pyramid_forward_f16": ("i", "P 4p 7i p"),
    "droid_ba_workspace_bytes": ("z", "7i"),
    "droid_ba": ("i", "9p 8i 2f i 3p z p"),
    "droid_ba_prepare": ("i", "2p 10i p z p"),
    "droid_ba_build": ("i", "9p 8i p z p"),
    "droid_ba_build_packed": ("i", "9p 8i p z p"),
    "droid_ba_packed_system": ("p", "p 7i Z"),
    "droid_ba_unpack_system": ("i", "8i p z p"),
    "droid_ba_overlap_available": ("i", "2i"),
    "droid_ba_overlap_plan": ("i", "3i I Z"),
    "droid_ba_unpack_chunk": ("i", "9i 2f i p z p"),
    "droid_ba_solve_update_overlap": ("i", "6p 9i 3p z p"),
    "droid_ba_solve_update": ("i", "6p 7i 2f i 3p z p"),
    "droid_ba_profile_iteration": ("i", "9p 7i 2f i p z 2p"),
    "droid_ba_system": ("p", "p 7i Z"),
    "droid_ba_status": ("i", "2p 2I"),
    "droid_ba_attach_status_mirror": ("i", "2p"),
    "droid_ba_attach_launch_hints": ("i", "2p"),
    "droid_chol_solve": ("i", "3p i 3p"),
    "droid_chol_scratch_doubles": ("z", "i"),
    "droid_reproject_motion": ("i", "3p i 3p 4i 4p"),
    "droid_frame_distance": ("i", "5p 4i f 2p"),
    "droid_frame_distance_matrix": ("i", "3p 4i f 2p"),
    "droid_projmap": ("i", "5p 4i 3p"),
    "droid_iproj": ("i", "3p 3i 2p"),
    "droid_depth_filter": ("i", "5p 4i 2p"),
    "droid_proximity_workspace_bytes": ("z", "5i"),
    "droid_proximity_edges": ("i", "p 7i f 2i 2p i 2p i p i 2p z p"),
    "droid_cvx_upsample": ("i", "4p 6i p"),
    "droid_graph_mean_workspace_bytes": ("z", "2i"),
    "droid_graph_mean": ("i", "3p i l 4i 2p z p"),
    "droid_se3_unary": ("i", "2p l i p"),
    "droid_se3_mul": ("i", "p i p i p l p"),
    "droid_pose_interpolate": ("i", "2p i p i 4p"),
    "droid_point_cloud_workspace_bytes": ("z", "3i"),
    "droid_point_cloud": ("i", "6p 5i d 6p z p"),
    "droid_test_wave_reduce32": ("i", "3p"),
}
SYMBOLS = list(ABI)   # tests check that the library exports them all and the header declares no other
# The second header, include/droid_update_hip.h, in the same notation (tests/test_ba_inputs_abi.py holds it against the
# prototypes there).  The same library exports these; load() binds both tables.
ABI_UPDATE = {
    "droid_ba_inputs_workspace_bytes": ("z", "3i"),
    "droid_ba_inputs": ("i", "11p 9i f 6p i 3p i 2p z p"),
}
SYMBOLS_UPDATE = list(ABI_UPDATE)
# include/droid_corr_encode_hip.h, the prototypes of the contract stated in droid_update_hip.h (tests/test_corr_encode_abi.py
# holds the table against them).  A table of its own because tests/test_ba_inputs_abi.py pins ABI_UPDATE at its two entries.
ABI_CORR_ENCODE = {
    "droid_corr_encode_packed_bytes": ("z", ""),
    "droid_corr_encode": ("i", "P 4p i l 7i p"),
}
SYMBOLS_CORR_ENCODE = list(ABI_CORR_ENCODE)
# include/droid_motion_encode_hip.h, contract and prototypes (tests/test_motion_encode_abi.py holds the table against
# them).  A table of its own for the same reason: tests/test_corr_encode_abi.py pins ABI_CORR_ENCODE at its two entries.
ABI_MOTION_ENCODE = {
    "droid_motion_encode_packed_bytes": ("z", ""),
    "droid_motion_encode": ("i", "3p i 8p 5i p"),
}
SYMBOLS_MOTION_ENCODE = list(ABI_MOTION_ENCODE)
# include/droid_heads_hip.h, contract and prototypes (tests/test_update_heads_abi.py holds the table against them).  A
# table of its own once more: tests/test_motion_encode_abi.py pins ABI_MOTION_ENCODE at its two entries.  The arrays of
# a call are "P" (the pointers of the heads) and "I" (n_out, act: one int per head).
ABI_HEADS = {
    "droid_head_packed_bytes": ("z", "i"),
    "droid_update_heads": ("i", "3P 2I 5i p"),
}
SYMBOLS_HEADS = list(ABI_HEADS)
# include/droid_conv3x3_hip.h, contract and prototypes (tests/test_conv3x3_abi.py holds the table against them).  A table
# of its own again: tests/test_update_heads_abi.py pins ABI_HEADS at its two entries.
ABI_CONV3X3 = {
    "droid_conv3x3_packed_bytes": ("z", "2i"),
    "droid_conv3x3": ("i", "3p 5i 3l 2i p"),
}
SYMBOLS_CONV3X3 = list(ABI_CONV3X3)
# include/droid_gru_hip.h, contract and prototypes (tests/test_conv_gru_abi.py holds the table against them).  A table of
# its own: tests/test_conv3x3_abi.py pins ABI_CONV3X3 at its two entries.  The segment table of a call is "P" (the
# pointers), "L" (const int64_t*: the batch strides) and "I" (the channels).
ABI_GRU = {
    "droid_gru_packed_bytes": ("z", "i"),
    "droid_gru_workspace_bytes": ("z", "3i"),
    "droid_gru_context": ("i", "p l p 4i 2p z p"),
    "droid_gru_gates": ("i", "P L I i 4p 3i p"),
    "droid_gru_update": ("i", "P L I i 4p l p l 3i p"),
    "droid_conv_gru": ("i", "P L I i 2p l 3i p z p"),
}
SYMBOLS_GRU = list(ABI_GRU)
# The test hooks, include/droid_test_hooks_hip.h (tests/test_gpu_lin_pinned.py holds the table against the prototypes).
# A table and a header of their own: the main header is the drop-in boundary and tests/test_abi.py pins its 48
# prototypes, so a hook that only the tests need is not added there.  load() binds a hook where the library exports it
# and requires none: a build from before a hook existed still loads through DROID_HIP_LIB (tools/ab_test.sh,
# tools/update_bits.py).
ABI_TEST = {
    "droid_test_ba_lin": ("i", "9p 9i p z 4p Z p"),
}
SYMBOLS_TEST = list(ABI_TEST)
_CTYPE = {"i": ctypes.c_int, "l": ctypes.c_int64, "z": ctypes.c_size_t, "f": ctypes.c_float, "d": ctypes.c_double,
          "p": ctypes.c_void_p, "P": ctypes.POINTER(ctypes.c_void_p), "I": ctypes.POINTER(ctypes.c_int),
          "Z": ctypes.POINTER(ctypes.c_size_t), "s": ctypes.c_char_p, "L": ctypes.POINTER(ctypes.c_int64)}


def signature(name):
    """(restype, argtypes) of an entry of ABI, ABI_UPDATE, ABI_CORR_ENCODE, ABI_MOTION_ENCODE, ABI_HEADS, ABI_CONV3X3, ABI_GRU
    or ABI_TEST as ctypes types."""
    for table in (ABI, ABI_TEST, ABI_CORR_ENCODE, ABI_MOTION_ENCODE, ABI_HEADS, ABI_CONV3X3, ABI_GRU):
        if name in table:
            break
    else:
        table = ABI_UPDATE
    res, args = table[name]
    return _CTYPE[res], [_CTYPE[run[-1]] for run in args.split() for _ in range(int(run[:-1] or 1))]


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
    for s in (SYMBOLS + SYMBOLS_UPDATE + SYMBOLS_CORR_ENCODE + SYMBOLS_MOTION_ENCODE + SYMBOLS_HEADS + SYMBOLS_CONV3X3
              + SYMBOLS_GRU + SYMBOLS_TEST):
        if not hasattr(lib, s):
            if s in SYMBOLS_TEST:
                continue
            raise DroidBackendError(f"{LIB_PATH} does not export {s}")
        fn = getattr(lib, s)
        fn.restype, fn.argtypes = signature(s)
    if lib.droid_abi_version() != 1:
        raise DroidBackendError("ABI version mismatch")
    _lib = lib
    return lib


def check(rc: int, what: str):
    if rc != 0:
        msg = load().droid_last_error().decode("utf-8", "replace")
        raise RuntimeError(f"droid_backends.{what} failed (rc={rc}): {msg}")
