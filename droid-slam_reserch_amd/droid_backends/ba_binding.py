"""The one Python binding of the bundle adjustment's C ABI (include/droid_backends_hip.h: droid_ba and its phase API).

`BaBinding` owns what a caller of that ABI has to keep: a grow-only workspace, the page-locked words the device reports
through (status mirror, launch hints), and the dimensions of the current call.  Every droid_ba_* function is called
from exactly one method here, so its argument order -- `... t0, t1, M` for droid_ba_workspace_bytes, droid_ba_system and
droid_ba_packed_system, `... M, t0, t1` for every other one -- is written down once.  `droid_backends.ba`,
`ba_driver.HipBackend`, the stage tests and the tools all go through it.
"""
from __future__ import annotations

import ctypes
from dataclasses import dataclass

import torch

from . import _lib
from ._args import _stream


@dataclass
class BAProblemDev:
    """Device tensors of one rank, shaped like the reference's `ba` arguments (droid.cpp:88-102)."""
    poses: torch.Tensor       # [nbuf,7] f32, replicated on all ranks
    disps: torch.Tensor       # [nbuf,H,W] f32, valid for owned frames
    intrinsics: torch.Tensor  # [4]
    disps_sens: torch.Tensor  # [nbuf,H,W]
    targets: torch.Tensor     # [E_local,2,H,W]
    weights: torch.Tensor     # [E_local,2,H,W]
    eta: torch.Tensor         # [M_local,H,W]  rows = depth slots of THIS rank, ascending frame
    ii: torch.Tensor          # [E_local] int64
    jj: torch.Tensor          # [E_local] int64


def read_status(lib, workspace):
    st, m = ctypes.c_int(0), ctypes.c_int(0)
    _lib.check(lib.droid_ba_status(workspace.data_ptr(), _stream(), ctypes.byref(st), ctypes.byref(m)), "ba_status")
    return st.value, m.value


class BaBinding:
    """Workspace + pinned words + dimensions of the BA calls of one owner (one (device, stream) of `droid_backends.ba`,
    one HipBackend).  Methods enqueue on PyTorch's current stream; `p` is a BAProblemDev (any object with its fields)."""

    HINT_WORD = 4   # `mirror` words 0-3: status mirror, words 4-5: launch hints

    def __init__(self, lib=None, status_mirror=True, pinned=None, headroom=(1.25, 4096)):
        self.lib = _lib.load() if lib is None else lib
        self.buf = None
        self.headroom = headroom   # a grown workspace gets factor * bytes + extra bytes
        # {status of the last iteration, depth slots, number of iterations that ended with a violation / a stalled
        # solve so far, OR of their status bits}: written by the device only (droid_ba_attach_status_mirror), and
        # {tag of the call, its slots of Schur class 3}: written by the call's first kernel and read by the library --
        # never waited for -- when it enqueues an iteration (droid_ba_attach_launch_hints).  One tensor for the life
        # of the binding: a prepare that is still queued when the workspace grows writes into it later.
        self.mirror = torch.zeros(8, dtype=torch.int32).pin_memory() if pinned is None else pinned
        self.status_mirror = status_mirror   # False: launch hints only (the device never writes words 0-3)
        self.seen = 0      # error count of the mirror already raised / shown to the caller
        self.dims = None   # (E, nbuf, H, W, M, t0, t1) of the current call

    # ---- workspace and pinned words ---------------------------------------------------------------------------------
    def attach_hints(self, on=True):
        """Registers the launch-hint words for the workspace, or drops the registration (every launch is then made)."""
        hints = self.mirror.data_ptr() + 4 * self.HINT_WORD if on else None
        _lib.check(self.lib.droid_ba_attach_launch_hints(self.buf.data_ptr(), hints), "ba (launch hints)")

    def _attach(self, on):
        if self.status_mirror:
            _lib.check(self.lib.droid_ba_attach_status_mirror(self.buf.data_ptr(), self.mirror.data_ptr() if on else None),
                       "ba (status mirror)")
        self.attach_hints(on)

    def close(self):
        """Drops the registrations (the library keys them by workspace address) and the workspace."""
        if self.buf is not None:
            self._attach(False)
            self.buf = None

    def reserve(self, nbytes, device):
        """Grows the workspace to `nbytes`; the registrations move from the old buffer to the new one."""
        if self.buf is None or self.buf.numel() < nbytes:
            self.close()
            self.buf = torch.empty(int(nbytes * self.headroom[0]) + self.headroom[1], dtype=torch.uint8, device=device)
            self._attach(True)

    def begin(self, p, t0, t1, motion_only, device="cuda"):
        """Takes the dimensions of a call from its tensors and makes the workspace fit them; returns
        (E, nbuf, H, W, M, t0, t1).  The one droid_ba_workspace_bytes call of a `ba`."""
        nbuf, H, W = (int(x) for x in p.disps.shape)
        E, M, t0, t1 = int(p.ii.shape[0]), 0 if motion_only else int(p.eta.shape[0]), int(t0), int(t1)
        nbytes = self.lib.droid_ba_workspace_bytes(E, nbuf, H, W, t0, t1, M)
        if nbytes == 0:
            raise RuntimeError("droid_backends.ba: bad sizes / window")
        self.reserve(nbytes, device)
        self.dims = (E, nbuf, H, W, M, t0, t1)
        return self.dims

    def _ws(self):
        return self.buf.data_ptr(), self.buf.numel(), _stream()

    def _view(self, fn):
        E, nbuf, H, W, M, t0, t1 = self.dims
        nel = ctypes.c_size_t(0)
        off = fn(self.buf.data_ptr(), E, nbuf, H, W, t0, t1, M, ctypes.byref(nel)) - self.buf.data_ptr()
        return self.buf[off:off + nel.value * 8].view(torch.float64)

    def system(self):
        """The reduced camera system in the workspace: (6P+1) rows of pitch ld, flat fp64 view."""
        return self._view(self.lib.droid_ba_system)

    def packed(self):
        """Its packed copy (lower triangle + rhs row, block-column major), contiguous: what the ranks all-reduce."""
        return self._view(self.lib.droid_ba_packed_system)

    def header(self):
        """The 16 header words of the workspace (csrc/ba_internal.hpp: enum HDR_*), copied to the host (blocking)."""
        return self.buf[:64].view(torch.int32).cpu().numpy().copy()

    def status(self):
        """(status, depth_slots) of the last iteration (blocking read)."""
        return read_status(self.lib, self.buf)

    # ---- one method per function of the ABI -------------------------------------------------------------------------
    def _build_args(self, p):   # the arrays a linearisation reads, then the dimensions
        return (p.poses.data_ptr(), p.disps.data_ptr(), p.intrinsics.data_ptr(), p.disps_sens.data_ptr(), p.targets.data_ptr(),
                p.weights.data_ptr(), p.eta.data_ptr() if self.dims[4] > 0 else None, p.ii.data_ptr(), p.jj.data_ptr(), *self.dims)

    def _update_args(self, p):  # the arrays the solve + update reads, then the dimensions
        return (p.poses.data_ptr(), p.disps.data_ptr(), p.intrinsics.data_ptr(), p.weights.data_ptr(), p.ii.data_ptr(),
                p.jj.data_ptr(), *self.dims)

    def _out(self, dx, dz):
        return dx.data_ptr(), dz.data_ptr() if self.dims[4] > 0 else None

    def ba(self, p, iterations, lm, ep, motion_only, dx, dz):
        _lib.check(self.lib.droid_ba(*self._build_args(p), int(iterations), float(lm), float(ep), int(motion_only),
                                     *self._out(dx, dz), *self._ws()), "ba")

    def prepare(self, p, own, motion_only):
        _lib.check(self.lib.droid_ba_prepare(p.ii.data_ptr(), p.jj.data_ptr(), *self.dims, int(own[0]), int(own[1]),
                                             int(motion_only), *self._ws()), "ba_prepare")

    def build(self, p, motion_only, packed=False):
        fn, what = (self.lib.droid_ba_build_packed, "ba_build_packed") if packed else (self.lib.droid_ba_build, "ba_build")
        _lib.check(fn(*self._build_args(p), int(motion_only), *self._ws()), what)

    def unpack_system(self, motion_only):
        _lib.check(self.lib.droid_ba_unpack_system(*self.dims, int(motion_only), *self._ws()), "ba_unpack_system")

    def solve_update(self, p, lm, ep, motion_only, dx, dz):
        _lib.check(self.lib.droid_ba_solve_update(*self._update_args(p), float(lm), float(ep), int(motion_only),
                                                  *self._out(dx, dz), *self._ws()), "ba_solve_update")

    def overlap_available(self):
        """Whether solve_update_overlap takes a window of this size on this device: the same answer on every rank."""
        return bool(self.lib.droid_ba_overlap_available(self.dims[5], self.dims[6]))

    def overlap_plan(self, max_chunks):
        """[(first, last)] element ranges of `packed()`, one per chunk (whole block rows of the system, in order)."""
        nc = ctypes.c_int(0)
        offs = (ctypes.c_size_t * (max_chunks + 1))()
        _lib.check(self.lib.droid_ba_overlap_plan(self.dims[5], self.dims[6], max_chunks, ctypes.byref(nc), offs),
                   "ba_overlap_plan")
        return [(int(offs[c]), int(offs[c + 1])) for c in range(nc.value)]

    def unpack_chunk(self, chunk, max_chunks, lm, ep, epoch):
        _lib.check(self.lib.droid_ba_unpack_chunk(*self.dims, int(chunk), max_chunks, float(lm), float(ep), int(epoch),
                                                  *self._ws()), "ba_unpack_chunk")

    def solve_update_overlap(self, p, epoch, motion_only, dx, dz):
        """False: the single-launch solver cannot take this system (DROID_E_ARG)."""
        rc = self.lib.droid_ba_solve_update_overlap(*self._update_args(p), int(epoch), int(motion_only), *self._out(dx, dz),
                                                    *self._ws())
        if rc == -1:
            return False
        _lib.check(rc, "ba_solve_update_overlap")
        return True

    def profile_iteration(self, p, lm, ep, motion_only):
        """The 8 stage times in ms of one iteration (synchronises)."""
        ms = (ctypes.c_float * 8)()
        _lib.check(self.lib.droid_ba_profile_iteration(*self._build_args(p), float(lm), float(ep), int(motion_only),
                                                       *self._ws(), ms), "ba_profile_iteration")
        return [float(x) for x in ms]
