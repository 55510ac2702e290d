"""Phase-level driver of the dense BA: single GPU and edge-sharded multi-GPU (one process per
GPU, torch.distributed; backend "nccl" is RCCL over xGMI on ROCm).

Sharding: the factor graph is partitioned BY SOURCE FRAME.  Rank g owns a
contiguous range of frames [f0,f1), the depth maps of those frames and every edge whose source
`ii` lies in the range.  Per Gauss-Newton iteration each rank linearises its edges and reduces its
depth frames locally (Hii/Hij/Hjj blocks, -E C^-1 E^T, rhs) into the dense (6P+1)^2 fp64 system,
ONE all-reduce(sum) of its lower triangle + rhs row (packed) combines the systems, every rank then runs the identical Cholesky solve (dx
is bit-identical on all ranks), back-substitutes its own depth frames and applies the same pose
retraction.  No other collective is on the data path; `gather_disps` optionally re-assembles the
depth maps at the end of a call.

The compute backend is pluggable so that the host logic (partition, collective, phase order) is
covered by world_size-2 gloo tests on CPU; the product backend is `HipBackend` (C ABI).
"""
from __future__ import annotations

import torch

from .ba_binding import BAProblemDev, BaBinding  # noqa: F401  (BAProblemDev: the argument of every backend method)


def partition_frames(ii, n_frames, world):
    """Contiguous frame ranges [(f0,f1)] * world balanced by outgoing-edge count (host side)."""
    ii = torch.as_tensor(ii).cpu().to(torch.int64)
    deg = torch.bincount(ii, minlength=n_frames).to(torch.float64) + 1e-3  # every frame costs a little
    csum = torch.cumsum(deg, 0)
    total = float(csum[-1])
    bounds = [0]
    for r in range(1, world):
        f = int(torch.searchsorted(csum, torch.tensor(total * r / world, dtype=torch.float64)).item()) + 1
        bounds.append(min(max(f, bounds[-1]), n_frames))
    bounds.append(n_frames)
    return [(bounds[r], bounds[r + 1]) for r in range(world)]


def local_eta_rows(ii_local, t0, t1, own):
    """Frames (ascending) that own a depth slot on this rank: unique(ii_local) U ([t0,t1) n own)."""
    w0, w1 = max(t0, own[0]), min(t1, own[1])
    fr = torch.unique(torch.cat([torch.as_tensor(ii_local).cpu().to(torch.int64),
                                 torch.arange(w0, max(w0, w1), dtype=torch.int64)]))
    return fr


class HipBackend:
    """The product compute backend: include/droid_backends_hip.h phase API on the current stream, through BaBinding
    (launch hints, no status mirror: `status()` reads the workspace)."""

    def __init__(self):
        self.binding = BaBinding(status_mirror=False, headroom=(1.0, 4096))
        self.lib, self.ws = self.binding.lib, None

    def __del__(self):
        # the library keys the launch hints by workspace address: drop the registration with the buffers it points to
        try:
            self.binding.close()
        except Exception:
            pass

    def prepare(self, p: BAProblemDev, t0, t1, own, motion_only):
        b = self.binding
        E, nbuf, H, W, M, t0, t1 = b.begin(p, t0, t1, motion_only, p.poses.device)
        self.ws = b.buf
        b.prepare(p, own, motion_only)
        self.system = b.system()
        self.packed = b.packed()   # lower triangle + rhs row, contiguous
        self.dx = torch.empty((t1 - t0, 6), dtype=torch.float32, device=p.poses.device)
        self.dz = torch.empty((M, H * W), dtype=torch.float32, device=p.poses.device)

    def build(self, p: BAProblemDev, motion_only):
        self.binding.build(p, motion_only)
        return self.system

    def build_packed(self, p: BAProblemDev, motion_only):
        """Multi-GPU build phase: the contribution of this rank lands in `self.packed` (what gets all-reduced)."""
        self.binding.build(p, motion_only, packed=True)
        return self.packed

    def unpack(self, motion_only):
        self.binding.unpack_system(motion_only)

    def solve_update(self, p: BAProblemDev, lm, ep, motion_only):
        self.binding.solve_update(p, lm, ep, motion_only, self.dx, self.dz)
        return self.dx

    # ---- overlap of the collective with the solve (opt-in: ShardedBA(overlap=True)) ----------------------------
    # chunks = collectives per iteration: each costs its own launch + synchronisation latency on the wire, so few
    OVERLAP_MAX_CHUNKS = int(__import__("os").environ.get("DROID_BA_OVERLAP_CHUNKS", "4"))

    def overlap_available(self):
        """Whether the overlap is taken for this window: decided from what every rank shares (ShardedBA.run)."""
        return self.binding.overlap_available()

    def overlap_plan(self):
        """[(first, last)] element ranges of `self.packed`, one per chunk (whole block rows of the system, in order)."""
        return self.binding.overlap_plan(self.OVERLAP_MAX_CHUNKS)

    def unpack_chunk(self, chunk, lm, ep, epoch):
        """Chunk `chunk` of the (all-reduced) packed system -> pitched matrix, damped, then published for `epoch`;
        on the current stream (the side stream of the overlap)."""
        self.binding.unpack_chunk(chunk, self.OVERLAP_MAX_CHUNKS, lm, ep, epoch)

    def solve_update_overlap(self, p: BAProblemDev, epoch, motion_only):
        """Launches the solve of iteration `epoch` BEFORE its system has been reduced: the factorisation waits for the
        block rows it is about to read.  Returns False when the single-launch solver cannot take this system."""
        return self.binding.solve_update_overlap(p, epoch, motion_only, self.dx, self.dz)

    def profile_iteration(self, p: BAProblemDev, lm, ep, motion_only):
        """Stage times in ms of one iteration (measurement support, synchronises)."""
        names = ["linearize", "assemble", "schur", "unused", "factor", "backsolve", "update", "total"]
        return dict(zip(names, self.binding.profile_iteration(p, lm, ep, motion_only)))

    def status(self):
        return self.binding.status()


class ShardedBA:
    """`iterations` Gauss-Newton steps over an edge-sharded graph.  world_size 1 degenerates to
    the single-GPU path (no collective is issued)."""

    def __init__(self, backend=None, group=None, overlap=None):
        """overlap: all-reduce the packed system in row chunks on a side stream while the factorisation, launched
        first, already works on the leading block rows (include/droid_backends_hip.h, droid_ba_overlap_plan).  Opt-in
        (default: the environment variable DROID_BA_OVERLAP=1): rehearsed with gloo and in-process shards, not yet
        measured over RCCL."""
        import os
        self.backend = backend if backend is not None else HipBackend()
        self.group = group
        self.overlap = (os.environ.get("DROID_BA_OVERLAP", "0") == "1") if overlap is None else bool(overlap)
        self._side = None

    def _world(self):
        import torch.distributed as dist
        if dist.is_available() and dist.is_initialized():
            return dist.get_world_size(self.group)
        return 1

    def run(self, p: BAProblemDev, t0, t1, iterations, lm, ep, own=None, motion_only=False):
        import torch.distributed as dist
        world = self._world()
        nbuf = int(p.disps.shape[0])
        own = (0, nbuf) if own is None else own
        be = self.backend
        be.prepare(p, t0, t1, own, motion_only)
        # Every rank of the group must issue the same collectives, so whether an iteration is cut into chunks depends
        # only on what the ranks share: the overlap flag, the world size, motion_only and the system size (through
        # overlap_available: window size, device and process-wide solver switches) -- never on the rank's own edges.
        use_overlap = self.overlap and world > 1 and hasattr(be, "solve_update_overlap") and not motion_only \
            and be.overlap_available()
        for it in range(int(iterations)):
            if use_overlap:
                packed = be.build_packed(p, motion_only)
                main = torch.cuda.current_stream()
                if self._side is None:
                    self._side = torch.cuda.Stream()
                built = torch.cuda.Event()
                built.record(main)
                # main stream: the solve waits chunk by chunk on the device.  A rank without edges cannot spin (the
                # solver scratch is preset by a build with edges): it reduces the same chunks, then solves the ordinary
                # way; so does a rank whose launch was refused after all.
                spinning = int(p.ii.shape[0]) > 0 and be.solve_update_overlap(p, it + 1, motion_only)
                with torch.cuda.stream(self._side):
                    self._side.wait_event(built)
                    for c, (a, b) in enumerate(be.overlap_plan()):
                        dist.all_reduce(packed[a:b], op=dist.ReduceOp.SUM, group=self.group)
                        if spinning:
                            be.unpack_chunk(c, lm, ep, it + 1)
                main.wait_stream(self._side)     # the next build clears the packed system
                if not spinning:
                    be.unpack(motion_only)
                    be.solve_update(p, lm, ep, motion_only)
                continue
            if world > 1 and hasattr(be, "build_packed"):
                # the build kernels add straight into the packed triangle: one collective on a contiguous tensor,
                # then ONE extra launch (unpack) in front of the solve -- no gather / scatter of the triangle
                packed = be.build_packed(p, motion_only)
                dist.all_reduce(packed, op=dist.ReduceOp.SUM, group=self.group)
                be.unpack(motion_only)
            else:
                system = be.build(p, motion_only)
                if world > 1:
                    ridx = be.reduce_index() if hasattr(be, "reduce_index") else None
                    if ridx is None:
                        dist.all_reduce(system, op=dist.ReduceOp.SUM, group=self.group)
                    else:  # only what the solve reads: lower triangle + rhs row, packed
                        flat = system.view(-1)
                        packed = flat.index_select(0, ridx)
                        dist.all_reduce(packed, op=dist.ReduceOp.SUM, group=self.group)
                        flat.index_copy_(0, ridx, packed)
            be.solve_update(p, lm, ep, motion_only)
        return be.dx

    def gather_disps(self, disps, ranges):
        """All ranks end up with every owner's depth maps (one all-reduce of the masked buffer)."""
        import torch.distributed as dist
        world = self._world()
        if world == 1:
            return disps
        rank = dist.get_rank(self.group)
        buf = torch.zeros_like(disps)
        f0, f1 = ranges[rank]
        buf[f0:f1] = disps[f0:f1]
        dist.all_reduce(buf, op=dist.ReduceOp.SUM, group=self.group)
        disps.copy_(buf)
        return disps


def shard_problem(prob, ranges, rank):
    """Host-side split of a synthetic BAProblem (numpy) into rank-local arrays."""
    import numpy as np
    f0, f1 = ranges[rank]
    keep = (prob.ii >= f0) & (prob.ii < f1)
    kx_all = np.unique(np.concatenate([np.arange(prob.t0, prob.t1), prob.ii]))
    fr = local_eta_rows(prob.ii[keep], prob.t0, prob.t1, (f0, f1)).numpy()
    rows = np.searchsorted(kx_all, fr)
    return dict(targets=prob.targets[keep], weights=prob.weights[keep], ii=prob.ii[keep], jj=prob.jj[keep],
                eta=prob.eta[rows], own=(f0, f1))
