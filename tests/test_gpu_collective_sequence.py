"""The sequence of collectives a rank of ShardedBA issues, in one process and without a process group: collectives that
do not match across the ranks of a group are a deadlock over RCCL, so the sequence may depend only on what every rank
shares (the overlap flag, the world size, motion_only, the system size) -- never on whether THIS rank holds edges.
torch.distributed is replaced by a recorder inside the test; no real mismatch is ever constructed (that is a hang by
design)."""
import numpy as np
import pytest

import shard_cases as sc
from util import shard_of, to_dev

pytestmark = pytest.mark.gpu


def test_every_rank_issues_the_same_collectives(backends, monkeypatch):
    """Both shards of an idle-owner graph (rank 1 owns half of the window and not one edge), 64 frames so that the
    overlap is taken, with and without it.  The recorder reports a world of 2, notes (elements, offset inside the packed
    tensor) of every all_reduce and returns at once -- it never blocks or raises, a solve may be spinning on the device.
    (Nothing is summed: rank 0 holds every edge, rank 1 solves the damping alone; both are positive definite.)

    Before the fix of ShardedBA.run the rank without edges issued ONE whole-tensor all_reduce per iteration with
    overlap=True (`use_overlap` had the rank-local term `E > 0`) while its peer issued one per chunk."""
    import torch
    import torch.distributed as dist
    from droid_backends import ba_driver
    assert torch.cuda.is_available()
    p = sc.idle_owner_graph(N=64, seed=37)
    ranges = sc.idle_owner_ranges(p)
    assert p.disps.shape == (64, 8, 16)
    iters = 2

    calls = []
    current = {}

    def all_reduce(tensor, op=None, group=None, async_op=False):
        calls.append((int(tensor.numel()), int(tensor.storage_offset() - current["be"].packed.storage_offset())))

    monkeypatch.setattr(dist, "is_initialized", lambda: True)
    monkeypatch.setattr(dist, "get_world_size", lambda group=None: 2)
    monkeypatch.setattr(dist, "all_reduce", all_reduce)

    def run(rank, overlap):
        q = shard_of(p, ranges, rank)
        d = ba_driver.BAProblemDev(**to_dev(q, torch))
        be = ba_driver.HipBackend()
        started = []
        inner = be.solve_update_overlap
        be.solve_update_overlap = lambda *a: started.append(inner(*a)) or started[-1]
        current["be"] = be
        del calls[:]
        ba_driver.ShardedBA(backend=be, overlap=overlap).run(d, p.t0, p.t1, iters, p.lm, p.ep, own=q.own)
        torch.cuda.synchronize()
        st, m = be.status()
        assert st & 15 == 0, (rank, overlap, st)
        assert m == q.eta.shape[0] > 0
        assert np.isfinite(d.poses.cpu().numpy()).all() and np.isfinite(d.disps.cpu().numpy()).all()
        return list(calls), started, len(q.ii), be.packed.numel(), be.overlap_plan()

    for overlap in (True, False):
        (seq0, started0, E0, total, plan), (seq1, started1, E1, _, _) = run(0, overlap), run(1, overlap)
        print(f"overlap={overlap}: rank 0 (E={E0}) {seq0}; rank 1 (E={E1}) {seq1}")
        assert E0 > 0 and E1 == 0
        assert seq0 == seq1, (overlap, seq0, seq1)
        if overlap:
            assert started0 == [True] * iters, started0          # the overlap was taken on the rank with edges
            assert started1 == []                                # the rank without edges cannot spin, and did not try
            assert len(plan) > 1 and seq0 == [(b - a, a) for a, b in plan] * iters
        else:
            assert started0 == [] and seq0 == [(total, 0)] * iters
