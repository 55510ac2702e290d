"""The table of edge-sharded BA problems the stage checker runs shard by shard (tests/test_gpu_shard_stages.py), and the
checks both that test and its CPU twin (tests/test_shard_cases.py) apply.  Every case is the smallest graph at which the
path it is named after still exists; tests/test_shard_cases.py asserts, from the host alone, the property that makes each
case decisive, so that the table cannot quietly stop covering it.

A case: the whole problem (synth.BAProblem), the frame range of every rank, the family of util.STAGE_BARS its errors are
held to, and -- where the table names them -- the Schur classes every rank's device must report."""
from dataclasses import dataclass

import numpy as np

import stage_graphs as sg
from droid_backends import ba_driver, synth
from util import STAGE_BARS, ba_args, scaled_system_errors, shard_of

H0, W0 = 8, 16          # pixels of every case that does not say otherwise
CUT_NBUF, CUT_T0 = 12, 3


@dataclass
class ShardCase:
    name: str
    problem: object           # () -> synth.BAProblem
    ranges: object            # (problem) -> [(f0, f1)] per rank
    family: str
    motion_only: bool = False
    classes: object = None    # [set per rank] the device must report, or None: printed only
    f32_room: bool = False    # H and b bars: max(family, 4 x the float32 oracle's error on the shard), see shard_bars


def _halves(p):
    return ba_driver.partition_frames(p.ii, p.t1, 2)


def cut_graph():
    """8 frames / 32 edges in a buffer of 12, window [3, 8): frames 0-2 are fixed sources, 8-11 lie past the window."""
    return synth.make_ba_problem(N=8, E=32, H=H0, W=W0, seed=31, nbuf=CUT_NBUF, t0=CUT_T0)


def idle_owner_graph(N=8, seed=32):
    """Every edge leaves a frame of the first half; the second half is observed (it is the target of edges) but owns no
    edge.  RGB-D: the disparities of the second half move by the sensor prior alone."""
    pairs = sorted({(i, j) for i in range(N // 2) for j in (i - 2, i - 1, i + 1, i + 2, i + N // 2 - 1, i + N // 2)
                    if 0 <= j < N and j != i})
    return synth.make_ba_problem(N=N, H=H0, W=W0, seed=seed, rgbd=True, edges=sg._edges(pairs))


def idle_owner_ranges(p):
    return [(0, p.t1 // 2), (p.t1 // 2, p.disps.shape[0])]


def six_frames():
    return synth.make_ba_problem(N=6, E=20, H=H0, W=W0, seed=33)


def motion_graph():
    """stage_graphs.motion_only at 8x16: the new frames [6, 10), each observed from every one of six fixed keyframes."""
    pairs = [(i, j) for i in range(6) for j in range(6, 10)]
    return synth.make_ba_problem(N=10, H=H0, W=W0, seed=7, t0=6, edges=sg._edges(pairs))


def ragged_graph():
    """20 frames, every ordered pair, 15x20 pixels: 19 edges per source and E >= 12 M on every shard, so only
    HW % 32 != 0 keeps the shards from the SYRK kernels (class 3, block pairs)."""
    N = 20
    pairs = [(i, j) for i in range(N) for j in range(N) if i != j]
    return synth.make_ba_problem(N=N, H=15, W=20, seed=34, lm=1e-4, ep=0.1, edges=sg._edges(pairs))


def _case_list():
    out = [ShardCase(f"cut_sweep[{c}]", cut_graph, lambda p, c=c: [(0, c), (c, CUT_NBUF)], "sparse")
           for c in range(CUT_NBUF + 1)]
    out += [
        ShardCase("idle_owner", idle_owner_graph, idle_owner_ranges, "sparse", classes=[{0}, {0}]),
        ShardCase("more_ranks_than_sources", six_frames, lambda p: ba_driver.partition_frames(p.ii, p.t1, 8), "sparse"),
        ShardCase("stereo", lambda: synth.make_ba_problem(N=8, E=40, H=H0, W=W0, seed=35, stereo=True), _halves, "stereo",
                  classes=[{0}, {0}]),
        ShardCase("rgbd", lambda: synth.make_ba_problem(N=8, E=32, H=H0, W=W0, seed=36, rgbd=True), _halves, "sparse",
                  classes=[{0}, {0}]),
        ShardCase("motion_only", motion_graph, lambda p: [(0, 3), (3, p.disps.shape[0])], "motion", motion_only=True,
                  classes=[{"motion"}, {"motion"}]),
        ShardCase("ragged", ragged_graph, _halves, "dense", classes=[{3}, {3}]),
        ShardCase("dense_classes", lambda: sg.every_class(synth), _halves, "dense", classes=[{0, 1, 2, 3}, {0, 1}]),
    ]
    return out


CASES = {c.name: c for c in _case_list()}
CUT_CASES = [n for n in CASES if n.startswith("cut_sweep")]


def shards(case):
    """(problem, ranges, [shard_of per rank]) of a case."""
    p = case.problem()
    ranges = [tuple(int(x) for x in r) for r in case.ranges(p)]
    return p, ranges, [shard_of(p, ranges, r) for r in range(len(ranges))]


def slot_frames(q, p):
    """Frames that hold a depth slot on the rank whose arrays `q` is (ascending)."""
    return ba_driver.local_eta_rows(q.ii, p.t0, p.t1, q.own).numpy()


def shard_classes(q):
    """The Schur classes of a shard's slots, predicted on the host (stage_graphs.predicted_classes)."""
    counts = sg.predicted_classes(q, own=q.own)
    return {c for c in range(4) if counts[c] > 0}


def is_wide(q):
    """ba_carve's decision for the arrays of one rank: dense slots go to the SYRK kernels."""
    M, E = q.eta.shape[0], len(q.ii)
    return M > 0 and E >= 12 * M and (q.disps.shape[1] * q.disps.shape[2]) % 32 == 0


def shard_bars(oracle, q, family, motion_only, f32_room=False, ref=None):
    """H and b bars of one shard's partial system: the family's (util.STAGE_BARS).  A case whose shards need more room
    (ShardCase.f32_room) takes it from the reference, the way hard_scenes.bars does: 4 x the distance of the oracle's
    own float32 evaluation of the same shard from its fp64 one where that is larger than the family's bar -- computed on
    the CPU, never from a device figure.  Returns the bars, the float32 errors and, per entry, where the bar comes
    from.  ref: the fp64 (H, b) if already built."""
    fam = STAGE_BARS[family]
    Ho, bo = ref if ref is not None else oracle.BAPhases("f64").build(*ba_args(q), q.own[0], q.own[1], motion_only)
    H32, b32 = oracle.BAPhases("f32").build(*ba_args(q), q.own[0], q.own[1], motion_only)
    e32 = scaled_system_errors(H32, b32, Ho, bo)
    bars = dict(fam)
    source = {}
    for k in ("H", "b"):
        source[k] = "f32" if f32_room and 4 * e32[k] > fam[k] else "family"
        if source[k] == "f32":
            bars[k] = 4 * e32[k]
    return bars, e32, source


def untouched_frames(before, after, slots):
    """Frames outside `slots` whose disparity map differs from the input in any bit (must be empty: a rank's
    back-substitution writes only the maps of its own slots)."""
    keep = np.ones(before.shape[0], bool)
    keep[np.asarray(slots, np.int64)] = False
    b, a = np.ascontiguousarray(before, np.float32), np.ascontiguousarray(after, np.float32)
    return [int(f) for f in np.flatnonzero(keep) if not np.array_equal(b[f].view(np.uint32), a[f].view(np.uint32))]
