"""CPU pins of the shard table (tests/shard_cases.py) and of the shard-aware stage checker (no GPU): for every case the
property that makes it decisive is asserted from the host alone -- an empty rank, an owner without edges whose
disparities still move, a range wholly before the window, the Schur classes of a split dense graph ... -- and the
checker passes the oracle's own float32 restatement of a shard while it fails one 6x6 block off by 1e-5 relative, one
non-zero entry in the row of a pose the shard does not touch, and one foreign disparity changed by one ulp."""
import os
import re

import numpy as np
import pytest

import shard_cases as sc
import util
from util import STAGE_BARS, ba_args, scaled_system_errors

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _shape(q):
    return len(q.ii), q.eta.shape[0]


@pytest.fixture(scope="module")
def built():
    """name -> (problem, ranges, shards), each case built once."""
    return {name: sc.shards(case) for name, case in sc.CASES.items()}


@pytest.mark.parametrize("name", list(sc.CASES))
def test_every_case_is_a_partition(oracle, built, name):
    """Ranges: a contiguous cover of the buffer.  Edges: each on exactly one rank, the one that owns its source.  Slots:
    each frame's on exactly one rank, as many as the rank has eta rows.  And the oracle's partial systems of the ranks sum
    to its unsharded system (the fp64 order of the sum is the only difference)."""
    case = sc.CASES[name]
    p, ranges, qs = built[name]
    nbuf = p.disps.shape[0]
    assert case.family in STAGE_BARS
    assert ranges[0][0] == 0 and ranges[-1][1] == nbuf and all(a[1] == b[0] for a, b in zip(ranges, ranges[1:]))
    assert sum(len(q.ii) for q in qs) == len(p.ii)
    slots = []
    for q in qs:
        assert np.all((q.ii >= q.own[0]) & (q.ii < q.own[1]))
        fr = sc.slot_frames(q, p)
        assert len(fr) == q.eta.shape[0]
        slots.append(fr)
    kx = np.unique(np.concatenate([np.arange(p.t0, p.t1), p.ii]))
    assert np.array_equal(np.sort(np.concatenate(slots)), kx)
    mo = case.motion_only
    Ho, bo = oracle.BAPhases("f64").build(*ba_args(p), 0, nbuf, mo)
    Hs, bs = np.zeros_like(Ho), np.zeros_like(bo)
    for q in qs:
        H, b = oracle.BAPhases("f64").build(*ba_args(q), q.own[0], q.own[1], mo)
        Hs += H
        bs += b
    e = scaled_system_errors(Hs, bs, Ho, bo)
    assert e["dead"] == 0 and e["stray"] == 0 and e["H"] < 1e-13 and e["b"] < 1e-13, e
    if case.classes is not None:
        assert len(case.classes) == len(qs)
        if not mo:
            assert [sc.shard_classes(q) for q in qs] == case.classes


def test_cut_sweep_covers_every_position_of_a_cut(built):
    p = sc.cut_graph()
    nbuf, t0, t1 = p.disps.shape[0], p.t0, p.t1
    assert (nbuf, t0, t1, len(p.ii)) == (sc.CUT_NBUF, sc.CUT_T0, 8, 32) and p.disps.shape[1:] == (8, 16)
    cuts = [built[n][1][0][1] for n in sc.CUT_CASES]
    assert cuts == list(range(nbuf + 1))                      # 0 and nbuf (an empty range), <= t0, inside, >= t1
    qs = [q for n in sc.CUT_CASES for q in built[n][2]]
    assert any(_shape(q) == (0, 0) for q in qs)                                   # an empty rank
    assert any(q.own[0] == q.own[1] for q in qs)                                  # ... with an empty range
    assert any(q.own[1] > q.own[0] and _shape(q) == (0, 0) for q in qs)           # ... with a range past the window
    assert any(q.eta.shape[0] > 0 and q.ii.max() < t0 for q in qs)                # slots from edges only, fixed sources
    assert any(q.own[0] < t0 < q.own[1] < t1 for q in qs)                         # a range cut by t0
    assert any(t0 < q.own[0] < t1 <= q.own[1] for q in qs)                        # ... and by t1


def test_idle_owner_moves_by_the_prior_alone(oracle, built):
    """Rank 1 owns window frames and no edge; the oracle moves every one of its disparity maps by more than 100 x the
    state bar, so "left untouched" and "correct" are different outcomes."""
    case = sc.CASES["idle_owner"]
    p, ranges, qs = built["idle_owner"]
    assert np.all(p.ii < p.t1 // 2) and np.any(p.disps_sens > 0)
    assert _shape(qs[1])[0] == 0 and _shape(qs[1])[1] > 0
    fr = sc.slot_frames(qs[1], p)
    assert np.all((fr >= max(p.t0, ranges[1][0])) & (fr < p.t1))
    Ho, bo = oracle.BAPhases("f64").build(*ba_args(p), 0, p.disps.shape[0], False)
    ph = oracle.BAPhases("f64")
    H1, b1 = ph.build(*ba_args(qs[1]), *qs[1].own, False)
    assert not H1.any() and not b1.any()                      # it contributes nothing to the camera system
    _, disps, _ = ph.finish(Ho, bo, float(np.float32(p.lm)), float(np.float32(p.ep)))
    move = np.abs(disps - p.disps).reshape(p.disps.shape[0], -1).max(axis=1)
    assert np.all(move[fr] > 100 * STAGE_BARS[case.family]["state"]), move[fr]
    keep = np.ones(len(move), bool)
    keep[fr] = False
    assert not move[keep].any()


def test_more_ranks_than_sources_has_empty_ranges(built):
    p, ranges, qs = built["more_ranks_than_sources"]
    assert p.t1 == 6 and len(ranges) == 8
    assert any(a == b for a, b in ranges) and any(_shape(q) == (0, 0) for q in qs)
    assert sum(len(q.ii) > 0 for q in qs) >= 2


def test_stereo_pairs_land_on_their_owner(built):
    p, ranges, qs = built["stereo"]
    assert int((p.ii == p.jj).sum()) == p.t1
    for q in qs:
        pair = q.ii[q.ii == q.jj]
        assert len(pair) > 0 and np.array_equal(np.sort(pair), np.arange(max(q.own[0], 0), min(q.own[1], p.t1)))


def test_rgbd_and_motion_only_ranks_all_hold_edges(built):
    p, ranges, qs = built["rgbd"]
    for q in qs:
        assert len(q.ii) > 0 and np.any(p.disps_sens[q.own[0]:q.own[1]] > 0)
    p, ranges, qs = built["motion_only"]
    assert sc.CASES["motion_only"].motion_only and all(len(q.ii) > 0 for q in qs)
    assert np.all(p.ii < p.t0) and np.all((p.jj >= p.t0) & (p.jj < p.t1))


def _constants():
    src = "".join(open(os.path.join(ROOT, "droid-slam_reserch_amd", "csrc", f)).read()
                  for f in ("ba_kernels.hip", "ba_internal.hpp"))
    return {k: int(re.search(r"constexpr int %s = (\d+);" % k, src).group(1))
            for k in ("S2_MAXE", "SW_MID", "SW_BIG", "SLOT_MAXE")}


def test_dense_shards_keep_every_schur_class(built):
    """From the edge counts per source against the kernels' own constants: the two halves of the every-class graph
    still hold classes 0-3 between them and stay wide; the ragged graph would be wide but for HW % 32."""
    import stage_graphs as sg
    k = _constants()
    classes = lambda q: {c for c, cnt in enumerate(sg.predicted_classes(q, own=q.own, **k)) if cnt > 0}
    p, ranges, qs = built["dense_classes"]
    assert len(qs) == 2 and set().union(*(classes(q) for q in qs)) == {0, 1, 2, 3}
    assert any(sc.is_wide(q) for q in qs)
    assert [classes(q) for q in qs] == sc.CASES["dense_classes"].classes
    p, ranges, qs = built["ragged"]
    assert p.disps.shape[1:] == (15, 20) and (15 * 20) % 32 != 0
    for q in qs:
        E, M = _shape(q)
        assert E >= 12 * M and not sc.is_wide(q)              # dense enough: only the pixel count keeps it narrow
        assert np.bincount(q.ii)[q.own[0]:].min() > k["S2_MAXE"] and classes(q) == {3}


# ---- the checker -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,rank", [("rgbd", 0), ("rgbd", 1), ("ragged", 0)])
def test_checker_passes_fp32_and_fails_a_wrong_block(oracle, built, name, rank):
    case = sc.CASES[name]
    q = built[name][2][rank]
    Ho, bo = oracle.BAPhases("f64").build(*ba_args(q), *q.own, False)
    H32, b32 = oracle.BAPhases("f32").build(*ba_args(q), *q.own, False)
    bars, e32, source = sc.shard_bars(oracle, q, case.family, False, case.f32_room, ref=(Ho, bo))
    print(f"[{name} rank {rank}] fp32 oracle: H {e32['H']:.2e} b {e32['b']:.2e}, bars {bars['H']:.2e} {bars['b']:.2e} {source}")
    util.assert_system_close(e32, bars, name)

    # the off-diagonal block that is largest against its diagonal, scaled by 1 + 1e-5
    n = Ho.shape[0]
    P = n // 6
    live = np.diag(Ho) > 0
    s = np.where(live, 1.0 / np.sqrt(np.where(live, np.diag(Ho), 1.0)), 0.0)
    blk = (np.abs(np.tril(Ho)) * s[:, None] * s[None, :]).reshape(P, 6, P, 6).max(axis=(1, 3))
    blk[np.triu_indices(P)] = 0
    a, b = np.unravel_index(np.argmax(blk), blk.shape)
    assert blk[a, b] >= 0.18, blk[a, b]
    bad = H32.copy()
    bad[6 * a:6 * a + 6, 6 * b:6 * b + 6] *= 1 + 1e-5
    e = scaled_system_errors(bad, b32, Ho, bo)
    assert e["H"] >= bars["H"], (name, e["H"], bars["H"])
    with pytest.raises(AssertionError):
        util.assert_system_close(e, bars, name)


def test_checker_rejects_a_write_into_a_pose_the_shard_does_not_touch(oracle, built):
    """cut_sweep, cut at 7: rank 1 holds the edges of frame 7 alone; the rows of every pose they do not reach are exactly
    zero in the oracle's partial system, and one entry of 1e-30 there fails."""
    q = built["cut_sweep[7]"][2][1]
    Ho, bo = oracle.BAPhases("f64").build(*ba_args(q), *q.own, False)
    dead = np.flatnonzero(np.diag(Ho) == 0)
    assert len(q.ii) > 0 and len(dead) >= 6 and np.diag(Ho).max() > 0
    assert scaled_system_errors(Ho.copy(), bo, Ho, bo)["dead"] == 0
    bad = Ho.copy()
    d, l = int(dead[-1]), int(np.flatnonzero(np.diag(Ho) > 0)[0])
    bad[max(d, l), min(d, l)] = 1e-30                         # lower triangle: the dead row or the dead column
    e = scaled_system_errors(bad, bo, Ho, bo)
    assert e["dead"] == 1 and e["H"] == 0.0
    with pytest.raises(AssertionError):
        util.assert_system_close(e, STAGE_BARS["sparse"], "dead row")
    badb = bo.copy()
    badb[dead[0]] = -1e-30
    assert scaled_system_errors(Ho, badb, Ho, bo)["dead"] == 1


def test_checker_rejects_one_ulp_in_a_foreign_disparity_map(built):
    p, ranges, qs = built["rgbd"]
    q = qs[0]
    slots = sc.slot_frames(q, p)
    foreign = [f for f in range(p.disps.shape[0]) if f not in set(slots.tolist())]
    assert foreign
    after = p.disps.copy()
    after[slots] += 0.01                                      # its own maps may move
    assert sc.untouched_frames(p.disps, after, slots) == []
    f = foreign[-1]
    after[f, 3, 5] = np.nextafter(after[f, 3, 5], np.float32(np.inf))
    assert sc.untouched_frames(p.disps, after, slots) == [f]


def test_a_rank_without_edges_and_slots_passes_the_host_checks(backends):
    """E == 0 and M == 0 (an empty or foreign range) is a legal rank of the phase API: the argument checks, all on the
    host and ahead of any HIP call, let it through to the workspace check (a 1-byte workspace: DROID_E_WORKSPACE); no
    slot although there are edges stays an argument error, and so does the single-GPU entry without eta rows."""
    import ctypes
    lib = backends._lib.load()
    ws = ctypes.create_string_buffer(64)
    prepare = lambda E, M, mo: lib.droid_ba_prepare(None, None, E, 12, 8, 16, M, 3, 8, 8, 12, mo, ctypes.addressof(ws), 1, None)
    assert prepare(0, 0, 0) == -2 and b"workspace" in lib.droid_last_error()
    assert lib.droid_ba_unpack_system(0, 12, 8, 16, 0, 3, 8, 0, ctypes.addressof(ws), 1, None) == -2
    assert prepare(5, 0, 0) == -1 and b"eta has no rows" in lib.droid_last_error()
    assert prepare(5, 0, 1) == -2                                      # motion-only: never a slot
    rc = lib.droid_ba(None, None, None, None, None, None, None, None, None, 0, 12, 8, 16, 0, 3, 8, 1, 1e-4, 0.1, 0,
                      None, None, ctypes.addressof(ws), 1, None)
    assert rc == -1 and b"eta has no rows" in lib.droid_last_error()
    assert lib.droid_ba_workspace_bytes(0, 12, 8, 16, 3, 8, 0) > 0
