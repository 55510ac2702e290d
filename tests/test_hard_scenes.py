"""CPU proof, from the oracle alone, that the scenes of tests/hard_scenes.py do what the GPU test
(tests/test_gpu_ba_stages.py::test_hard_scene_stages_match_oracle) relies on: few pixels inside the band of MIN_DEPTH, a
decisive share of live observations behind it, every permutation of the intrinsics far outside the bars, a solvable
system with the Schur classes of the plain graph -- so that a later edit of a seed cannot turn that test vacuous.
Prints, per scene, the band count against the cap, the decisive share, the four permutation distances and the bars."""
import copy

import numpy as np
import pytest

import geom_cases as gc
import hard_scenes as hs
import stage_graphs as sg
from util import scaled_system_errors

IDS = list(hs.SCENES)
DECISIVE = 0.05         # live observations behind MIN_DEPTH, of all live observations
FAR = 100.0             # a wrong intrinsic, or a lost MIN_DEPTH branch, in units of the scene's H or b bar
SAME = 1e-6             # the same system, in the same units: the oracle sums its edges in parallel, in an order that
#                         differs from run to run, so two evaluations of one system agree to about 1e-10 of a bar


def _live(p):
    return (p.weights > 0).any(axis=1)


def _distance(oracle, q, mo, b):
    """distance of the fp64 system of `q` from the scene's, in units of the H bar and of the b bar"""
    _, H, rhs = hs.build64(oracle, q, mo)
    e = scaled_system_errors(H, rhs, b["ref"]["H"], b["ref"]["b"])
    return e["H"] / b["H"], e["b"] / b["b"]


@pytest.mark.parametrize("shape", [(9, 19), (13, 21), (8, 32), (15, 20), (16, 32), (8, 16), (48, 64)], ids=str)
def test_intrinsics_are_pairwise_apart(shape):
    K = hs.aniso_K(*shape).astype(np.float64)
    for a in range(4):
        for c in range(a):
            assert abs(K[a] - K[c]) >= 0.1 * max(K[a], K[c]), (shape, K)
    H, W = shape
    assert abs(K[2] - W / 2) > 0.05 * W and abs(K[3] - H / 2) > 0.05 * H
    Kf = hs.aniso_K_frames(H, W, 8).astype(np.float64)
    r = Kf / Kf[0]
    assert all(np.ptp(r[f]) > 5e-3 for f in range(1, 8))                   # no frame a common multiple of frame 0
    assert len({tuple(k) for k in Kf}) == 8


@pytest.mark.parametrize("sid", IDS)
def test_scene_is_decisive_discriminating_and_solvable(oracle, sid):
    sc = hs.SCENES[sid]
    p, mo = sc.problem(), sc.motion_only
    E, _, H, W = p.weights.shape
    Z, mag, _ = hs.depths(p)
    band = gc.in_z_band(Z, mag, (hs.MIN_DEPTH,))
    live = _live(p)
    assert not (live & band).any()                                         # the band rule: weight 0 on both rows
    assert band.sum() <= gc.cap(E * H * W), (int(band.sum()), gc.cap(E * H * W))
    share = float((live & (Z < hs.MIN_DEPTH)).sum() / live.sum())
    assert share >= DECISIVE, share
    assert np.isfinite(p.targets).all() and (p.weights == 0).mean() >= (0.0 if sid == "ladder" else 0.08)
    assert sid == "ladder" or float(p.disps[:p.t1].max() / p.disps[:p.t1].min()) > 10.0
    # solvable: finite, positive definite, no dead rows, the classes of the plain graph
    b = hs.bars(sid)
    ref = b["ref"]
    assert all(np.isfinite(ref[k]).all() for k in ("H", "b", "poses", "disps", "dx")) and b["e32"]["dead"] == 0
    alive = np.diag(ref["H"]) > 0
    if not alive.all():                                                    # motion_only: a new frame no kept edge enters
        plain = hs.build64(oracle, sg.GRAPHS[sid[len("hard_"):]][0](hs.synth), mo)[1]
        assert np.array_equal(alive, np.diag(plain) > 0) and alive.sum() >= 12
    assert np.abs(ref["dx"]).max() > 0
    np.linalg.cholesky(ref["A"])
    if not mo:
        assert {c for c, k in enumerate(sg.predicted_classes(p)) if k > 0} == sc.classes
    # discrimination: each permutation of the intrinsics, and the loss of the MIN_DEPTH branch (observations behind it
    # given weight 0 by hand is what a correct kernel computes: the system must not move)
    dist = {}
    for name, perm in hs.PERMUTATIONS.items():
        q = copy.copy(p)
        q.intrinsics = p.intrinsics[list(perm)]
        dist[name] = _distance(oracle, q, mo, b)
        assert max(dist[name]) >= FAR, (name, dist[name])
    q = copy.copy(p)
    q.weights = np.where((Z < hs.MIN_DEPTH)[:, None], np.float32(0), p.weights)
    assert max(_distance(oracle, q, mo, b)) < SAME
    print(f"[{sid}] band {int(band.sum())} of a cap of {gc.cap(E * H * W)}, live behind MIN_DEPTH {share:.3f}, permutations "
          + " ".join(f"{k} {max(v):.1e}" for k, v in dist.items()) + " bars")
    print(hs.bars_line(sid))


def test_ladder_rows_decide_min_depth(oracle):
    """Z sits on the levels; the rows at 0.245 are dropped by the oracle itself (zeroing them changes nothing), the rows at 0.255 are not (zeroing them moves the system by more than FAR bars)."""
    p, level = hs.ladder()
    Z, mag, _ = hs.depths(p)
    fwd = level >= 0
    assert np.abs(Z[fwd] - hs.LADDER_LEVELS[level[fwd]]).max() < 1e-6 and (Z[~fwd] >= 1.0).all()
    assert np.abs(Z - hs.MIN_DEPTH).min() > 4e-3 and not gc.in_z_band(Z, mag, (hs.MIN_DEPTH,)).any()
    assert (p.weights > 0).all() and p.t1 - p.t0 >= 2
    b = hs.bars("ladder")
    for lv, moved in ((0, False), (1, True)):
        q = copy.copy(p)
        q.weights = np.where((level == lv)[:, None], np.float32(0), p.weights)
        d = _distance(oracle, q, False, b)
        print(f"ladder: rows at Z = {hs.LADDER_LEVELS[lv]} zeroed: system moves by {d[0]:.2e} H bars, {d[1]:.2e} b bars")
        assert (max(d) > FAR) if moved else (max(d) < SAME), (lv, d)


def test_harden_keeps_what_it_says():
    from droid_backends import synth
    base = synth.make_ba_problem(N=8, E=32, H=9, W=19, seed=3, nbuf=10, t0=2)
    a, n = hs.harden(base, 5, 20.0, "plain"), hs.harden(base, 5, 20.0, "negated")
    assert np.array_equal(a.poses[:2], base.poses[:2]) and np.array_equal(a.poses[8:], base.poses[8:])
    assert not np.array_equal(a.poses[2:8], base.poses[2:8])
    assert np.array_equal(n.poses[3:8:2, 3:], -a.poses[3:8:2, 3:]) and np.array_equal(n.poses[2:8:2], a.poses[2:8:2])
    assert np.array_equal(n.poses[:, :3], a.poses[:, :3]) and np.array_equal(a.ii, base.ii) and a.eta is not base.eta
    assert np.allclose(np.linalg.norm(a.poses[:, 3:].astype(np.float64), axis=1), 1.0, atol=1e-6)
    assert np.array_equal(base.intrinsics, np.array([9.5, 9.5, 9.5, 4.5], np.float32))   # the input is not modified
