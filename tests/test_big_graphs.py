"""CPU proof, from the oracle alone, that the scenes of tests/big_graphs.py reach the code they are there for and that
this code decides the result -- so that tests/test_gpu_ba_big_graphs.py cannot pass a kernel that drops a metadata chunk,
and a later edit of a seed cannot turn it vacuous.  Prints, per hub scene, the share of live weights of every chunk and
the distance, in bars, by which the fp64 system moves when one chunk's weights are zeroed."""
import numpy as np
import pytest

import big_graphs as bg
import hard_scenes as hs
import stage_graphs as sg
from util import scaled_system_errors

LIVE_SHARE = 0.85       # of a chunk's weights, positive
FAR = 1000.0            # a dropped chunk, in units of the scene's H bar and of its b bar


def _distance(oracle, q, b):
    """distance of the fp64 system of `q` from the scene's, in units of the H bar and of the b bar"""
    _, H, rhs = hs.build64(oracle, q, False)
    e = scaled_system_errors(H, rhs, b["ref"]["H"], b["ref"]["b"])
    return e["H"] / b["H"], e["b"] / b["b"]


@pytest.mark.parametrize("sid", list(bg.SCENES))
def test_scene_is_the_one_of_the_table(sid):
    sc = bg.SCENES[sid]
    p = sc.problem()
    nbuf, H, W = p.disps.shape
    assert len(p.ii) == sc.E and len(set(zip(p.ii.tolist(), p.jj.tolist()))) == sc.E
    assert tuple(sg.predicted_classes(p)) == sc.counts, (tuple(sg.predicted_classes(p)), sc.counts)
    assert p.eta.shape[0] == sum(sc.counts)
    assert bg.zsplit_of(p) == sc.zsplit
    deg = np.bincount(p.ii, minlength=nbuf)
    assert {int(f): int(deg[f]) for f in np.flatnonzero(deg > 100)} == sc.hubs
    if sc.ints is not None:
        assert bg.prep_ints(nbuf, sc.E) == sc.ints
        assert (sc.ints <= bg.PREP_LDS_INTS) == (sid == "prep_lds_limit")


def test_prep_threshold_is_met_exactly():
    """prep_lds_limit fills the 150 KB of dynamic LDS to the int; one edge more, or one frame more, is past it; the
    largest graph of the other suites (256 frames, 8000 edges) is below."""
    assert bg.PREP_LDS_INTS == 38400 == bg.prep_ints(1022, 7295)
    assert bg.prep_ints(1022, 7296) == 38404 and bg.prep_ints(1023, 7295) == 38409 and bg.prep_ints(4400, 40) == 39782
    assert bg.prep_ints(256, 8000) == 34326 and bg.prep_ints(1024, 7300) > bg.PREP_LDS_INTS


def test_edge_ranges_cross_and_start_inside_chunks():
    p = bg.HUBS["hub160"].problem()
    r = bg.edge_ranges(159, bg.zsplit_of(p))
    assert (120, 140) in r and (140, 159) in r and len(r) == 8 and all(b - a == 20 for a, b in r[:-1])
    assert bg.edge_ranges(128, 8) == [(16 * k, 16 * k + 16) for k in range(8)]
    assert bg.edge_ranges(129, 8)[-1] == (119, 129)                    # 17 per range: the last one crosses 128
    q = bg.HUBS["hub262"].problem()
    r = bg.edge_ranges(261, bg.zsplit_of(q))
    assert r == [(0, 53), (53, 106), (106, 159), (159, 212), (212, 261)]
    assert any(a < 128 < b for a, b in r) and any(a < 256 < b for a, b in r)
    assert bg.edge_ranges(256, 5)[2] == (104, 156) and bg.edge_ranges(256, 5)[-1] == (208, 256)
    assert bg.zsplit_of(bg.HUBS["hub160_z1"].problem()) == 1 and 160 * 5 > bg.LIN_WGS // 2
    assert bg.edge_ranges(5, 8) == [(k, k + 1) for k in range(5)]      # empty ranges are left out


def test_entry_base_of_the_second_chunk_is_not_its_edge_offset():
    """Thirty targets of hub 40's first chunk lie before t0: with the self row, the entries of its second chunk start at
    1 + 98, not at 1 + 128 -- and not at 1, what a chunk loop that forgot to carry the base would use."""
    p = bg.HUBS["hub160"].problem()
    first = bg.chunks(p, 40)[0]
    assert len(first) == 128 and np.array_equal(p.jj[first], [j for j in range(129) if j != 40])
    assert int((p.jj[first] < p.t0).sum()) == 30
    wide = bg.HUBS["hub160_wide"].problem()
    e = bg.hub_edges(wide, 40)
    assert int(np.flatnonzero(wide.jj[e] == 40)[0]) == 40 and len(e) == 160        # the stereo edge, in the first chunk


@pytest.mark.parametrize("sid", list(bg.HUBS))
def test_every_chunk_decides_the_system(oracle, sid):
    sc = bg.HUBS[sid]
    p = sc.problem()
    b = bg.bars(sid)
    assert b["e32"]["dead"] == 0 and (np.diag(b["ref"]["H"]) > 0).all()
    np.linalg.cholesky(b["ref"]["A"])
    print(bg.bars_line(sid))
    for f, ne in sc.hubs.items():
        if ne <= bg.SLOT_MAXE:
            assert len(bg.chunks(p, f)) == 1
            continue
        for c, edges in enumerate(bg.chunks(p, f)):
            share = float((p.weights[edges] > 0).mean())
            d = _distance(oracle, bg.without(p, edges), b)
            print(f"[{sid}] hub {f} chunk {c} ({len(edges)} edges): live {share:.3f}, zeroed: H {d[0]:.2e} b {d[1]:.2e} bars")
            assert share >= LIVE_SHARE, (f, c, share)
            assert min(d) >= FAR, (f, c, d)


def test_plain_hub_has_a_dead_tail(oracle):
    """The reason for `hover`: on the generator's drifting trajectory the second chunk of hub 40 carries nothing."""
    sc, plain = bg.HUBS["hub160"], bg.scene("hub160_plain").problem()
    assert np.array_equal(plain.ii, sc.problem().ii) and np.array_equal(plain.jj, sc.problem().jj)
    b = bg.bars("hub160_plain")
    tail = bg.chunks(plain, 40)[1]
    share = float((plain.weights[tail] > 0).mean())
    d = _distance(oracle, bg.without(plain, tail), b)
    print(f"[hub160, plain] hub 40 chunk 1: live {share:.3f}, zeroed: H {d[0]:.2e} b {d[1]:.2e} bars")
    assert share < 0.01 and max(d) < 1.0, (share, d)


def test_hover_keeps_what_it_says():
    sc = bg.HUBS["hub262"]
    plain = bg.plain_hub(*bg.HUB262)
    before = plain.poses.copy()
    p = bg.hover(plain, 700)
    assert np.array_equal(plain.poses, before)                                             # the input is not modified
    assert np.array_equal(p.poses, sc.problem().poses) and np.array_equal(p.weights, sc.problem().weights)
    assert np.array_equal(p.poses[0], [0, 0, 0, 0, 0, 0, 1]) and p.poses.dtype == np.float32
    assert np.allclose(np.linalg.norm(p.poses[:, 3:].astype(np.float64), axis=1), 1.0, atol=1e-6)
    assert np.abs(p.poses[1:, :3]).max() < 0.3 and 0.01 < p.poses[1:, :3].std() < 0.1
    assert np.array_equal(p.disps, plain.disps) and np.array_equal(p.intrinsics, plain.intrinsics)
    assert np.array_equal(p.eta, plain.eta) and not np.array_equal(p.targets, plain.targets)


def test_appended_frame_is_unused():
    p = bg.PREPS["prep_lds_limit"].problem()
    q = bg.appended_frame(p)
    assert q.poses.shape[0] == q.disps.shape[0] == q.disps_sens.shape[0] == 1023
    assert bg.prep_ints(1023, len(q.ii)) == 38409 and q.ii is p.ii and q.eta is p.eta and (q.t0, q.t1) == (p.t0, p.t1)
    assert np.array_equal(q.poses[:1022], p.poses) and p.poses.shape[0] == 1022
