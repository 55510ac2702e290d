"""GPU checks of droid_proximity_edges / backends.proximity_edges: EXACT equality of the whole edge list, order
included, with the host restatement (tests/proximity_ref.py) fed the same fp32 matrix copied back from the device.
Integer results: no tolerance anywhere.

Every non-degenerate case asserts, on the restatement's own statistics, that it accepts at least 8 pairs in the walk,
and the cases that exist for one mechanism (suppression by an earlier accept, by a listed edge, the max_factors stop,
the known-edge filter) assert that the mechanism fired."""
import ctypes

import numpy as np
import pytest

import proximity_ref as pr

pytestmark = pytest.mark.gpu

BETA = 0.25


def _torch():
    import torch
    return torch


def _dev(a):
    torch = _torch()
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _lists(edges):
    e = np.asarray(edges, np.int64).reshape(-1, 2)
    return _dev(e[:, 0].copy()), _dev(e[:, 1].copy())


def _gpu(backends, dist_t, t, t0, t1, rad, nms, thresh, mf, stereo, sup, known=None):
    """The product, on a directed device matrix."""
    si, sj = _lists(sup)
    ki, kj = _lists(known) if known is not None else (None, None)
    ii, jj = backends.proximity_edges(None, None, None, t, t0, t1, rad, nms, BETA, thresh, mf, stereo, si, sj, ki, kj,
                                      dist=dist_t)
    assert ii.dtype == _torch().int64 and ii.is_cuda and ii.shape == jj.shape
    return np.stack([ii.cpu().numpy(), jj.cpu().numpy()], 1)


def _check(backends, dist, t, t0, t1, rad, nms, thresh, mf, stereo, sup=(), known=None, min_accept=8):
    """Run one case both ways; returns (edges, stats of the restatement)."""
    dist_t = dist if hasattr(dist, "is_cuda") else _dev(np.asarray(dist, np.float32))
    sup = [tuple(e) for e in np.asarray(sup, np.int64).reshape(-1, 2).tolist()]
    st = {}
    want = pr.proximity_edges(dist_t.cpu().numpy(), t, t0, t1, rad, nms, thresh, mf, stereo, sup, known, stats=st)
    got = _gpu(backends, dist_t, t, t0, t1, rad, nms, thresh, mf, stereo, sup, known)
    print(f"t={t} t0={t0} t1={t1} rad={rad} nms={nms} thresh={thresh} mf={mf} stereo={stereo} sup={len(sup)} "
          f"known={0 if known is None else len(known)}: {st} -> {len(want)} edges, device {len(got)}")
    assert st.get("accepted", 0) >= min_accept, ("badly chosen input", st)
    assert got.shape == want.shape, (got.shape, want.shape)
    bad = np.flatnonzero((got != want).any(1))
    assert bad.size == 0, (bad[:5], got[bad[:5]], want[bad[:5]])
    return want, st


# ------------------------------------------------------------------------------------------ synthetic matrices
@pytest.mark.parametrize("nms", [0, 1, 2, 3])
@pytest.mark.parametrize("rad", [1, 2, 3])
def test_random_distinct_backend_shape(backends, nms, rad):
    d = pr.random_symmetric(100, 10 * nms + rad)   # 100: not a multiple of 32 or 64
    _, st = _check(backends, d, 100, 0, 0, rad, nms, 20.0, 10000, False)
    assert nms == 0 or st["suppressed"] > 0        # (i) an earlier accept of the same call masks a candidate


@pytest.mark.parametrize("stereo", [False, True])
@pytest.mark.parametrize("t,t0,t1,rad,nms", [(100, 95, 75, 2, 1), (77, 72, 52, 1, 0), (131, 120, 97, 3, 2), (61, 40, 0, 2, 3)])
def test_random_distinct_frontend_shape(backends, stereo, t, t0, t1, rad, nms):
    d = pr.random_symmetric(t, t + int(stereo))
    _check(backends, d, t, t0, t1, rad, nms, 30.0, 10000, stereo)


def test_banded_trajectory_with_loop_closures(backends):
    d = pr.banded(256, 1)
    _, st = _check(backends, d, 256, 0, 0, 2, 3, 22.0, 4096, False)
    assert st["forced"] == 1524 and st["accepted"] >= 100 and st["suppressed"] >= 500
    _check(backends, d, 256, 0, 0, 2, 3, 22.0, 4096, True)
    _check(backends, pr.banded(203, 2, slope=0.8), 203, 198, 178, 2, 1, 16.0, 48, False)   # the frontend's call


@pytest.mark.parametrize("t,t0,t1", [(90, 0, 0), (90, 60, 31)])
def test_exact_ties_follow_the_flat_index(backends, t, t0, t1):
    d = pr.with_ties(t, 4)
    for nms in (0, 2):
        _check(backends, d, t, t0, t1, 1, nms, 10.0, 10000, False)
    z = np.zeros((t, t), np.float32)
    z[::2] = -0.0                                    # +0 and -0 are one value
    _check(backends, z, t, t0, t1, 2, 1, 1.0, 10000, False)


def test_all_far_gives_forced_edges_only(backends):
    d = np.full((70, 70), 1000.0, np.float32)
    for stereo in (False, True):
        want, st = _check(backends, d, 70, 0, 0, 2, 2, 16.0, 10000, stereo, min_accept=0)
        assert st["accepted"] == 0 and len(want) == pr.forced_count(70, 0, 2, stereo)
    d = pr.random_symmetric(70, 3)
    d[5, 40] = d[40, 5] = np.nan
    d[6, 41] = np.inf
    want, st = _check(backends, d, 70, 0, 0, 2, 2, 16.0, -1, False, min_accept=0)   # the FactorGraph default
    assert st["accepted"] == 0 and len(want) == pr.forced_count(70, 0, 2, False)
    _check(backends, d, 70, 0, 0, 2, 0, 50.0, 10000, False)                       # NaN / inf cells are never selected


@pytest.mark.parametrize("t,t0,t1,rad,stereo", [(1, 0, 0, 2, False), (1, 0, 0, 2, True), (2, 0, 0, 2, False), (2, 0, 0, 1, True),
                                                (3, 0, 0, 3, True), (3, 1, 0, 5, False), (4, 4, 0, 2, True), (3, 7, 2, 2, False),
                                                (0, 0, 0, 2, True)])
def test_tiny_and_empty(backends, t, t0, t1, rad, stereo):
    d = pr.random_symmetric(8, 1, 1.0, 5.0)
    want, _ = _check(backends, d, t, t0, t1, rad, 1, 16.0, 100, stereo, min_accept=0)
    assert len(want) == pr.forced_count(t, t0, rad, stereo)


def test_one_row_rectangle(backends):
    d = pr.random_symmetric(150, 8)
    _check(backends, d, 150, 149, 0, 2, 1, 30.0, 10000, False)
    _check(backends, d, 150, 149, 149, 2, 1, 30.0, 10000, True, min_accept=0)   # one cell


# ------------------------------------------------------------------------------------------ device matrices
@pytest.mark.parametrize("N,thresh,mf", [(12, 8.0, 192), (64, 8.0, 1024), (256, 8.0, 4096), (256, 16.0, 4096)])
def test_fused_call_on_synthetic_trajectories(backends, N, thresh, mf):
    torch = _torch()
    from droid_backends import synth
    p = synth.make_ba_problem(N=N, E=2 * N, H=24, W=32, seed=3)
    poses, disps, intr = _dev(p.poses), _dev(p.disps), _dev(p.intrinsics)
    keep = poses.clone(), disps.clone()
    e = torch.zeros(0, dtype=torch.int64, device="cuda")
    ii, jj = backends.proximity_edges(poses, disps, intr, N, 0, 0, 2, 1, BETA, thresh, mf, False, e, e)
    got = np.stack([ii.cpu().numpy(), jj.cpu().numpy()], 1)
    dist = backends.frame_distance_matrix(poses, disps, intr, N, BETA, bidirectional=False)
    st = {}
    want = pr.proximity_edges(dist.cpu().numpy(), N, 0, 0, 2, 1, thresh, mf, False, [], stats=st)
    print(N, thresh, st)
    assert st["accepted"] >= 8
    assert np.array_equal(got, want)
    assert torch.equal(poses, keep[0]) and torch.equal(disps, keep[1])
    # frontend rectangle on the same video, and the matrix handed in
    if N >= 64:
        _check(backends, dist, N, N - 5, max(N - 25, 0), 2, 1, 16.0, 48, False)


# ------------------------------------------------------------------------------------------ suppressing / known lists
def test_select_add_select_again(backends):
    """The real sequence: the first call's edges are in the graph when the second call runs."""
    d = pr.banded(180, 7, closures=30)
    first, st = _check(backends, d, 180, 0, 0, 2, 2, 20.0, 1100, False)
    assert st["stopped"] and st["left"] > 0            # (iii) the stop fired with candidates left
    plain = pr.proximity_edges(d, 180, 0, 0, 2, 2, 20.0, 2200, False, [])
    second, _ = _check(backends, d, 180, 0, 0, 2, 2, 20.0, 2200, False, sup=first, known=first)
    # (ii) listed edges removed candidates the plain call accepts, and nothing new lies inside a listed diamond
    have = set(map(tuple, first.tolist()))
    assert len(set(map(tuple, plain.tolist())) - have - set(map(tuple, second.tolist()))) > 0
    for i, j in second.tolist():
        assert (i, j) not in have
    masked = set()
    for i, j in first.tolist():
        masked.update(pr._diamond(i, j, 2))
    nf = pr.forced_count(180, 0, 2, False)
    unfiltered = pr.proximity_edges(d, 180, 0, 0, 2, 2, 20.0, 2200, False, [tuple(e) for e in first.tolist()])
    assert all(tuple(e) not in masked for e in unfiltered[nf::2].tolist())
    # (iv) the filter removed some edges (the forced ones, known from the first call) but not all
    assert 0 < len(second) < len(unfiltered)
    # filtering against the call's own output leaves nothing
    again = _gpu(backends, _dev(d), 180, 0, 0, 2, 2, 20.0, 1100, False, [], known=first)
    assert again.shape == (0, 2)


def test_suppressing_list_with_duplicates_and_outsiders(backends):
    d = pr.random_symmetric(120, 11)
    rng = np.random.default_rng(0)
    inside = [(int(i), int(j)) for i, j in zip(rng.integers(100, 120, 40), rng.integers(60, 110, 40))]
    sup = inside + inside[:10] + [(-5, 3), (3, -5), (500, 2), (2, 500), (119, 119), (0, 0), (2 ** 40, 7), (99, 80), (80, 99)]
    base = pr.proximity_edges(d, 120, 100, 60, 2, 3, 25.0, 10000, False, [])
    got, _ = _check(backends, d, 120, 100, 60, 2, 3, 25.0, 10000, False, sup=sup)
    assert not np.array_equal(base, got)                # (ii)
    _check(backends, d, 120, 100, 60, 2, 3, 25.0, 10000, True, sup=sup, known=[(101, 70), (70, 101), (119, 118), (7, 7), (-1, 4)])


def test_known_filter_partial(backends):
    d = pr.banded(140, 5)
    full = pr.proximity_edges(d, 140, 0, 0, 2, 1, 18.0, 10000, True, [])
    known = [tuple(e) for e in full[::3].tolist()] + [(1000, 2), (3, 1000)]
    got, _ = _check(backends, d, 140, 0, 0, 2, 1, 18.0, 10000, True, known=known)
    assert 0 < len(got) < len(full)                     # (iv)
    many = [(int(i), int(j)) for i in range(140) for j in range(0, 140, 2)]   # 9800 known edges
    _check(backends, d, 140, 0, 0, 2, 1, 18.0, 10000, True, known=many)


def test_max_factors_boundary(backends):
    d = pr.random_symmetric(96, 21)
    nf = pr.forced_count(96, 0, 2, False)
    full, st = _check(backends, d, 96, 0, 0, 2, 1, 25.0, 100000, False)
    assert not st["stopped"] and st["accepted"] >= 40
    for mf, n in [(nf + 20, nf + 22), (nf + 21, nf + 22), (nf + 19, nf + 20), (nf, nf + 2), (nf - 1, nf), (0, nf)]:
        got, st = _check(backends, d, 96, 0, 0, 2, 1, 25.0, mf, False, min_accept=0)
        assert len(got) == n and st["stopped"] and st["left"] > 0   # (iii); == max_factors continues, > stops
        assert np.array_equal(got, full[:n])


# ------------------------------------------------------------------------------------------ sort fallback, largest size
def test_more_candidates_than_one_lds_sort(backends):
    d = pr.random_symmetric(320, 2)
    _, st = _check(backends, d, 320, 0, 0, 2, 1, 45.0, 100000, False)    # ~ 3/4 of 50k cells: three sorted runs
    assert st["under"] > 2 * 16384 and not st["stopped"]
    _, st = _check(backends, pr.with_ties(260, 9), 260, 0, 0, 1, 3, 10.0, 100000, True)
    assert st["under"] > 16384


def test_largest_rectangle(backends):
    d = pr.random_symmetric(1024, 6)
    _, st = _check(backends, d, 1024, 0, 0, 2, 3, 20.0, 16 * 1024, False)
    assert st["under"] > 8 * 16384 and st["stopped"]
    lib = backends._lib.load()
    assert lib.droid_proximity_workspace_bytes(1025, 0, 0, 0, 8) == 0


# ------------------------------------------------------------------------------------------ streams, inputs untouched
def test_two_streams_with_separate_workspaces(backends):
    torch = _torch()
    lib = backends._lib.load()
    cases = [(pr.banded(256, 3), 256, 0, 0, 2, 3, 22.0, 4096), (pr.random_symmetric(200, 4), 200, 150, 20, 2, 1, 25.0, 10000)]
    alone = [pr.proximity_edges(d, t, t0, t1, rad, nms, th, mf, False, []) for d, t, t0, t1, rad, nms, th, mf in cases]
    streams = [torch.cuda.Stream(), torch.cuda.Stream()]
    bufs = []
    torch.cuda.synchronize()
    for rep in range(3):
        for (d, t, t0, t1, rad, nms, th, mf), s in zip(cases, streams):
            cap = backends.proximity_edge_bound(t, t0, t1, rad, mf, False)
            dist = _dev(d)
            ws = torch.empty(lib.droid_proximity_workspace_bytes(t, t0, t1, 0, cap), dtype=torch.uint8, device="cuda")
            out = torch.empty((cap, 2), dtype=torch.int64, device="cuda")
            cnt = torch.zeros(1, dtype=torch.int32, device="cuda")
            bufs.append((dist, ws, out, cnt))
        torch.cuda.synchronize()
        for k, ((d, t, t0, t1, rad, nms, th, mf), s) in enumerate(zip(cases, streams)):
            dist, ws, out, cnt = bufs[-2 + k]
            rc = lib.droid_proximity_edges(dist.data_ptr(), t, 1, t, t0, t1, rad, nms, th, mf, 0, None, None, 0, None, None, 0,
                                           out.data_ptr(), out.shape[0], cnt.data_ptr(), ws.data_ptr(), ws.numel(),
                                           ctypes.c_void_p(s.cuda_stream))
            assert rc == 0, lib.droid_last_error()
        torch.cuda.synchronize()
        for k in range(2):
            dist, ws, out, cnt = bufs[-2 + k]
            n = int(cnt.item())
            assert n == len(alone[k]) and np.array_equal(out[:n].cpu().numpy(), alone[k])
    st = {}
    pr.proximity_edges(cases[1][0], 200, 150, 20, 2, 1, 25.0, 10000, False, [], stats=st)
    assert st["accepted"] >= 8


def test_inputs_are_left_untouched(backends):
    torch = _torch()
    d = _dev(pr.banded(160, 9))
    first = pr.proximity_edges(d.cpu().numpy(), 160, 0, 0, 2, 2, 20.0, 800, False, [])
    si, sj = _lists(first)
    ki, kj = _lists(first[::2])
    keep = [x.clone() for x in (d, si, sj, ki, kj)]
    backends.proximity_edges(None, None, None, 160, 0, 0, 2, 2, BETA, 20.0, 2000, False, si, sj, ki, kj, dist=d)
    torch.cuda.synchronize()
    for a, b in zip(keep, (d, si, sj, ki, kj)):
        assert torch.equal(a, b)
    # a matrix larger than [t, t] and a view with a row pitch of its own
    big = _dev(pr.random_symmetric(128, 5))
    _check(backends, big, 100, 0, 0, 2, 1, 20.0, 10000, False)
    wide = torch.zeros((100, 160), dtype=torch.float32, device="cuda")
    wide[:, :100] = big[:100, :100]
    got = _gpu(backends, wide[:, :100], 100, 0, 0, 2, 1, 20.0, 10000, False, [])
    assert np.array_equal(got, pr.proximity_edges(big.cpu().numpy(), 100, 0, 0, 2, 1, 20.0, 10000, False, []))
