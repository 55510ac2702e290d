"""CPU checks of the proximity-edge selection: the host restatement (tests/proximity_ref.py) against hand-worked
cases, its literal (flat-indexed, as the reference) and frame-indexed versions against each other, and the host side
of the C ABI and of the Python mirror.  No GPU needed."""
import ctypes

import numpy as np
import pytest

import proximity_ref as pr

INF = np.inf


def _six():
    """6 frames, symmetric; only the cells named below are at or under a threshold of 10."""
    d = np.full((6, 6), 50.0, np.float32)
    for (i, j), v in {(3, 0): 4.0, (4, 0): 2.0, (5, 0): 3.0, (4, 1): 6.0, (5, 2): 5.0, (5, 1): 7.0}.items():
        d[i, j] = d[j, i] = v
    return d


def _sel(d, **kw):
    a = dict(t=6, t0=0, t1=0, rad=1, nms=0, thresh=10.0, max_factors=1000, stereo=False, sup=[])
    a.update(kw)
    t, t0, t1 = a.pop("t"), a.pop("t0"), a.pop("t1")
    return pr.select(pr.rect_distance(d, t, t0, t1), t, t0, t1, **a)


FORCED_6_RAD1 = [(1, 0), (0, 1), (2, 0), (0, 2), (2, 1), (1, 2), (3, 1), (1, 3), (3, 2), (2, 3),
                 (4, 2), (2, 4), (4, 3), (3, 4), (5, 3), (3, 5), (5, 4), (4, 5)]


def _pairs(cells):
    return [e for (i, j) in cells for e in ((i, j), (j, i))]


def test_six_frames_by_eye():
    # rad = 1: i - 1 < j masked, so candidates need i - j >= 2; (3,1), (4,2), (5,3) are forced cells.  nms = 0: an
    # accepted cell masks only itself.  Ascending d: (4,0) 2, (5,0) 3, (3,0) 4, (5,2) 5, (4,1) 6, (5,1) 7.
    es = _sel(_six())
    assert es == FORCED_6_RAD1 + _pairs([(4, 0), (5, 0), (3, 0), (5, 2), (4, 1), (5, 1)])
    # nms = 1: accepting (4,0) (|i-j| - 2 = 2 -> radius 1) masks (5,0), (3,0), (4,1); (5,2) has radius 1 and masks (5,1)
    es = _sel(_six(), nms=1)
    assert es == FORCED_6_RAD1 + _pairs([(4, 0), (5, 2)])
    # the threshold is inclusive (`d > thresh` skips)
    assert _sel(_six(), thresh=4.0) == FORCED_6_RAD1 + _pairs([(4, 0), (5, 0), (3, 0)])
    assert pr.forced_count(6, 0, 1, False) == len(FORCED_6_RAD1)


def test_default_max_factors_gives_forced_edges_only():
    assert _sel(_six(), max_factors=-1) == FORCED_6_RAD1
    assert _sel(_six(), max_factors=-1, t0=4, t1=1) == [(4, 2), (2, 4), (4, 3), (3, 4), (5, 3), (3, 5), (5, 4), (4, 5)]


def test_suppressing_edge_removes_its_diamond():
    # (4,0) in the list: radius min(4 - 2, nms = 1) = 1 -> (4,0), (3,0), (5,0), (4,1) are gone before the walk
    es = _sel(_six(), sup=[(4, 0)], nms=1)
    assert es == FORCED_6_RAD1 + _pairs([(5, 2)])
    # a neighbouring edge |i - j| = 2 has radius 0: only its own cell
    es = _sel(_six(), sup=[(5, 3), (2, 0), (40, -3)], nms=1)
    assert es == FORCED_6_RAD1 + _pairs([(4, 0), (5, 2)])
    # nms = 0: a listed edge still masks its own cell
    assert _sel(_six(), sup=[(5, 0), (5, 0)]) == FORCED_6_RAD1 + _pairs([(4, 0), (3, 0), (5, 2), (4, 1), (5, 1)])


def test_stereo_rows_start_with_the_self_edge():
    es = _sel(_six(), stereo=True, max_factors=-1)
    want = []
    for i in range(6):
        want.append((i, i))
        for j in range(max(i - 2, 0), i):
            want += [(i, j), (j, i)]
    assert es == want
    assert pr.forced_count(6, 0, 1, True) == len(want)


def test_stop_fires_mid_list():
    n = len(FORCED_6_RAD1)   # 18
    st = {}
    # len == max_factors continues, len > max_factors stops: 18 -> 20 -> 22 > 21
    es = pr.select(pr.rect_distance(_six(), 6, 0, 0), 6, 0, 0, 1, 0, 10.0, n + 3, False, [], st)
    assert es == FORCED_6_RAD1 + _pairs([(4, 0), (5, 0)])
    assert st["stopped"] and st["left"] == 4 and st["accepted"] == 2
    assert _sel(_six(), max_factors=n + 2) == FORCED_6_RAD1 + _pairs([(4, 0), (5, 0)])      # 20 <= 20: one more? no: 18, 20 ok, 22 stop
    assert _sel(_six(), max_factors=n + 4) == FORCED_6_RAD1 + _pairs([(4, 0), (5, 0), (3, 0)])
    assert _sel(_six(), max_factors=n) == FORCED_6_RAD1 + _pairs([(4, 0)])
    assert _sel(_six(), max_factors=n - 1) == FORCED_6_RAD1


def test_ties_go_by_flat_index_and_nan_is_inf():
    d = np.full((6, 6), 50.0, np.float32)
    for (i, j) in [(5, 1), (3, 0), (4, 2), (5, 0), (4, 0)]:
        d[i, j] = d[j, i] = 5.0
    d[4, 1] = d[1, 4] = np.nan
    es = _sel(d, rad=0, max_factors=1000)
    forced = [e for i in range(1, 6) for e in ((i, i - 1), (i - 1, i))]
    assert es == forced + _pairs([(3, 0), (4, 0), (4, 2), (5, 0), (5, 1)])


def test_known_filter_keeps_order():
    es = _sel(_six())
    out = pr.filter_known(es, [(0, 4), (2, 1), (9, 9)])
    assert out == [e for e in es if e not in ((0, 4), (2, 1))] and len(out) == len(es) - 2


def test_literal_flat_indexing_agrees_wherever_the_reference_is_called():
    """The contract ignores cells outside the rectangle; the reference wraps them by flat index.  For t1 < t0 and for
    t1 = t0 = 0 the two must give the same list, except where the literal version raises IndexError -- which needs
    t0 - t1 <= rad (a forced column left of the rectangle by more than the array holds)."""
    rng = np.random.default_rng(5)
    cases = raised = 0
    for t in list(range(1, 20)) + [23, 31, 40, 47]:
        for seed in range(3):
            full = pr.banded(t, 100 * t + seed, closures=4, patch=1) if seed else pr.random_symmetric(t, t, 1.0, 40.0)
            shapes = [(0, 0)] + [(int(a), int(b)) for a, b in
                                 [sorted(rng.integers(0, t, 2), reverse=True) for _ in range(14)] if b < a]
            for (t0, t1) in shapes:
                for rad in (1, 2, 3):
                    nms = int(rng.integers(0, 4))
                    stereo = bool(rng.integers(0, 2))
                    thresh = float(rng.choice([8.0, 16.0, 30.0]))
                    mf = int(rng.choice([-1, 10, 40, 10000]))
                    sup = [(int(rng.integers(0, t)), int(rng.integers(0, t))) for _ in range(int(rng.integers(0, 6)))]
                    d = pr.rect_distance(full, t, t0, t1)
                    want = pr.select(d, t, t0, t1, rad, nms, thresh, mf, stereo, sup)
                    cases += 1
                    try:
                        got = pr.select_literal(d, t, t0, t1, rad, nms, thresh, mf, stereo, sup)
                    except IndexError:
                        raised += 1
                        assert t0 - t1 <= rad, (t, t0, t1, rad)
                        continue
                    assert got == want, (t, t0, t1, rad, nms, stereo, thresh, mf, sup)
    assert cases > 2000 and raised < cases // 20


# ------------------------------------------------------------------------------------------ C ABI, host side only
def _call(lib, *, dist=None, ld=64, t=8, t0=0, t1=0, rad=2, nms=1, thresh=16.0, mf=48, stereo=0, n_sup=0, n_known=0,
          out=None, cap=1 << 20, count=None, ws=None, ws_bytes=0):
    return lib.droid_proximity_edges(dist, ld, 1, t, t0, t1, rad, nms, thresh, mf, stereo, None, None, n_sup, None, None,
                                     n_known, out, cap, count, ws, ws_bytes, None)


def test_abi_exports_and_lists_the_proximity_symbols(backends):
    lib = ctypes.CDLL(backends._lib.LIB_PATH)
    for s in ("droid_proximity_workspace_bytes", "droid_proximity_edges"):
        assert hasattr(lib, s) and s in backends._lib.SYMBOLS
    assert "proximity_edges" in backends.__all__ and callable(backends.proximity_edges)


def test_host_side_argument_checks(backends):
    lib = backends._lib.load()
    fake = ctypes.c_void_p(4096)   # never dereferenced: every call below fails on the host
    ok = dict(dist=fake, out=fake, count=fake, ws=fake, ws_bytes=1 << 30)
    for bad in (dict(t0=2, t1=3), dict(rad=-1), dict(nms=-1), dict(cap=3), dict(dist=None), dict(out=None),
                dict(count=None), dict(ws=None), dict(t=2000), dict(t=-1), dict(ld=4), dict(n_sup=2), dict(n_known=2)):
        rc = _call(lib, **{**ok, **bad})
        assert rc == -1 and b"proximity" in lib.droid_last_error(), (bad, rc, lib.droid_last_error())
    rc = _call(lib, **{**ok, "ws_bytes": 16})
    assert rc == -2 and b"proximity" in lib.droid_last_error() and b"workspace" in lib.droid_last_error()
    # cap: exactly the bound passes the cap check (and fails on the next one), one below does not
    bound = backends.proximity_edge_bound(8, 0, 0, 2, 48, False)
    assert bound == 50 and pr.forced_count(8, 0, 2, False) == 36
    assert _call(lib, **{**ok, "cap": bound - 1}) == -1 and b"cap" in lib.droid_last_error()
    assert _call(lib, **{**ok, "cap": bound, "count": None}) == -1 and b"count_out" in lib.droid_last_error()
    assert backends.proximity_edge_bound(8, 0, 0, 2, -1, True) == pr.forced_count(8, 0, 2, True) == 44
    assert backends.proximity_edge_bound(8, 5, 1, 2, 10 ** 9, False) == pr.forced_count(8, 5, 2, False) + 2 * 3 * 7
    for t, t0, rad, s in [(30, 0, 3, True), (30, 11, 1, False), (5, 4, 9, True), (9, 9, 2, True), (3, 7, 2, False)]:
        assert backends.proximity_edge_bound(t, t0, 0, rad, -1, s) == pr.forced_count(t, t0, rad, s)


def test_workspace_query_grows_with_the_rectangle(backends):
    lib = backends._lib.load()
    q = lib.droid_proximity_workspace_bytes
    assert 0 < q(64, 0, 0, 0, 100) < q(256, 0, 0, 0, 100) < q(512, 0, 0, 0, 100) < q(1024, 0, 0, 0, 100)
    assert q(256, 251, 231, 0, 100) < q(256, 0, 0, 0, 100)
    assert q(256, 0, 0, 500, 100) > q(256, 0, 0, 0, 100)
    assert q(1025, 0, 0, 0, 100) == 0 and q(8, 2, 3, 0, 100) == 0    # what droid_proximity_edges rejects
    assert q(4000, 3995, 3975, 0, 100) > 0                           # a frontend rectangle late in a long run


def test_python_mirror_refuses_cpu_tensors(backends):
    import torch
    e = torch.zeros(0, dtype=torch.int64)
    with pytest.raises(RuntimeError, match="no CPU path"):
        backends.proximity_edges(None, None, None, 8, 0, 0, 2, 1, 0.25, 16.0, 48, False, e, e, dist=torch.zeros(8, 8))
    with pytest.raises(RuntimeError, match="no CPU path"):
        backends.proximity_edges(torch.zeros(8, 7), torch.zeros(8, 4, 4), torch.zeros(4), 8, 0, 0, 2, 1, 0.25, 16.0, 48,
                                 False, e, e)
