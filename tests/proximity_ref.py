"""Host restatement of the edge selection in `FactorGraph.add_proximity_factors` and of
`__filter_repeated_edges` (reference droid_slam/factor_graph.py:315-379, :44-55), written from the contract in
include/droid_backends_hip.h.  Test code only: the product never imports it.

Two versions of the selection:
  select_literal  addresses d by FLAT index exactly as the reference does, Python's negative-index wrap and
                  IndexError included, so that what the contract says about those quirks is checked, not assumed;
  select          addresses d by frame and ignores cells outside the rectangle -- the contract the device meets.
Both break ties of the sort by ascending flat index (np.argsort(kind="stable")) and treat NaN as inf.
"""
import numpy as np


def rect_distance(dist, t, t0, t1, bidirectional=True):
    """Step 1: the rectangle rows [t0,t) x columns [t1,t) of the DIRECTED fp32 matrix `dist`, flat, as
    .5 * (d + d.T) in fp32 (one rounding: the sum; the halving is exact)."""
    dist = np.asarray(dist, np.float32)
    R, C = max(t - t0, 0), max(t - t1, 0)
    if R == 0 or C == 0:
        return np.zeros((0,), np.float32)
    a = dist[t0:t, t1:t]
    if bidirectional:
        a = np.float32(0.5) * (a + dist[t1:t, t0:t].T)
    return np.ascontiguousarray(a, np.float32).reshape(-1)


def forced_count(t, t0, rad, stereo):
    return sum((1 if stereo else 0) + 2 * (i - max(i - rad - 1, 0)) for i in range(t0, t))


def _mask(d, t, t0, t1, rad):
    C = t - t1
    ii, jj = np.meshgrid(np.arange(t0, t), np.arange(t1, t), indexing="ij")
    ii, jj = ii.reshape(-1), jj.reshape(-1)
    d = np.array(d, np.float32, copy=True)
    d[np.isnan(d)] = np.inf
    d[ii - rad < jj] = np.inf
    d[d > 100] = np.inf
    return d, ii, jj, C


def _diamond(i, j, nms):
    r = max(min(abs(i - j) - 2, nms), 0)
    for di in range(-nms, nms + 1):
        for dj in range(-nms, nms + 1):
            if abs(di) + abs(dj) <= r:
                yield i + di, j + dj


def select_literal(d, t, t0, t1, rad, nms, thresh, max_factors, stereo, sup, stats=None):
    """The reference's loop, flat indexing kept literally.  d: flat fp32 rectangle (rect_distance); sup: iterable
    of (i, j).  Returns the list of (i, j).  May raise IndexError where the reference would."""
    t, t0, t1 = int(t), int(t0), int(t1)
    if t <= t0:
        return []
    d, ii, jj, C = _mask(d, t, t0, t1, rad)
    for i, j in sup:
        for i1, j1 in _diamond(int(i), int(j), nms):
            if t0 <= i1 < t and t1 <= j1 < t:
                d[(i1 - t0) * C + (j1 - t1)] = np.inf
    es = []
    for i in range(t0, t):
        if stereo:
            es.append((i, i))
            d[(i - t0) * C + (i - t1)] = np.inf
        for j in range(max(i - rad - 1, 0), i):
            es.append((i, j))
            es.append((j, i))
            d[(i - t0) * C + (j - t1)] = np.inf      # j < t1: a negative column, lands in another row (or raises)
    return _walk(d, ii, jj, C, t, t0, t1, nms, thresh, max_factors, es, stats)


def select(d, t, t0, t1, rad, nms, thresh, max_factors, stereo, sup, stats=None):
    """The contract: frame-indexed, cells outside the rectangle ignored."""
    t, t0, t1 = int(t), int(t0), int(t1)
    if t <= t0:
        return []
    assert t1 <= t0
    d, ii, jj, C = _mask(d, t, t0, t1, rad)
    d2 = d.reshape(t - t0, C)
    for i, j in sup:
        for i1, j1 in _diamond(int(i), int(j), nms):
            if t0 <= i1 < t and t1 <= j1 < t:
                d2[i1 - t0, j1 - t1] = np.inf
    es = []
    for i in range(t0, t):
        if stereo:
            es.append((i, i))
            d2[i - t0, i - t1] = np.inf
        for j in range(max(i - rad - 1, 0), i):
            es.append((i, j))
            es.append((j, i))
            if j >= t1:
                d2[i - t0, j - t1] = np.inf
    return _walk(d, ii, jj, C, t, t0, t1, nms, thresh, max_factors, es, stats)


def _walk(d, ii, jj, C, t, t0, t1, nms, thresh, max_factors, es, stats):
    """Step 5.  stats (a dict, optional) receives: forced, accepted (pairs), under (cells at or under the threshold
    when the walk starts), suppressed (of those, visited before the stop and found at inf because an EARLIER ACCEPT
    of this walk masked them), stopped (the max_factors stop fired), left (cells still at or under the threshold
    that the stop left unvisited)."""
    thresh = np.float32(thresh)
    order = np.argsort(d, kind="stable")
    start = d <= thresh
    forced, accepted, suppressed, stopped, left = len(es), 0, 0, False, 0
    for n, k in enumerate(order):
        if d[k] > thresh:
            suppressed += int(start[k])
            continue
        if len(es) > max_factors:
            stopped = True
            left = int(np.count_nonzero(d[order[n:]] <= thresh))
            break
        i, j = int(ii[k]), int(jj[k])
        es.append((i, j))
        es.append((j, i))
        accepted += 1
        for i1, j1 in _diamond(i, j, nms):
            if t0 <= i1 < t and t1 <= j1 < t:
                d[(i1 - t0) * C + (j1 - t1)] = np.inf
    if stats is not None:
        stats.update(forced=forced, accepted=accepted, under=int(np.count_nonzero(start)), suppressed=suppressed,
                     stopped=stopped, left=left)
    return es


def filter_known(es, known):
    """Step 6 (`__filter_repeated_edges`): drop the edges that are in `known`, keep the order."""
    eset = set((int(i), int(j)) for i, j in known)
    return [e for e in es if e not in eset]


def proximity_edges(dist, t, t0, t1, rad, nms, thresh, max_factors, stereo, sup, known=None, bidirectional=True,
                    stats=None):
    """What droid_proximity_edges returns for the directed matrix `dist`: an [n, 2] int64 array."""
    es = select(rect_distance(dist, t, t0, t1, bidirectional), t, t0, t1, rad, nms, thresh, max_factors, stereo, sup,
                stats)
    if known is not None and len(known):
        es = filter_known(es, known)
    return np.asarray(es, np.int64).reshape(-1, 2)


# ---------------------------------------------------------------------------------------------- synthetic inputs
def random_symmetric(n, seed, lo=1.0, hi=60.0):
    """Symmetric fp32 matrix whose entries below the diagonal are all different."""
    rng = np.random.default_rng(seed)
    vals = rng.permutation(n * n).astype(np.float64) / (n * n) * (hi - lo) + lo
    a = np.tril(vals.reshape(n, n), -1)
    a = (a + a.T).astype(np.float32)
    low = a[np.tril_indices(n, -1)]
    assert len(np.unique(low)) == len(low)
    return a


def banded(n, seed, slope=3.0, noise=2.0, closures=20, patch=3):
    """A trajectory: distance grows with |i - j| (plus noise), with `closures` patches of small distance far from
    the diagonal (loop closures).  Symmetric fp32."""
    rng = np.random.default_rng(seed)
    i, j = np.meshgrid(np.arange(n), np.arange(n), indexing="ij")
    a = slope * np.abs(i - j) + rng.uniform(0, noise, (n, n))
    for _ in range(closures):
        ci = int(rng.integers(n // 3, n)) if n >= 12 else int(rng.integers(0, n))
        cj = int(rng.integers(0, max(ci - n // 4, 1)))
        for di in range(-patch, patch + 1):
            for dj in range(-patch, patch + 1):
                if 0 <= ci + di < n and 0 <= cj + dj < n:
                    a[ci + di, cj + dj] = rng.uniform(0.5, 8.0)
    a = np.tril(a, -1)
    return (a + a.T).astype(np.float32)


def with_ties(n, seed, levels=7):
    """Symmetric fp32 matrix with only `levels` distinct values: the order is decided by the tie rule."""
    rng = np.random.default_rng(seed)
    a = np.tril(rng.integers(1, levels + 1, (n, n)).astype(np.float64) * 2.5, -1)
    return (a + a.T).astype(np.float32)
