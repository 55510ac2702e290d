"""The contract of droid_graph_mean (include/droid_backends_hip.h) restated in numpy, bit for bit, with the fp64
evaluation of the same means, the error bound derived from the arithmetic, and the case table the CPU and GPU tests
share.  No tests here.

Arithmetic of a group with the entries e_0 < e_1 < ... and count n, per element:
    acc = float32(x[e_0]); acc = acc + float32(x[e_k]) in ascending k; q = acc / float32(n); out = T(q).

Bound.  With u = 2^-24, the n - 1 sequential fp32 additions are within (n - 1) u sum|x| (1 + O(n u)) of the exact sum
(Higham, Accuracy and Stability of Numerical Algorithms, section 4.2), the division adds u |q|, and |q| <= sum|x| / n
up to the same factor, so |q - mean| <= n u (sum|x| / n) (1 + O(n u)); (n + 2) u (sum|x| / n) leaves 2 u (sum|x| / n)
for the second-order terms.  A half output adds its own rounding, 2^-11 |q| for a normal result and 2^-25 for a
subnormal one; |q| differs from |mean| by at most the first bound, and 2^-11 of that is inside the slack above for
n <= 4094.  fp32 results below 2^-126 are outside the bound (the quotient's absolute error is then 2^-150): no case
here has one -- the subnormal inputs are half subnormals, which are fp32 normals.
"""
import functools

import numpy as np

U = 2.0 ** -24
TILE = {np.float16: 2048, np.float32: 1024}   # elements one reduce workgroup covers: 256 threads x 16 bytes
UNROLL = 4                                    # rows the reduce kernel loads before it adds the first of them
RANGE = 40

# frames with gaps, 0 and RANGE - 1 among them; group sizes 1, 2, 5, 67 and the values around the unroll depth (the first
# entry of a list is loaded apart, so lists of UNROLL and UNROLL + 1 are the ones either side of a full unrolled step)
FRAMES = (0, 3, 4, 9, 17, 30, 31, RANGE - 1)
SIZES = (1, 2, 5, 67, UNROLL - 1, UNROLL, UNROLL + 1, UNROLL + 2)
IGNORED = (-1, RANGE, 2 ** 40)                # no frame of a buffer of RANGE: belong to no group
PLANES = {np.float16: (1, 7, 8, 9, 2047, 2048, 2049, 6144), np.float32: (1, 7, 8, 9, 1023, 1024, 1025, 6144)}
DTYPES = (np.float16, np.float32)


def interleaved_index(seed=0):
    """Every group's entries scattered among the others' and among ignored ones (a fixed shuffle)."""
    idx = [f for f, n in zip(FRAMES, SIZES) for _ in range(n)] + list(IGNORED) * 2
    rng = np.random.default_rng(seed)
    return np.array(idx, np.int64)[rng.permutation(len(idx))]


def lists(index, M, rng, compact):
    """Per row of out the ascending entry list (None: the row is not written), and the distinct in-range count."""
    index = np.asarray(index, np.int64)
    ok = (index >= 0) & (index < rng)
    present = np.unique(index[ok])
    if compact:
        rows = [np.flatnonzero(index == present[g]) if g < len(present) else np.zeros(0, np.int64) for g in range(M)]
    else:
        assert rng == M
        rows = [np.flatnonzero(index == r) for r in range(M)]
    return rows, len(present)


def ref(x, index, M, rng, compact):
    """The restatement: [M, plane] of x.dtype, the bits the kernel must produce."""
    x = np.asarray(x)
    out = np.zeros((M,) + x.shape[1:], x.dtype)
    rows, _ = lists(index, M, rng, compact)
    with np.errstate(all="ignore"):
        for g, es in enumerate(rows):
            if len(es) == 0:
                continue
            acc = x[es[0]].astype(np.float32)
            for e in es[1:]:
                acc = acc + x[e].astype(np.float32)
            out[g] = (acc / np.float32(len(es))).astype(x.dtype)
    return out


def mean64(x, index, M, rng, compact):
    """(mean, sum|x| / n, n) per row in fp64; empty rows are 0 with n = 0."""
    x = np.asarray(x)
    mean = np.zeros((M,) + x.shape[1:], np.float64)
    absmean = np.zeros_like(mean)
    rows, _ = lists(index, M, rng, compact)
    n = np.array([len(es) for es in rows])
    with np.errstate(all="ignore"):
        for g, es in enumerate(rows):
            if len(es):
                x64 = x[es].astype(np.float64)
                mean[g] = x64.sum(0) / len(es)
                absmean[g] = np.abs(x64).sum(0) / len(es)
    return mean, absmean, n


def bound(mean, absmean, n, dtype):
    """The derived bound per element, [M, plane]."""
    b = (n.reshape((-1,) + (1,) * (mean.ndim - 1)) + 2) * U * absmean
    if np.dtype(dtype) == np.float16:
        b = b + 2.0 ** -11 * np.abs(mean) + 2.0 ** -25
    return b


def within_bound(got, x, index, M, rng, compact, factor=1.0):
    """Largest |got - mean64| / bound over the finite elements, and whether every one is within factor x bound."""
    mean, absmean, n = mean64(x, index, M, rng, compact)
    b = bound(mean, absmean, n, x.dtype)
    fin = np.isfinite(mean) & np.isfinite(absmean)
    with np.errstate(all="ignore"):
        err = np.abs(np.asarray(got).astype(np.float64) - mean)
        ratio = np.where(fin & (b > 0), err / b, np.where(fin, err, 0.0))   # b == 0: the mean of zeros must be exact
    worst = float(ratio.max()) if ratio.size else 0.0
    return worst, bool((err[fin] <= factor * b[fin]).all())


def same_bits(a, b):
    """Bit for bit, except that any NaN matches any NaN (the payload is not part of the contract)."""
    a, b = np.asarray(a), np.asarray(b)
    if a.shape != b.shape or a.dtype != b.dtype:
        return False
    iv = {2: np.uint16, 4: np.uint32}[a.dtype.itemsize]
    na, nb = np.isnan(a), np.isnan(b)
    return bool(np.array_equal(na, nb) and np.array_equal(a.view(iv)[~na], b.view(iv)[~nb]))


def _ro(a):
    a.setflags(write=False)
    return a


@functools.lru_cache(maxsize=None)
def shape_problem(dtype, plane):
    """Random rows of the interleaved index at one plane size: (x [E, plane], index [E]).  Read-only, shared."""
    index = interleaved_index()
    rng = np.random.default_rng(plane * 2 + (dtype is np.float32))
    x = rng.normal(0.0, 4.0, (len(index), plane)).astype(dtype)
    return _ro(x), _ro(index)


# the value cases: one problem, frame -> what its group holds (plane VPLANE, every element of a row alike unless noted)
VPLANE = 24
V_FRAMES = dict(max3=1, negzero=2, cancel=5, nan=6, inf=8, subnormal=11, big2=12, long60=20)
V_RANGE = 24


@functools.lru_cache(maxsize=None)
def value_problem(dtype):
    """(x [E, VPLANE], index [E], where): the groups of V_FRAMES interleaved.  `where[name]` = its entries, ascending.
    max3: three entries of 65504 (mean 65504, not inf); negzero: a lone -0.0; cancel: +a, -a, b in this order of e (the sum of the first two
    is exactly 0, so the mean is b / 3); nan / inf: three finite entries, one NaN resp. +inf at element 3 of one of them; subnormal: five
    entries of half subnormals k 2^-24; big2: two entries of 40000 (a half running sum overflows, the mean does not);
    long60: 2048 first, then 59 entries in [0.25, 0.75): a half running sum stays at 2048 (half an ulp there is 1), so
    it loses all 59 of them, about 30 in the sum."""
    rng = np.random.default_rng(11)
    rows, idx = [], []

    def add(name, block):
        for r in np.asarray(block, np.float64).reshape(-1, VPLANE):
            rows.append(r)
            idx.append(V_FRAMES[name])

    add("max3", np.full((3, VPLANE), 65504.0))
    add("negzero", np.full((1, VPLANE), -0.0))
    a, b = rng.uniform(1e3, 1e4, VPLANE), rng.uniform(-1e-3, 1e-3, VPLANE)
    a = a.astype(dtype).astype(np.float64)
    add("cancel", np.stack([a, -a, b]))
    for name, bad in (("nan", np.nan), ("inf", np.inf)):
        blk = rng.normal(0.0, 1.0, (3, VPLANE))
        blk[1, 3] = bad
        add(name, blk)
    add("subnormal", rng.integers(1, 1024, (5, VPLANE)) * 2.0 ** -24 * rng.choice([-1.0, 1.0], (5, VPLANE)))
    add("big2", np.full((2, VPLANE), 40000.0))
    add("long60", rng.uniform(0.25, 0.75, (60, VPLANE)))
    perm = np.random.default_rng(12).permutation(len(idx))
    with np.errstate(all="ignore"):
        x = np.stack(rows)[perm].astype(dtype)
    index = np.array(idx, np.int64)[perm]
    x[np.flatnonzero(index == V_FRAMES["long60"])[0]] = 2048.0
    x[np.flatnonzero(index == V_FRAMES["cancel"])] = np.stack([a, -a, b]).astype(dtype)   # in this order of e
    where = {name: np.flatnonzero(index == f) for name, f in V_FRAMES.items()}
    return _ro(x), _ro(index), where


def compact_row(name):
    """Row of a value group in compact mode: its rank among the frames of V_FRAMES."""
    return sorted(V_FRAMES.values()).index(V_FRAMES[name])


def half_chain(x, index, M):
    """What `zeros(M, ...).index_add_(0, index, x) / bincount` does to a half tensor whose partial sums stay half (the
    sequential model: one rounding per addition, ascending e)."""
    x = np.asarray(x)
    acc = np.zeros((M,) + x.shape[1:], np.float16)
    cnt = np.zeros(M, np.int64)
    with np.errstate(all="ignore"):
        for e, r in enumerate(index):
            if 0 <= r < M:
                acc[r] = (acc[r] + x[e].astype(np.float16)).astype(np.float16)
                cnt[r] += 1
        return (acc / np.maximum(cnt, 1).astype(np.float16).reshape((-1,) + (1,) * (x.ndim - 1))).astype(np.float16)
