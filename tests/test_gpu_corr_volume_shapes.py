"""corr_volume_pyramid on the device at the shapes of tests/corr_volume_cases.py: maps wider than the kernel's 64-column
tile (nxc > 1, a narrow tile after a wide one), partial bands, odd H, the ragged p-tile, both block orders -- and the
value and index edges (half overflow, NaN features, frame indices that only 64-bit compares refuse).

Every build goes into capacity buffers with one guard slot before and one behind the written slots, filled with a byte
sentinel, through both entry points (offset= and slots=).  The criteria are those of test_gpu_corr_volume.py:
level 0 -- EVERY entry within [T(x - beta), T(x + beta)], beta = (C + 2) 2^-24 sum |a||b| (corr_volume_ref);
levels 1-3 -- bit-equal to ref.pool of the device's own previous level; where that pool is NaN (inf + -inf, or a NaN
input) the device must be NaN, payload and sign not compared.  The regimes each case reaches are printed."""
import numpy as np
import pytest
import torch

import corr_volume_cases as cvc
import corr_volume_ref as ref

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
DT = {np.float16: torch.float16, np.float32: torch.float32}
SENTINEL = 0x7B
PATHS = ("offset", "slots")


def _t(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _idx(v):
    return torch.tensor(list(v), dtype=torch.int64, device=DEV)


def _bits(x):
    return np.ascontiguousarray(x).view(np.uint8)


def _build(db, fmaps, ii, jj, levels, path):
    """Build E edges into sentinel-filled capacity buffers of E + 2 slots (slot 0 and slot E + 1 are guards), check the
    guards at every level, return the levels as numpy arrays [E, h, w, h>>l, w>>l] in edge order."""
    h, w = fmaps.shape[-2:]
    E, cap = len(ii), len(ii) + 2
    out = [torch.empty((cap, h, w, h >> l, w >> l), dtype=fmaps.dtype, device=DEV) for l in range(levels)]
    for o in out:
        o.view(torch.uint8).fill_(SENTINEL)
    if path == "offset":
        slots = list(range(1, E + 1))
        got = db.corr_volume_pyramid(fmaps, _idx(ii), _idx(jj), levels, out=out, offset=1)
        assert all(g.data_ptr() == o[1:].data_ptr() and g.shape[0] == E for g, o in zip(got, out))
    else:
        slots = list(range(E, 0, -1))      # the last edge first: a slot order that is not the block order
        db.corr_volume_pyramid(fmaps, _idx(ii), _idx(jj), levels, out=out, slots=_idx(slots))
    torch.cuda.synchronize()
    dev = []
    for l, o in enumerate(out):
        o = o.cpu().numpy()
        for g in (0, cap - 1):
            assert np.all(_bits(o[g]) == SENTINEL), f"{path}: level {l}: guard slot {g} was written"
        dev.append(o[slots])
    return dev


def _check(dev, lo, hi, npdt, label, nan0=None):
    """Level 0 against the interval (NaN exactly where `nan0` says, if given), levels 1.. against the pool rule."""
    E, h, w = dev[0].shape[:3]
    d0 = dev[0].reshape(E, h * w, h * w)
    if nan0 is None:
        inside = (lo <= d0) & (d0 <= hi)             # false for a NaN
    else:
        assert np.array_equal(np.isnan(d0), nan0), f"{label}: level-0 NaNs: {int(np.isnan(d0).sum())} for {int(nan0.sum())}"
        inside = nan0 | ((lo <= d0) & (d0 <= hi))
    outside = int(np.sum(~inside))
    for l in range(len(dev) - 1):
        with np.errstate(invalid="ignore", over="ignore"):
            want = ref.pool(dev[l], npdt)
        nan = np.isnan(want)
        got = dev[l + 1]
        assert got.shape == want.shape
        assert np.all(np.isnan(got[nan])), f"{label}: level {l + 1}: pool(level {l}) is NaN, the device is not"
        diff = int(np.sum(np.where(nan, 0, want).view(_U[npdt]) != np.where(nan, 0, got).view(_U[npdt])))
        assert diff == 0, f"{label}: level {l + 1}: {diff} entries != pool(level {l})"
    return outside


_U = {np.float16: np.uint16, np.float32: np.uint32}


# ------------------------------------------------------------------------------------------------------ the table
@pytest.mark.parametrize("case", cvc.CASES, ids=[c.name for c in cvc.CASES])
def test_table_case(backends, case):
    npdt, r = case.dtype, cvc.regime_of(case)
    fm = cvc.make_fmaps(case)
    a, b = ref.operands(fm, case.ii, case.jj, npdt)
    lo, hi, mid = ref.level0_interval(a, b, npdt)
    assert np.all(np.isfinite(lo)) and np.all(np.isfinite(hi))
    fmaps = _t(fm)
    built = {}
    for path in PATHS:
        dev = _build(backends, fmaps, case.ii, case.jj, case.levels, path)
        assert len(dev) == case.levels and dev[0].dtype == npdt
        d0 = dev[0].reshape(lo.shape)
        outside = _check(dev, lo, hi, npdt, f"{case.name} {path}")
        print(f"CASE {case.name} {path:6s} | {cvc.describe(r)} | share != T(x) {np.mean(d0 != mid):.2e} | outside the interval {outside}")
        assert outside == 0
        assert all(np.any(d0[e] != 0) for e in range(len(case.ii)))
        built[path] = dev
    for x, y in zip(built["offset"], built["slots"]):      # the slot entry point gives the bits of the offset one
        assert np.array_equal(_bits(x), _bits(y))
    # a stereo edge read camera 1: against camera 0 it would be the Gram matrix of one map (symmetric)
    for e, (i, j) in enumerate(zip(case.ii, case.jj)):
        if case.ncam == 2 and i == j:
            g = built["offset"][0][e].reshape(case.H * case.W, case.H * case.W)
            assert not np.array_equal(g, g.T)


# --------------------------------------------------------------------------------------------- batch independence
@pytest.mark.parametrize("npdt", [np.float16, np.float32])
@pytest.mark.parametrize("H,W", [(12, 80), (8, 136), (10, 72)])
def test_an_edges_bits_do_not_depend_on_the_block_order(backends, npdt, H, W):
    """The same edge alone (E = 1) and inside a batch whose E flips the reordering condition: identical bits."""
    alone = cvc.classify(npdt, 1, H, W, 32, 4)
    Eb = next(E for E in range(2, 9) if cvc.classify(npdt, E, H, W, 32, 4).reorder != alone.reorder)
    batch = cvc.classify(npdt, Eb, H, W, 32, 4)
    print(f"{H}x{W} {npdt.__name__}: E=1 {cvc.describe(alone)} || E={Eb} {cvc.describe(batch)}")
    assert alone.nxc > 1 and alone.reorder != batch.reorder
    rng = np.random.default_rng(H * W)
    fmaps = _t(rng.normal(0, 1, (4, 1, 32, H, W)).astype(npdt))
    ii = [k % 4 for k in range(Eb)]
    jj = [(k + 1 + k // 4) % 4 for k in range(Eb)]
    whole = [p.cpu().numpy() for p in backends.corr_volume_pyramid(fmaps, _idx(ii), _idx(jj), 4)]
    assert all(np.any(whole[0][e] != 0) for e in range(Eb))
    for e in range(Eb):
        single = backends.corr_volume_pyramid(fmaps, _idx(ii[e:e + 1]), _idx(jj[e:e + 1]), 4)
        for l in range(4):
            assert np.array_equal(_bits(single[l].cpu().numpy()[0]), _bits(whole[l][e])), f"edge {e} level {l}"


# -------------------------------------------------------------------------------------------------- special values
def test_half_overflow_rounds_to_the_signed_infinities(backends):
    """Level 0 is T(fp32 sum): sums beyond half's range come out as +-inf, and the interval test stays decisive there
    because rounding to T is monotone (lo == hi == +-inf forces the device's value).  The pools of inf and -inf are NaN."""
    H, W, C = cvc.OVERFLOW_SHAPE
    fm = cvc.overflow_fmaps()
    a, b = ref.operands(fm, [0], [1], np.float16)
    lo, hi, _ = ref.level0_interval(a, b, np.float16)
    r = cvc.classify(np.float16, 1, H, W, C, 4)
    assert r.nxc > 1
    fmaps = _t(fm)
    for path in PATHS:
        dev = _build(backends, fmaps, [0], [1], 4, path)
        outside = _check(dev, lo, hi, np.float16, f"overflow {path}")
        d0 = dev[0]
        print(f"CASE overflow-{H}x{W}-f16-C{C}-L4-cam1-E1 {path:6s} | {cvc.describe(r)} | level 0: +inf {int(np.isposinf(d0).sum())} "
              f"-inf {int(np.isneginf(d0).sum())} finite {int(np.isfinite(d0).sum())} NaN {int(np.isnan(d0).sum())}; "
              f"NaN in levels 1-3: {[int(np.isnan(d).sum()) for d in dev[1:]]} | outside the interval {outside}")
        assert outside == 0
        assert np.isposinf(d0).sum() >= 100 and np.isneginf(d0).sum() >= 100 and np.isfinite(d0).sum() >= 100
        assert np.isnan(dev[1]).sum() >= 100


@pytest.mark.parametrize("npdt", [np.float16, np.float32])
def test_a_nan_feature_poisons_one_row_and_one_column(backends, npdt):
    """One NaN in fmaps[ii] at pixel p* (last p-tile), one in fmaps[jj] at pixel q* (last band, last x-tile): level 0 is
    NaN exactly on row p* and column q* of that edge -- no staging or transposed-read row leaks into its neighbours, no
    dead lane's 0 * NaN is stored -- and within the interval everywhere else; the second edge of the call is clean."""
    H, W, C = cvc.NAN_SHAPE
    fm, pstar, qstar = cvc.nan_fmaps(npdt)
    ii, jj = [0, 2], [1, 3]
    a, b = ref.operands(fm, ii, jj, npdt)
    lo, hi, _ = ref.level0_interval(a, b, npdt)
    nan0 = np.zeros(lo.shape, bool)
    nan0[0, pstar, :] = True
    nan0[0, :, qstar] = True
    assert np.array_equal(np.isnan(lo), nan0) and np.array_equal(np.isnan(hi), nan0)
    r = cvc.classify(npdt, 2, H, W, C, 4)
    fmaps = _t(fm)
    for path in PATHS:
        dev = _build(backends, fmaps, ii, jj, 4, path)
        outside = _check(dev, lo, hi, npdt, f"nan {npdt.__name__} {path}", nan0=nan0)
        print(f"CASE nan-{H}x{W}-{'f16' if npdt is np.float16 else 'f32'}-C{C}-L4-cam1-E2 {path:6s} | {cvc.describe(r)} | "
              f"level-0 NaN {int(np.isnan(dev[0]).sum())} (row {pstar}, column {qstar}); NaN in levels 1-3: "
              f"{[int(np.isnan(d).sum()) for d in dev[1:]]} | outside the interval {outside}")
        assert outside == 0
        assert not any(np.isnan(d[1]).any() for d in dev)
        # level 1: the whole plane of p*, and the one cell that pools q* in every other plane
        n1 = np.zeros(dev[1][0].shape, bool).reshape(H * W, H >> 1, W >> 1)
        n1[pstar] = True
        n1[:, (qstar // W) >> 1, (qstar % W) >> 1] = True
        assert np.array_equal(np.isnan(dev[1][0]).reshape(n1.shape), n1)


@pytest.mark.parametrize("npdt", [np.float16, np.float32])
def test_frame_indices_outside_the_buffer_give_zeros(backends, npdt):
    """ii / jj in {-1, nbuf, 2^32, 2^32 + 1, 2^63 - 1}: an all-zero slot at every level, written into a poisoned buffer
    (2^32 and 2^32 + 1 are valid frames once cut to 32 bits); the valid edge of the same call keeps its bits."""
    H, W, C, nbuf = 10, 72, 32, 3
    rng = np.random.default_rng(11)
    fmaps = _t(rng.normal(0, 1, (nbuf, 1, C, H, W)).astype(npdt))
    bad = cvc.bad_indices(nbuf)
    ii = bad + [0] + [0] * len(bad)
    jj = [1] * len(bad) + [1] + bad
    good = len(bad)
    print(f"indices {npdt.__name__}: {cvc.describe(cvc.classify(npdt, len(ii), H, W, C, 4))}")
    want = [p.cpu().numpy()[0] for p in backends.corr_volume_pyramid(fmaps, _idx([0]), _idx([1]), 4)]
    assert np.any(want[0] != 0)
    for path in PATHS:
        dev = _build(backends, fmaps, ii, jj, 4, path)
        for l in range(4):
            for e in range(len(ii)):
                if e == good:
                    assert np.array_equal(_bits(dev[l][e]), _bits(want[l])), f"{path}: level {l}: the valid edge changed"
                else:
                    assert not _bits(dev[l][e]).any(), f"{path}: level {l}: edge {e} (ii {ii[e]}, jj {jj[e]}) is not all zero bits"
