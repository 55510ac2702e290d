"""Host-side half of the correlation-pyramid shape tests (tests/corr_volume_cases.py): the classifier's constants are
the kernel's, the case table reaches every regime the classifier names and holds nothing the entry point refuses, the
kernel's write maps cover every element of a slot exactly once, and corr_volume_ref is pinned in the value regimes the
GPU tests add (half overflow, inf/NaN pooling, NaN features).  Needs no GPU."""
import os
import re

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import corr_volume_cases as cvc
import corr_volume_ref as ref

CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "droid-slam_reserch_amd", "csrc")
TYPES = [np.float16, np.float32]


def _src(name):
    with open(os.path.join(CSRC, name)) as f:
        return f.read()


def _one(pattern, text):
    m = re.findall(pattern, text)
    assert len(m) == 1, (pattern, m)
    return m[0]


# ------------------------------------------------------------------------------------------------------ constants
def test_classifier_constants_are_the_kernels():
    k = _src("corr_volume.hip")
    p, kc = _one(r"CvCfg<_Float16>\s*\{\s*static constexpr int P = (\d+), KC = (\d+);", k)
    assert (int(p), int(kc)) == (cvc.P[np.float16], cvc.KC[np.float16])
    p, kc = _one(r"CvCfg<float>\s*\{\s*static constexpr int P = (\d+), KC = (\d+);", k)
    assert (int(p), int(kc)) == (cvc.P[np.float32], cvc.KC[np.float32])
    # host code: p-tiles, bands, x-tiles
    assert re.search(r"a\.nptiles = \(int\)\(\(hw \+ P - 1\) / P\);", k)
    assert int(_one(r"a\.nbands = \(H \+ 7\) / (\d+);", k)) == cvc.BAND
    w1, w = _one(r"a\.nxc = \(W \+ (\d+)\) / (\d+);", k)
    assert int(w) == cvc.TILE_W and int(w1) == cvc.TILE_W - 1
    # the tile walk (twice: the prefetch and the loop) and the row of a thread
    walks = re.findall(r"const int band = t / a\.nxc, x0 = \(t % a\.nxc\) \* (\d+);", k)
    assert walks == [str(cvc.TILE_W)] * 2
    assert re.findall(r"wc = min\((\d+), W - x0\)", k) == [str(cvc.TILE_W)] * 2
    assert re.findall(r"y = (\d+) \* band \+ s_r", k) == [str(cvc.BAND)] * 2
    # the reordering condition, and the block size the write maps assume
    assert _one(r"if \(\(total & (\d+)u\) == 0\) v = ", k) == str(cvc.XCD - 1)
    assert int(_one(r"__launch_bounds__\((\d+),", k)) == cvc.THREADS
    assert re.search(r"dim3\(\(unsigned\)grid\), dim3\(256\)", k) and re.search(r"const long long grid = \(long long\)E \* a\.nptiles;", k)


def test_legal_restates_the_entry_points_shape_rules():
    a = _src("api.hip")
    body = a[a.index("static int corr_volume_pyramid_any"):a.index("int droid_corr_volume_pyramid(")]
    step, cmax = _one(r"if \(C <= 0 \|\| C % (\d+) != 0 \|\| C > (\d+)\)", body)
    assert (int(step), int(cmax)) == (cvc.C_STEP, cvc.C_MAX)
    h, w, ws, hws, sh = _one(r"if \(H < (\d+) \|\| W < (\d+) \|\| W % (\d+) != 0 \|\| \(\(long long\)H \* W\) % (\d+) != 0 \|\| "
                             r"\(long long\)H \* W > \(1 << (\d+)\)\)", body)
    assert int(h) == int(w) == cvc.MIN_SIDE and int(ws) == cvc.W_STEP and int(hws) == cvc.HW_STEP and 1 << int(sh) == cvc.HW_MAX
    assert _one(r"if \(levels < 1 \|\| levels > (\d+)\)", body) == str(cvc.MAX_LEVELS)
    assert re.search(r"ncam < 1 \|\| ncam > 2", body)
    # the kernel's chunks divide every legal C, and a p-tile of fp32 is never ragged
    assert cvc.C_STEP % cvc.KC[np.float16] == 0 and cvc.C_STEP % cvc.KC[np.float32] == 0
    assert cvc.HW_STEP % cvc.P[np.float32] == 0 and cvc.HW_STEP % cvc.P[np.float16] != 0
    assert cvc.legal(1, 8, 8, 32, 1) and cvc.legal(3, 60, 80, 128, 4, 2)
    for bad in [dict(H=7), dict(W=12), dict(H=9, W=8), dict(C=48), dict(C=288), dict(levels=5), dict(levels=0), dict(ncam=3)]:
        kw = dict(E=1, H=16, W=24, C=128, levels=4, ncam=1)
        kw.update(bad)
        assert not cvc.legal(**kw), bad


# -------------------------------------------------------------------------------------------------------- coverage
def test_no_case_is_one_the_entry_point_refuses():
    names = [c.name for c in cvc.CASES]
    assert len(set(names)) == len(names) and len(names) <= 48
    for c in cvc.CASES:
        assert cvc.legal(len(c.ii), c.H, c.W, c.C, c.levels, c.ncam), c.name
        assert len(c.ii) == len(c.jj) >= 1 and all(0 <= i < c.nbuf for i in c.ii + c.jj), c.name
        assert (c.H, c.W) in cvc.SHAPES
    assert {(c.H, c.W) for c in cvc.CASES} == set(cvc.SHAPES)


@pytest.mark.parametrize("dt", TYPES)
def test_the_table_reaches_every_regime(dt):
    cases = [c for c in cvc.CASES if c.dtype is dt]
    regs = [cvc.regime_of(c) for c in cases]
    wide = [(c, r) for c, r in zip(cases, regs) if r.nxc > 1]
    assert {r.P for r in regs} == {cvc.P[dt]}
    assert {r.nptiles == 1 for r in regs} == {False}                 # H, W >= 8: always more than one workgroup per edge
    # a ragged p-tile exists for half only (H * W % 16 == 0 is the rule and P = 16 for fp32)
    assert {r.ragged_ptile for r in regs} == ({False, True} if dt is np.float16 else {False})
    if dt is np.float16:
        assert any(r.ragged_ptile and r.nxc > 1 for r in regs)
    assert {r.nbands for r in regs} >= {1, 2}
    assert {r.last_band_rows for r in regs} >= {1, 2, 3, 4, 8}      # partial bands of every small height, and a full one
    assert {r.odd_h for r in regs} == {False, True} and any(r.odd_h for _, r in wide)
    assert {r.nxc for r in regs} >= {1, 2, 3}
    assert {r.last_wc for r in regs} >= {8, 16, 64}
    assert {r.last_wc for _, r in wide} >= {8, 16, 64}               # a narrower tile after a wide one, and two full ones
    assert {r.wc_changes for _, r in wide} == {False, True}
    assert {r.reorder for r in regs if r.nxc == 1} == {False, True}
    assert {r.reorder for _, r in wide} == {False, True}
    for shape in cvc.WIDE:                                           # every wide shape both ways, where E can decide it
        seen = {r.reorder for c, r in wide if (c.H, c.W) == shape}
        if (dt,) + shape in cvc.ALWAYS_REORDERED:
            assert all(cvc.classify(dt, E, shape[0], shape[1], 32, 4).reorder for E in range(1, 17))
            assert seen == {True}
        else:
            assert seen == {False, True}, shape
    want_chunks = {1, 3, 8} if dt is np.float16 else {2, 6, 16}
    assert {r.chunks for r in regs} == want_chunks and {r.chunks for _, r in wide} == want_chunks
    assert {c.levels for c in cases} == {1, 2, 3, 4} and {c.levels for c, _ in wide} >= {1, 3, 4}
    assert {c.ncam for c in cases} == {1, 2}
    assert any(c.ncam == 2 and any(i == j for i, j in zip(c.ii, c.jj)) for c, _ in wide)   # a stereo edge at nxc > 1
    # odd level sizes (the floors) at nxc > 1
    assert any((c.W >> 1) % 2 == 0 and (c.W >> 2) % 2 == 0 and (c.W >> 3) % 2 == 1 and (c.H >> 1) % 2 == 1 for c, _ in wide)


def test_classifier_on_known_shapes():
    r = cvc.classify(np.float16, 1, 60, 80, 128, 4)                  # TartanAir's 480x640 at 1/8
    assert (r.nptiles, r.ragged_ptile, r.nbands, r.last_band_rows, r.nxc, r.last_wc, r.wc_changes, r.reorder, r.chunks) == \
        (150, False, 8, 4, 2, 16, True, False, 4)
    r = cvc.classify(np.float16, 2, 10, 72, 32, 4)
    assert (r.nptiles, r.ragged_ptile, r.nbands, r.last_band_rows, r.odd_h, r.nxc, r.last_wc, r.reorder) == \
        (23, True, 2, 2, False, 2, 8, False)
    assert cvc.classify(np.float16, 8, 10, 72, 32, 4).reorder
    r = cvc.classify(np.float32, 1, 11, 128, 96, 4)
    assert (r.P, r.nptiles, r.odd_h, r.last_band_rows, r.nxc, r.last_wc, r.wc_changes, r.reorder, r.chunks) == \
        (16, 88, True, 3, 2, 64, False, True, 6)
    # the shapes the older tests use never leave nxc == 1
    for h, w in [(48, 64), (30, 40), (24, 32), (16, 24), (8, 8)]:
        assert cvc.classify(np.float16, 1, h, w, 128, 4).nxc == 1


# ------------------------------------------------------------------------------------------------------ write maps
@pytest.mark.parametrize("dt", TYPES)
@pytest.mark.parametrize("H,W", cvc.SHAPES)
def test_write_maps_cover_a_slot_exactly_once(dt, H, W):
    """From the address arithmetic alone: every element of every level of the slot is written exactly once, and no
    write falls outside the slot.  The sentinel guards of the GPU test confirm it on the device."""
    for levels in (4, 1) if (H, W) == (10, 72) else (4,):
        counts, outside = cvc.write_counts(dt, H, W, levels)
        assert outside == 0
        assert len(counts) == levels
        for l, c in enumerate(counts):
            assert c.size == H * W * (H >> l) * (W >> l)
            assert c.min() == 1 and c.max() == 1, (l, int(c.min()), int(c.max()))


def test_write_maps_notice_a_wrong_map():
    """The restatement is not vacuous: it is a model of addresses, so a shape outside the kernel's rules (W % 8 != 0
    is what makes a tile's last 16-byte piece hang over the row) must show double writes."""
    counts, outside = cvc.write_counts(np.float16, 8, 12, 1)
    assert counts[0].max() > 1 or outside > 0


# ---------------------------------------------------------------------------------- the reference in the new regimes
def test_reference_overflow_populations():
    f = cvc.overflow_fmaps()
    H, W, C = cvc.OVERFLOW_SHAPE
    assert f.shape == (2, 1, C, H, W) and f.dtype == np.float16 and np.all(np.isfinite(f))
    assert cvc.classify(np.float16, 1, H, W, C, 4).nxc > 1
    a, b = ref.operands(f, [0], [1], np.float16)
    lo, hi, mid = ref.level0_interval(a, b, np.float16)
    x = ref.level0_exact(a, b)
    assert np.abs(x).max() < 1e7 and not np.any(np.isnan(lo)) and not np.any(np.isnan(hi))   # far from fp32 overflow
    assert np.all(lo <= hi)
    pos, neg = (lo == np.inf) & (hi == np.inf), (lo == -np.inf) & (hi == -np.inf)
    fin = np.isfinite(lo) & np.isfinite(hi)
    print(f"+inf {int(pos.sum())}, -inf {int(neg.sum())}, finite {int(fin.sum())}, undecided {int((~(pos | neg | fin)).sum())}")
    assert pos.sum() >= 100 and neg.sum() >= 100 and fin.sum() >= 100
    assert np.all(mid[pos] == np.inf) and np.all(mid[neg] == -np.inf)
    # every x-tile and both bands hold all three populations
    q = np.arange(H * W)
    for sel in [(q % W) < 64, (q % W) >= 64, (q // W) >= 8]:
        assert pos[0][:, sel].any() and neg[0][:, sel].any() and fin[0][:, sel].any()
    # torch's own half matmul lies in the interval as well: rounding to T is monotone, infinities included
    vol = torch.matmul(torch.from_numpy(a[0]).float().T, torch.from_numpy(b[0]).float()).half().numpy()
    assert np.all(lo[0] <= vol) and np.all(vol <= hi[0])
    # and the pooled levels hold NaN (inf + -inf), +-inf and finite values
    with np.errstate(invalid="ignore"):
        l1 = ref.pool(mid.reshape(1, H, W, H, W), np.float16)
    assert np.isnan(l1).sum() >= 100 and np.isposinf(l1).sum() >= 100 and np.isneginf(l1).sum() >= 100


@pytest.mark.parametrize("dt", TYPES)
def test_pool_over_inf_and_nan_is_avg_pool2d(dt):
    """NaN where avg_pool2d gives NaN (payload and sign not compared), the same bits everywhere else."""
    rng = np.random.default_rng(5)
    x = rng.normal(0, 1, (8, 11, 36)).astype(dt)
    kind = rng.integers(0, 8, x.shape)
    x[kind == 0], x[kind == 1], x[kind == 2] = np.inf, -np.inf, np.nan
    x[kind == 3] = np.finfo(dt).max                      # four of these overflow T but not fp32 (half); inf for fp32
    lvl, t = x, torch.from_numpy(x)[:, None]
    seen_nan = seen_inf = 0
    for _ in range(3):
        with np.errstate(invalid="ignore", over="ignore"):
            lvl = ref.pool(lvl, dt)
        t = F.avg_pool2d(t, 2, stride=2)
        want = t[:, 0].numpy()
        assert lvl.shape == want.shape and lvl.dtype == want.dtype
        nan = np.isnan(want)
        assert np.array_equal(np.isnan(lvl), nan)
        assert np.array_equal(np.where(nan, 0, lvl).view(np.uint8), np.where(nan, 0, want).view(np.uint8))
        seen_nan += int(nan.sum())
        seen_inf += int(np.isinf(want).sum())
    assert seen_nan > 50 and seen_inf > 20


@pytest.mark.parametrize("dt", TYPES)
def test_reference_confines_a_nan_feature_to_one_row_and_one_column(dt):
    f, pstar, qstar = cvc.nan_fmaps(dt)
    H, W, C = cvc.NAN_SHAPE
    r = cvc.classify(dt, 2, H, W, C, 4)
    assert r.nxc > 1 and pstar // r.P == r.nptiles - 1 and (qstar % W) // cvc.TILE_W == r.nxc - 1 and qstar // W == H - 1
    assert int(np.isnan(f).sum()) == 2
    a, b = ref.operands(f, [0, 2], [1, 3], dt)
    lo, hi, mid = ref.level0_interval(a, b, dt)
    want = np.zeros((2, H * W, H * W), bool)
    want[0, pstar, :] = True
    want[0, :, qstar] = True
    for v in (lo, hi, mid):
        assert np.array_equal(np.isnan(v), want)
    # level 1 of the reference: NaN exactly in the cells that pool the NaN row / column
    with np.errstate(invalid="ignore"):
        l1 = ref.pool(mid.reshape(2, H, W, H, W), dt).reshape(2, H * W, H >> 1, W >> 1)
    w1 = np.zeros_like(l1, bool)
    w1[0, pstar] = True
    w1[0, :, (qstar // W) >> 1, (qstar % W) >> 1] = True
    assert np.array_equal(np.isnan(l1), w1)
