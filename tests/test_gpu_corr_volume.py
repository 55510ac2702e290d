"""corr_volume_pyramid on the device against tests/corr_volume_ref.py.

Level 0 -- the criterion is derived, not measured: with x the exact value (fp64 dot product of the T(f / 4) operands)
and beta = (C + 2) 2^-24 sum_c |a_c b_c| (first-order bound for C products and C - 1 additions rounded to fp32 in any
order) the fp32 sum lies in [x - beta, x + beta]; rounding to T is monotone, so EVERY entry must satisfy
T(x - beta) <= dev <= T(x + beta).  The share of entries with dev != T(x) is printed for information only.
Levels 1-3 -- bit-exact: dev[l+1] == pool(dev[l]), the restatement applied to the device's own level l, which is how
the reference defines level l+1."""
import numpy as np
import pytest
import torch

import corr_volume_ref as ref

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
DT = {np.float16: torch.float16, np.float32: torch.float32}


def _t(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _bits(x):
    return np.ascontiguousarray(x).view(np.uint8)


def _fmaps(seed, nbuf, ncam, C, h, w, npdt, scale=1.0):
    rng = np.random.default_rng(seed)
    shape = (nbuf, C, h, w) if ncam is None else (nbuf, ncam, C, h, w)
    return (rng.normal(0, 1, shape) * scale).astype(npdt)


def _check(db, fmaps, ii, jj, levels, npdt, label):
    pyr = db.corr_volume_pyramid(_t(fmaps), _t(np.asarray(ii, np.int64)), _t(np.asarray(jj, np.int64)), levels)
    torch.cuda.synchronize()
    h, w = fmaps.shape[-2:]
    E = len(ii)
    assert len(pyr) == levels
    dev = []
    for l, p in enumerate(pyr):
        assert tuple(p.shape) == (E, h, w, h >> l, w >> l) and p.dtype == DT[npdt] and p.is_contiguous()
        dev.append(p.cpu().numpy())
    a, b = ref.operands(fmaps, ii, jj, npdt)
    lo, hi, mid = ref.level0_interval(a, b, npdt)
    d0 = dev[0].reshape(E, h * w, h * w)
    print(f"{label}: share of level-0 entries != T(x): {np.mean(d0 != mid):.2e}; outside the interval: "
          f"{int(np.sum(~((lo <= d0) & (d0 <= hi))))}")
    assert np.all(np.isfinite(d0))
    assert np.all(lo <= d0) and np.all(d0 <= hi)
    for l in range(levels - 1):
        want = ref.pool(dev[l], npdt)
        print(f"{label}: level {l + 1} entries != pool(level {l}): {int(np.sum(_bits(want) != _bits(dev[l + 1])))}")
        assert np.array_equal(_bits(want), _bits(dev[l + 1]))
    return dev


@pytest.mark.parametrize("npdt", [np.float16, np.float32])
def test_stereo_and_out_of_range_edges_48x64(backends, npdt):
    """E = 3, ncam = 2: a plain edge, a stereo edge (ii == jj reads camera 1), an edge with an index out of range."""
    fmaps = _fmaps(1, 4, 2, 128, 48, 64, npdt)
    dev = _check(backends, fmaps, [0, 2, 1], [3, 2, 4], 4, npdt, f"48x64 {npdt.__name__}")
    assert np.any(dev[0][0] != 0) and np.any(dev[0][1] != 0)
    for lvl in dev:
        assert not lvl[2].any()
    # the stereo edge really read camera 1: against camera 0 it would be the Gram matrix of one map (symmetric)
    g = dev[0][1].reshape(48 * 64, 48 * 64)
    assert not np.array_equal(g, g.T)


@pytest.mark.parametrize("npdt", [np.float16, np.float32])
def test_floors_30x40(backends, npdt):
    fmaps = _fmaps(2, 3, 1, 128, 30, 40, npdt)
    dev = _check(backends, fmaps, [0, 1], [1, 2], 4, npdt, f"30x40 {npdt.__name__}")
    assert [d.shape[3:] for d in dev] == [(30, 40), (15, 20), (7, 10), (3, 5)]


@pytest.mark.parametrize("npdt", [np.float16, np.float32])
@pytest.mark.parametrize("C", [32, 256])
def test_channel_counts_16x24(backends, npdt, C):
    fmaps = _fmaps(3 + C, 3, 1, C, 16, 24, npdt)
    _check(backends, fmaps, [0, 2], [1, 0], 4, npdt, f"16x24 C={C} {npdt.__name__}")


@pytest.mark.parametrize("npdt", [np.float16, np.float32])
def test_one_level_and_four_dim_input(backends, npdt):
    fmaps = _fmaps(5, 3, None, 128, 16, 24, npdt)       # [nbuf, C, h, w]
    one = _check(backends, fmaps, [0, 1], [2, 0], 1, npdt, f"levels=1 {npdt.__name__}")
    four = _check(backends, fmaps, [0, 1], [2, 0], 4, npdt, f"levels=4 {npdt.__name__}")
    assert np.array_equal(_bits(one[0]), _bits(four[0]))
    five = _check(backends, fmaps[:, None], [0, 1], [2, 0], 4, npdt, f"5-dim {npdt.__name__}")
    for x, y in zip(four, five):
        assert np.array_equal(_bits(x), _bits(y))


def test_half_subnormal_operands(backends):
    """Features scaled by 2^-13: f / 4 is subnormal in half and must be kept (rounded, not flushed)."""
    fmaps = _fmaps(6, 2, 1, 128, 16, 24, np.float16, scale=2.0 ** -13)
    a, _ = ref.operands(fmaps, [0], [1], np.float16)
    assert np.mean((a != 0) & (np.abs(a) < 2.0 ** -14)) > 0.5
    dev = _check(backends, fmaps, [0], [1], 4, np.float16, "subnormal half")
    assert np.any(dev[0] != 0)


@pytest.mark.parametrize("npdt", [np.float16, np.float32])
def test_slots_batch_independence_and_determinism(backends, npdt):
    db = backends
    h, w, levels = 16, 24, 4
    fmaps = _t(_fmaps(7, 4, 1, 128, h, w, npdt))
    ii, jj = _t(np.array([0, 3], np.int64)), _t(np.array([1, 2], np.int64))
    plain = [p.cpu().numpy() for p in db.corr_volume_pyramid(fmaps, ii, jj, levels)]
    # capacity buffers pre-filled with a NaN pattern; E = 2 built at offset 3
    pat = 0x7E5A if npdt is np.float16 else 0x7FC5A5A5
    idt = torch.int16 if npdt is np.float16 else torch.int32
    cap = 6
    out = [torch.full((cap, h, w, h >> l, w >> l), pat, dtype=idt, device=DEV).view(DT[npdt]) for l in range(levels)]
    views = db.corr_volume_pyramid(fmaps, ii, jj, levels, out=out, offset=3)
    torch.cuda.synchronize()
    for l in range(levels):
        o = out[l].view(idt).cpu().numpy()
        assert views[l].data_ptr() == out[l][3:5].data_ptr() and tuple(views[l].shape) == (2, h, w, h >> l, w >> l)
        assert np.array_equal(_bits(o[3:5]), _bits(plain[l]))
        assert np.all(o[:3] == pat) and np.all(o[5:] == pat)
    # one edge at a time == all at once == a second run
    again = [p.cpu().numpy() for p in db.corr_volume_pyramid(fmaps, ii, jj, levels)]
    for e in range(2):
        single = db.corr_volume_pyramid(fmaps, ii[e:e + 1].contiguous(), jj[e:e + 1].contiguous(), levels)
        for l in range(levels):
            assert np.array_equal(_bits(single[l].cpu().numpy()[0]), _bits(plain[l][e]))
    for l in range(levels):
        assert np.array_equal(_bits(again[l]), _bits(plain[l]))


class _CorrBlock:
    """CorrBlock replica (droid_slam/modules/corr.py:24-50, 52-61) whose __init__ is the one call."""

    def __init__(self, db, fmaps, ii, jj, num_levels=4, radius=3):
        self.db, self.num_levels, self.radius = db, num_levels, radius
        self.corr_pyramid = db.corr_volume_pyramid(fmaps, ii, jj, num_levels)

    def cat(self, other):
        for i in range(self.num_levels):
            self.corr_pyramid[i] = torch.cat([self.corr_pyramid[i], other.corr_pyramid[i]], 0)
        return self

    def __call__(self, coords):
        b, n, h, w, _ = coords.shape
        c = coords.permute(0, 1, 4, 2, 3).contiguous().view(b * n, 2, h, w)
        out, = self.db.corr_pyramid_forward(self.corr_pyramid, c, self.radius)
        return out.view(b, n, -1, h, w)


def test_caller_shaped_corr_block(backends):
    """Two blocks joined by stock torch.cat equal one build of the concatenated edge list; the pyramid goes through
    corr_pyramid_forward and corr_index_forward as it is, and the lookup agrees with the stock-built pyramid's."""
    from callers import VolumeLookup
    db = backends
    h, w, C = 24, 32, 128
    fm_np = _fmaps(8, 5, 1, C, h, w, np.float16)
    fmaps = _t(fm_np)
    ii = _t(np.array([0, 1, 2, 4], np.int64))
    jj = _t(np.array([1, 0, 3, 2], np.int64))
    whole = _CorrBlock(db, fmaps, ii, jj)
    joined = _CorrBlock(db, fmaps, ii[:3].contiguous(), jj[:3].contiguous()).cat(
        _CorrBlock(db, fmaps, ii[3:].contiguous(), jj[3:].contiguous()))
    for x, y in zip(whole.corr_pyramid, joined.corr_pyramid):
        assert x.shape == y.shape and torch.equal(x.view(torch.int16), y.view(torch.int16))
    stock = VolumeLookup(fmaps[ii, 0][None], fmaps[jj, 0][None])
    for l, (x, y) in enumerate(zip(whole.corr_pyramid, stock.pyramid)):
        assert x.shape == y.shape and x.dtype == y.dtype and x.is_contiguous()
    rng = np.random.default_rng(9)
    coords = _t(np.stack([rng.uniform(-2, w + 1, (1, 4, h, w)), rng.uniform(-2, h + 1, (1, 4, h, w))], -1).astype(np.float32))
    got = whole(coords)
    assert tuple(got.shape) == (1, 4, 4 * 49, h, w)
    c = coords.permute(0, 1, 4, 2, 3).contiguous().view(4, 2, h, w)
    per_level = torch.cat([db.corr_index_forward(whole.corr_pyramid[l], c / 2 ** l, 3)[0].view(4, -1, h, w)
                           for l in range(4)], 1)
    assert torch.equal(got[0].view(torch.int16), per_level.view(torch.int16))
    want = stock(coords)
    err = (got.float() - want.float()).abs().max().item()
    scale = want.float().abs().max().item()
    print(f"lookup through the device-built pyramid vs the stock-built one: max |diff| {err:.3e} of {scale:.3e}")
    assert err <= 2e-2 * scale   # two half pyramids whose level 0 differs by summation order: a few half ulps of the scale
