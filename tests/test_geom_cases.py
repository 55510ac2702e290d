"""CPU proof, from the fp64 reference alone (oracle/geom.py), that the cases of tests/geom_cases.py exercise what the
GPU tests (tests/test_gpu_geom.py) claim and stay inside the cap of the band rule -- so that a later edit of a seed
cannot silently turn one of those tests vacuous."""
import numpy as np
import pytest

import geom_cases as gc
from oracle import geom

CASES = gc.all_cases()


def _both_sides(Z, thr, pixels):
    """pixels on both sides of a threshold: at least 5 % each (one pixel at least for the 32-pixel cases)."""
    lo, hi = int((Z <= thr).sum()), int((Z > thr).sum())
    need = max(1, int(0.05 * pixels))
    return lo >= need and hi >= need, (lo, hi, need)


@pytest.mark.parametrize("case", CASES, ids=[c.id for c in CASES])
def test_case_is_within_the_cap_and_populates_every_branch(case):
    c = case
    _, _, m = geom.projmap(c.poses, c.disps, c.K, c.ii, c.jj, margins=True)
    assert gc.in_z_band(m["Z"], m["mag"], gc.Z_PROJMAP).sum() <= gc.cap(c.pixels)
    for thr in gc.Z_PROJMAP:
        ok, why = _both_sides(m["Z"], thr, c.pixels)
        assert ok, ("projmap", thr, why)
    for K in (c.K, c.K_frames):
        _, _, r = geom.reproject(c.poses, c.disps, K, c.ii_st, c.jj_st, margins=True)
        assert gc.in_z_band(r["Z"], r["mag"], gc.Z_REPROJECT).sum() <= gc.cap(c.pixels)
        for thr in gc.Z_REPROJECT:
            ok, why = _both_sides(r["Z"], thr, c.pixels)
            assert ok, ("reproject", thr, why)
    _, f = geom.frame_distance(c.poses, c.disps, c.K, c.ii, c.jj, 0.5, margins=True)
    band = gc.in_z_band(f["Z"], f["mag"], (geom.KERNEL_MIN_DEPTH,)) | gc.in_z_band(f["Zt"], f["mag"], (geom.KERNEL_MIN_DEPTH,))
    assert band.sum() <= gc.cap(c.pixels)
    need = np.array([gc.share_margin(n, c.H * c.W) for n in band.sum(axis=(1, 2))])
    for beta in gc.BETAS:
        dist, share = geom.frame_distance_from_parts(f, beta)
        assert (np.abs(share - 0.75) > need).all(), (beta, float((np.abs(share - 0.75) - need).min()))
        assert (dist == 1000.0).any() and (dist != 1000.0).any(), beta     # edges on both sides of 0.75


def test_negating_every_quaternion_leaves_the_reference_unchanged():
    c = gc.Case(17, 24, 60.0, "nonunit")
    a, b = geom.projmap(c.poses, c.disps, c.K, c.ii, c.jj), geom.projmap(c.twin().poses, c.disps, c.K, c.ii, c.jj)
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])


def test_variants_change_the_poses_the_way_they_say():
    base = gc.Case(9, 19, 20.0, "plain")
    neg, non, sh = (gc.Case(9, 19, 20.0, v) for v in gc.VARIANTS)
    assert np.array_equal(neg.poses[0::2], base.poses[0::2]) and np.array_equal(neg.poses[1::2, 3:], -base.poses[1::2, 3:])
    n = np.linalg.norm(non.poses[:, 3:].astype(np.float64), axis=1)
    assert np.allclose(n[[0, 6]], 1.001, atol=1e-6) and np.allclose(n[3], 0.999, atol=1e-6) and np.allclose(n[[1, 2, 4, 5, 7]], 1, atol=1e-6)
    assert np.abs(sh.poses[:, :3]).max() > 50 and np.array_equal(sh.poses[:, 3:], base.poses[:, 3:])
    # a shifted world leaves every relative pose, hence every result, where it was (up to the float32 poses)
    a, b = geom.projmap(base.poses, base.disps, base.K, base.ii, base.jj, margins=True), \
        geom.projmap(sh.poses, sh.disps, sh.K, sh.ii, sh.jj, margins=True)
    assert np.abs(a[2]["Z"] - b[2]["Z"]).max() < 1e-3


def test_anisotropic_cases_have_four_different_intrinsics():
    aniso = [c for c in CASES if c.variant == gc.ANISO]
    assert sorted((c.H, c.W, c.rot_deg) for c in aniso) == sorted((H, W, r) for (H, W) in ((9, 19), (48, 64)) for r in gc.ROT_DEG)
    for c in aniso:
        plain = gc.Case(c.H, c.W, c.rot_deg, "plain")
        assert np.array_equal(c.poses, plain.poses) and np.array_equal(c.target, plain.target)
        for K in (c.K, *c.K_frames):
            K = K.astype(np.float64)
            assert all(abs(K[a] - K[b]) >= 0.1 * max(K[a], K[b]) for a in range(4) for b in range(a)), K
        r = c.K_frames.astype(np.float64) / c.K_frames[0]
        assert all(np.ptp(r[f]) > 5e-3 for f in range(1, 8))                # no frame a common multiple of frame 0
    assert all(c.K[0] == c.K[1] == c.K[2] for c in CASES if c.variant != gc.ANISO)


def test_depth_ladder_levels_decide_every_flag():
    L = gc.depth_ladder()
    lv = gc.LEVELS[L["level"]]
    coords, valid, m = geom.projmap(L["poses"], L["disps"], L["K"], L["ii"], L["jj"], margins=True)
    back = ~L["forward"]
    assert np.abs(m["Z"][back] - lv[back]).max() < 1e-6 and np.abs(m["Z"][L["forward"]] - 1.5).max() < 1e-6
    for thr in (0.01, 0.1, 0.2, 0.25):                          # no level within 4e-3 of a constant
        assert np.abs(m["Z"] - thr).min() > 4e-3
    assert np.array_equal(valid[..., 0] == 1.0, lv > 0.25)
    x, y = np.meshgrid(np.arange(gc.LADDER_W), np.arange(gc.LADDER_H))
    fell = (coords[..., 0] == x) & (coords[..., 1] == y)
    assert np.array_equal(fell, L["itself"]) and np.array_equal(m["Z"] <= 0.01, L["level"] == 0)
    _, rvalid, r = geom.reproject(L["poses"], L["disps"], L["K"], L["ii"], L["jj"], margins=True)
    assert np.array_equal(rvalid[..., 0] == 1.0, lv > 0.2) and np.array_equal(r["Z"] < 0.1, lv < 0.1)
    for beta in gc.BETAS:
        dist, share = geom.frame_distance_from_parts(geom.frame_distance(L["poses"], L["disps"], L["K"], L["ii"], L["jj"],
                                                                        beta, margins=True)[1], beta)
        n = (lv > 0.25).sum(axis=(1, 2))
        assert np.allclose(share, n / (gc.LADDER_H * gc.LADDER_W))
        assert np.abs(share - 0.75).min() > 0.03
        # patterns "a" (edges 4, 5) pass only with the threshold at 0.25 or below, "b" (6, 7) fail only at 0.25 or above
        assert list(dist == 1000.0) == [True, True, True, True, False, False, True, True, False]
        n24, n26 = (lv > 0.24).sum(axis=(1, 2)) / 273.0, (lv > 0.26).sum(axis=(1, 2)) / 273.0
        assert (n26[4:6] < 0.75).all() and (n24[6:8] > 0.75).all()


@pytest.mark.parametrize("n", gc.MATRIX_N)
@pytest.mark.parametrize("shape", gc.MATRIX_SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_matrix_cases_decide_the_1000_pattern(n, shape):
    _matrix_case_decides(n, shape, gc.matrix_case(n, *shape))


def test_anisotropic_matrix_case_decides_the_1000_pattern():
    n, H, W = gc.MATRIX_ANISO
    mc = gc.matrix_case(n, H, W, aniso=True)
    assert np.array_equal(mc["K"], gc.aniso_K(H, W)) and np.array_equal(mc["poses"], gc.matrix_case(n, H, W)["poses"])
    _matrix_case_decides(n, (H, W), mc)


def _matrix_case_decides(n, shape, mc):
    ii, jj, parts, nband = gc.matrix_reference(mc)
    hw = shape[0] * shape[1]
    assert nband.sum() <= gc.cap(n * n * hw)
    need = np.array([gc.share_margin(b, hw) for b in nband])
    for beta in gc.BETAS:
        dist, share = geom.frame_distance_from_parts(parts, beta)
        assert (np.abs(share - 0.75) > need).all(), (beta, float((np.abs(share - 0.75) - need).min()))
        assert (dist[ii == jj] < 1e-6).all()                   # a frame against itself: no flow
        if n >= 31:
            off = ii != jj
            assert (dist[off] == 1000.0).mean() > 0.02 and (dist[off] != 1000.0).mean() > 0.2, beta


@pytest.mark.parametrize("case", CASES, ids=[c.id for c in CASES])
def test_depth_filter_cases_are_within_the_cap(case):
    dc = gc.depth_filter_case(case)
    cnt, band = geom.depth_filter(dc["poses"], dc["disps"], dc["K"], dc["ix"], dc["thresh"], margins=True)
    live = dc["live"]
    assert band().any(axis=1).sum() <= gc.cap(dc["pixels"])
    assert (cnt[live:] == 0).all()                             # indices outside the buffer
    d = dc["disps"]
    if case.H > 1:
        # counts on both sides, and disparities that differ between the corners of a pixel
        assert (cnt[:live] == 0).mean() > 0.05 and (cnt[:live] > 0).mean() > 0.01 and cnt[:live].max() >= 1
        assert (np.abs(np.diff(d, axis=1)) > 1e-4).mean() > 0.9 and (np.abs(np.diff(d, axis=2)) > 1e-4).mean() > 0.9
    else:
        assert (cnt == 0).all()                                # one row: no 2 x 2 corner fits
