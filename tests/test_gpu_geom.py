"""GPU parity of the geometry operators against the fp64 oracle.

The first tests run on one input (cfg1).  The case tests further down run on tests/geom_cases.py: ragged shapes, wild
poses, thresholds, with the band rule for decisions and a value tolerance in units of 2^-24 * scale that is 4 x the
error of the C oracle's own float32 variant on the same case (at least 4 units, at most the derived 64).  Float32-oracle
errors measured on the MI355X, worst over the 42 cases, and the kernel's next to them:
    projmap         3.2 units  (182 on the 100 m trajectories: the C oracle's relative pose is float32)   kernel 1.7
    frame_distance  150 units  (the C oracle sums up to 12288 pixels sequentially in float32)             kernel 0.45
    iproj           1.5 units                                                                             kernel 1.35
    reproject       no float32 oracle: derived bound 64 units                                             kernel 2.0
"""
import numpy as np
import pytest

from util import to_dev

pytestmark = pytest.mark.gpu


def _torch():
    import torch
    assert torch.cuda.is_available()
    return torch


@pytest.fixture(scope="module")
def prob():
    from droid_backends import synth
    return synth.make_config("cfg1")


def test_frame_distance(backends, oracle, prob):
    torch = _torch()
    d = to_dev(prob, torch)
    for beta in (0.3, 0.0, 1.0):
        got = backends.frame_distance(d["poses"], d["disps"], d["intrinsics"], d["ii"], d["jj"], beta).cpu().numpy()
        ref = oracle.frame_distance(prob.poses, prob.disps, prob.intrinsics, prob.ii, prob.jj, beta)
        assert np.abs(got - ref).max() < 1e-4 * max(1.0, np.abs(ref).max())


def test_frame_distance_flags_low_overlap(backends, oracle, prob):
    torch = _torch()
    d = to_dev(prob, torch)
    poses = prob.poses.copy()
    poses[3, :3] += np.array([0, 0, -8.0], np.float32)  # push frame 3 far behind
    got = backends.frame_distance(torch.from_numpy(poses).cuda(), d["disps"], d["intrinsics"], d["ii"], d["jj"], 0.3)
    ref = oracle.frame_distance(poses, prob.disps, prob.intrinsics, prob.ii, prob.jj, 0.3)
    assert (ref == 1000.0).any()
    assert np.array_equal(got.cpu().numpy() == 1000.0, ref == 1000.0)


def test_projmap(backends, oracle, prob):
    torch = _torch()
    d = to_dev(prob, torch)
    coords, valid = backends.projmap(d["poses"], d["disps"], d["intrinsics"], d["ii"], d["jj"])
    rc, rv = oracle.projmap(prob.poses, prob.disps, prob.intrinsics, prob.ii, prob.jj)
    assert np.abs(coords.cpu().numpy() - rc).max() < 2e-3  # pixels, fp32 projection
    assert np.mean(valid.cpu().numpy() != rv) < 1e-4


def test_iproj(backends, oracle, prob):
    torch = _torch()
    d = to_dev(prob, torch)
    pts = backends.iproj(d["poses"], d["disps"], d["intrinsics"]).cpu().numpy()
    ref = oracle.iproj(prob.poses, prob.disps, prob.intrinsics)
    assert np.abs(pts - ref).max() < 1e-4 * np.abs(ref).max()


def test_depth_filter_counts_consistent_neighbours(backends, prob):
    """With GT poses/disparities every interior pixel agrees with its temporal neighbours."""
    torch = _torch()
    poses = torch.from_numpy(prob.gt_poses.astype(np.float32)).cuda()
    disps = torch.from_numpy(prob.gt_disps.astype(np.float32)).cuda()
    intr = torch.from_numpy(prob.intrinsics).cuda()
    ix = torch.tensor([3, 4], dtype=torch.int64, device="cuda")
    thresh = torch.full((2,), 0.2, dtype=torch.float32, device="cuda")
    cnt = backends.depth_filter(poses, disps, intr, ix, thresh).cpu().numpy()
    assert cnt.shape == (2, 48, 64)
    assert cnt.max() <= 6 and cnt[:, 8:-8, 8:-8].mean() > 3.0


def _reproject_case(prob, rng, per_frame_K):
    poses = prob.poses.copy()
    poses[5, :3] += np.array([0, 0, -6.0], np.float32)      # some edges end behind the camera
    nb = prob.disps.shape[0]
    st = np.array([2, nb - 1, nb // 2])
    ii = np.concatenate([prob.ii, st])                       # + three stereo edges (ii == jj)
    jj = np.concatenate([prob.jj, st])
    K = prob.intrinsics.astype(np.float32)
    if per_frame_K:
        K = np.stack([K * np.float32(1.0 + 0.01 * (f % 7)) for f in range(prob.disps.shape[0])]).astype(np.float32)
    H, W = prob.disps.shape[1:]
    target = rng.uniform(-20, 90, (len(ii), H, W, 2)).astype(np.float32)
    return poses, ii, jj, K, target


@pytest.mark.parametrize("per_frame_K", [False, True])
def test_reproject_and_motion_features(backends, prob, per_frame_K):
    """Fused DepthVideo.reproject + motion features against the numpy restatement: coordinates
    within the derived 64 units of 2^-24 * coord_scale, validity identical outside the band of the depth thresholds,
    features clamped to 64."""
    torch = _torch()
    from oracle import geom
    rng = np.random.default_rng(11)
    poses, ii, jj, K, target = _reproject_case(prob, rng, per_frame_K)
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()
    c, v, m = backends.reproject(t(poses), t(prob.disps), t(K), t(ii), t(jj), t(target))
    rm, rc, rv = geom.motion_features(poses, prob.disps, K, ii, jj, target)
    c, v, m = c.cpu().numpy()[0], v.cpu().numpy()[0], m.cpu().numpy()[0]
    assert c.shape == rc.shape and v.shape == rv.shape and m.shape == rm.shape
    _, _, r = geom.reproject(poses, prob.disps, K, ii, jj, margins=True)
    band = gc.in_z_band(r["Z"], r["mag"], gc.Z_REPROJECT)    # coordinates blow up only next to the clamp: the band names it
    assert band.sum() <= gc.cap(band.size) and np.array_equal(v[~band], rv[~band])
    scale = _proj_scales(r["Kj"], r, r["Zc"])
    assert _units(c, rc, scale, np.broadcast_to(~band[..., None], scale.shape)) <= G.Z_BAND_C
    assert np.abs(m - rm).max() < 5e-3 and np.abs(m).max() <= 64.0
    assert (rv == 0).any() and (np.abs(rm) == 64.0).any()    # the case exercises both branches
    # plain reproject (no target) returns the same coordinates; motion_features() orders (motn, coords, mask)
    c2, v2 = backends.reproject(t(poses)[None], t(prob.disps)[None], t(K)[None] if per_frame_K else t(K), t(ii), t(jj))
    assert torch.equal(c2.cpu(), torch.from_numpy(c)[None]) and torch.equal(v2.cpu(), torch.from_numpy(v)[None])
    m3, c3, _ = backends.motion_features(t(poses), t(prob.disps), t(K), t(ii), t(jj), t(target)[None])
    assert torch.equal(m3.cpu(), torch.from_numpy(m)[None]) and torch.equal(c3.cpu(), torch.from_numpy(c)[None])


def test_reproject_rejects_cpu_tensors_and_bad_indices(backends, prob):
    torch = _torch()
    d = to_dev(prob, torch)
    with pytest.raises(RuntimeError):
        backends.reproject(torch.from_numpy(prob.poses), d["disps"], d["intrinsics"], d["ii"], d["jj"])
    ii = d["ii"].clone()
    ii[0] = 10 ** 6
    c, v = backends.reproject(d["poses"], d["disps"], d["intrinsics"], ii, d["jj"])
    assert float(c[0, 0].abs().max()) == 0.0 and float(v[0, 0].max()) == 0.0   # out-of-range edge: zeros, no fault


def test_depth_filter_matches_oracle(backends, prob):
    """depth_filter counts (droid_kernels.cu:661-775) against the numpy restatement: perturbed poses, frames at
    both ends of the buffer (missing neighbours), an index outside the buffer.  The reference compares in
    double precision, the kernel in fp32: pixels whose error sits on the threshold may differ by one count."""
    torch = _torch()
    from oracle import geom
    d = to_dev(prob, torch)
    nb = prob.disps.shape[0]
    ix = np.array([0, 2, nb // 2, nb - 1, nb + 3], dtype=np.int64)
    thresh = np.array([0.05, 0.1, 0.2, 0.02, 0.1], dtype=np.float32)
    got = backends.depth_filter(d["poses"], d["disps"], d["intrinsics"], torch.from_numpy(ix).cuda(),
                                torch.from_numpy(thresh).cuda()).cpu().numpy()
    ref = geom.depth_filter(prob.poses, prob.disps, prob.intrinsics, ix, thresh)
    assert got.shape == ref.shape and got[-1].max() == 0 and ref[-1].max() == 0
    assert np.abs(got - ref).max() <= 1.0 and np.mean(got != ref) < 2e-3
    assert ref[:4].max() >= 3 and (ref[:4] == 0).any()      # the case is not trivial


def test_geom_golden_vectors_on_device(backends):
    """The committed fixtures (tests/golden/geom_golden.npz, altcorr_backward_golden.npz) through the HIP path."""
    import os
    torch = _torch()
    gold = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
    g = np.load(os.path.join(gold, "geom_golden.npz"), allow_pickle=False)
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()
    c, v, m = backends.reproject(t(g["poses"]), t(g["disps"]), t(g["intrinsics"]), t(g["ii"]), t(g["jj"]), t(g["target"]))
    ok = np.abs(g["coords"]).max(axis=-1) < 1e4
    assert np.abs(c.cpu().numpy()[0] - g["coords"])[ok].max() < 2e-3
    assert np.mean(v.cpu().numpy()[0] != g["valid"]) < 1e-3 and np.abs(m.cpu().numpy()[0] - g["motn"]).max() < 5e-3
    cnt = backends.depth_filter(t(g["df_poses"]), t(g["disps"]), t(g["df_intrinsics"]), t(g["df_ix"]), t(g["df_thresh"]))
    assert np.abs(cnt.cpu().numpy() - g["df_counter"]).max() <= 1.0 and np.mean(cnt.cpu().numpy() != g["df_counter"]) < 5e-3
    a = np.load(os.path.join(gold, "altcorr_backward_golden.npz"), allow_pickle=False)
    g1, g2, _ = backends.altcorr_backward(t(a["fmap1"]), t(a["fmap2"]), t(a["coords"]), t(a["corr_grad"]), 3)
    assert np.abs(g1.cpu().numpy() - a["fmap1_grad"]).max() < 2e-5 * np.abs(a["fmap1_grad"]).max()
    assert np.abs(g2.cpu().numpy() - a["fmap2_grad"]).max() < 2e-5 * np.abs(a["fmap2_grad"]).max()


# ---------------------------------------------------------------------------------------------------------------------
# Ragged shapes, wild poses, thresholds: the cases of tests/geom_cases.py (proved non-vacuous and within the cap of the
# band rule by tests/test_geom_cases.py) against the fp64 reference of oracle/geom.py.
#
# Decisions (valid flag, clamp branch, 1000 flag, one count) may differ from the reference only inside the band of
# the threshold (geom_cases.in_z_band: 64 * 2^-24 * mag, the 64 counted in oracle/geom.py); outside it they are
# identical.  Values are measured in units of 2^-24 * scale, scale = what the float32 error of the value grows with
# (oracle.geom.coord_scale for a projected coordinate, mag / |d| + |p| for a point of iproj):
#   * projmap, frame_distance, iproj: 4 x the error of the C oracle's own float32 variant on the same case (the
#     kernel contracts FMAs and orders sums differently: an operation count of the same order, not a wrong formula),
#     floored at 4 units, the rounding of the output itself, which that variant can undercut only by luck;
#   * reproject, depth ladder (only oracle/geom.py covers them): the derived bound, 64 units.
# Float32-oracle errors measured over all cases, in those units (worst case; the 100 m trajectories, where the C
# oracle forms the relative pose in float32 and the kernel in fp64, are the large ones): see DESIGN.md section 5.
import geom_cases as gc                                     # noqa: E402
from oracle import geom as G                                # noqa: E402

CASES = gc.all_cases()
CASE_IDS = [c.id for c in CASES]
UNIT = G.EPS32


def _dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _units(got, ref, scale, where):
    """max over `where` of |got - ref| / (2^-24 scale); 0 for an empty selection"""
    if not where.any():
        return 0.0
    with np.errstate(divide="ignore", invalid="ignore"):
        e = np.abs(got.astype(np.float64) - ref)[where] / (UNIT * scale[where])
    return float(np.nanmax(e))


def _allow(e32):
    """4 x the float32 oracle's error, at least 4 units (the rounding of the output), at most the derived bound (the
    C oracle forms the relative pose and its sums in float32: on the 100 m trajectories and the large maps it is
    far less accurate than the kernel has any reason to be)"""
    return min(4 * max(e32, 1.0), float(G.Z_BAND_C))


def _proj_scales(K, m, Z=None):
    Z = m["Z"] if Z is None else Z
    fx, fy, cx, cy = (K[..., n] for n in range(4))
    return np.stack([G.coord_scale(fx, cx, m["X"][..., 0], Z, m["mag"]), G.coord_scale(fy, cy, m["X"][..., 1], Z, m["mag"])], -1)


@pytest.mark.parametrize("case", CASES, ids=CASE_IDS)
def test_projmap_cases(backends, oracle, case):
    torch = _torch()
    c = case
    args = (_dev(c.disps), _dev(c.K), _dev(c.ii), _dev(c.jj))
    coords, valid = backends.projmap(_dev(c.poses), *args)
    c2, v2 = backends.projmap(_dev(c.twin().poses), *args)
    # q against -q: rel_pose is bilinear in (qi, qj) and act_so3 quadratic in q, products and FMAs are odd in each
    # factor, so every intermediate changes sign exactly or not at all
    assert torch.equal(coords, c2) and torch.equal(valid, v2)
    coords, valid = coords.cpu().numpy(), valid.cpu().numpy()
    rc, rv, m = G.projmap(c.poses, c.disps, c.K, c.ii, c.jj, margins=True)
    band = gc.in_z_band(m["Z"], m["mag"], gc.Z_PROJMAP)
    assert band.sum() <= gc.cap(c.pixels)
    assert np.array_equal(valid[~band], rv[~band]) and (coords[..., 2] == 0).all()
    itself = (m["Z"] <= G.PROJMAP_CLAMP) & ~band
    assert np.array_equal(coords[itself][:, :2], rc[itself][:, :2])          # the fall-back is the pixel, exactly
    scale = _proj_scales(c.K.astype(np.float64), m)
    sel = np.broadcast_to(((m["Z"] > G.PROJMAP_CLAMP) & ~band)[..., None], scale.shape)
    c32, _ = oracle.projmap(c.poses, c.disps, c.K, c.ii, c.jj, precision="f32")
    e32, e = _units(c32[..., :2], rc[..., :2], scale, sel), _units(coords[..., :2], rc[..., :2], scale, sel)
    print(f"projmap {c.id}: float32 oracle {e32:.2f} units, kernel {e:.2f}, band {int(band.sum())}")
    assert e <= _allow(e32), (e, e32)


@pytest.mark.parametrize("case", CASES, ids=CASE_IDS)
def test_frame_distance_cases(backends, oracle, case):
    torch = _torch()
    c = case
    args = (_dev(c.disps), _dev(c.K), _dev(c.ii), _dev(c.jj))
    _, m = G.frame_distance(c.poses, c.disps, c.K, c.ii, c.jj, 0.5, margins=True)
    b1, b2 = gc.in_z_band(m["Z"], m["mag"], (G.KERNEL_MIN_DEPTH,)), gc.in_z_band(m["Zt"], m["mag"], (G.KERNEL_MIN_DEPTH,))
    v1, v2 = m["Z"] > G.KERNEL_MIN_DEPTH, m["Zt"] > G.KERNEL_MIN_DEPTH
    K = c.K.astype(np.float64)
    s1 = _proj_scales(K, m).sum(-1)
    s2 = _proj_scales(K, dict(X=m["Xt"], mag=m["mag"]), m["Zt"]).sum(-1)
    sm = lambda a, w: np.where(w, a, 0.0).sum(axis=(1, 2))
    for beta in gc.BETAS:
        got = backends.frame_distance(_dev(c.poses), *args, beta)
        assert torch.equal(got, backends.frame_distance(_dev(c.twin().poses), *args, beta))     # q against -q
        got = got.cpu().numpy()
        ref, share = G.frame_distance_from_parts(m, beta)
        flag = ref == 1000.0
        assert np.array_equal(got == 1000.0, flag), (beta, share[(got == 1000.0) != flag])     # every edge, no exclusions
        with np.errstate(divide="ignore", invalid="ignore"):
            nvalid = beta * m["n_full"] + (1 - beta) * m["n_trans"]
            scale = (beta * sm(s1, v1) + (1 - beta) * sm(s2, v2)) / nvalid
            # an edge with pixels inside the band may count them or not: their flow, over the valid weight
            slack = (beta * sm(m["flow"], b1) + (1 - beta) * sm(m["flow_t"], b2)) / nvalid
        f32 = oracle.frame_distance(c.poses, c.disps, c.K, c.ii, c.jj, beta, precision="f32")
        clean = ~flag & (slack == 0) & (f32 != 1000.0)
        e32 = _units(f32, ref, scale, clean)
        bad = ~flag & ~(np.abs(got - ref) <= _allow(e32) * UNIT * scale + 2 * slack)
        print(f"frame_distance {c.id} beta {beta}: float32 oracle {e32:.2f} units, kernel {_units(got, ref, scale, clean):.2f}")
        assert not bad.any(), (beta, got[bad], ref[bad])


@pytest.mark.parametrize("case", CASES, ids=CASE_IDS)
def test_iproj_cases(backends, oracle, case):
    torch = _torch()
    c = case
    pts = backends.iproj(_dev(c.poses), _dev(c.disps), _dev(c.K))
    assert torch.equal(pts, backends.iproj(_dev(c.twin().poses), _dev(c.disps), _dev(c.K)))     # q against -q
    ref, m = G.iproj(c.poses, c.disps, c.K, margins=True)
    scale = (m["mag"] / np.abs(c.disps.astype(np.float64)))[..., None] + np.abs(ref)
    sel = np.ones(ref.shape, bool)
    e32 = _units(oracle.iproj(c.poses, c.disps, c.K, precision="f32"), ref, scale, sel)
    e = _units(pts.cpu().numpy(), ref, scale, sel)
    print(f"iproj {c.id}: float32 oracle {e32:.2f} units, kernel {e:.2f}")
    assert e <= _allow(e32), (e, e32)


def test_iproj_zero_disparity_is_inf_or_nan_where_the_reference_says(backends):
    c = gc.Case(17, 24, 20.0, "plain")
    disps = c.disps.copy()
    disps[:, ::3, ::5] = 0.0
    disps[2] = 0.0
    pts = backends.iproj(_dev(c.poses), _dev(disps), _dev(c.K)).cpu().numpy()
    with np.errstate(divide="ignore", invalid="ignore"):
        ref = G.iproj(c.poses, disps, c.K)
    assert np.isinf(ref).any()
    assert np.array_equal(np.isinf(pts), np.isinf(ref)) and np.array_equal(np.isnan(pts), np.isnan(ref))
    assert np.array_equal(np.sign(pts[np.isinf(ref)]), np.sign(ref[np.isinf(ref)]))


@pytest.mark.parametrize("per_frame_K", [False, True], ids=["sharedK", "frameK"])
@pytest.mark.parametrize("case", CASES, ids=CASE_IDS)
def test_reproject_cases(backends, case, per_frame_K):
    torch = _torch()
    c = case
    K = c.K_frames if per_frame_K else c.K
    args = (_dev(c.disps), _dev(K), _dev(c.ii_st), _dev(c.jj_st))
    co, va, mo = backends.reproject(_dev(c.poses), *args, _dev(c.target))
    c2, v2 = backends.reproject(_dev(c.poses), *args)                        # without target: the same pass
    assert torch.equal(co, c2) and torch.equal(va, v2)
    c3, v3, m3 = backends.reproject(_dev(c.twin().poses), *args, _dev(c.target))   # q against -q
    assert torch.equal(co, c3) and torch.equal(va, v3) and torch.equal(mo, m3)
    # the fused motion features are clamp(cat(...)) of the pass's own coordinates, bit for bit
    ys, xs = torch.meshgrid(torch.arange(c.H, device="cuda").float(), torch.arange(c.W, device="cuda").float(), indexing="ij")
    coords0 = torch.stack([xs, ys], -1)
    want = torch.cat([co - coords0, _dev(c.target)[None] - co], -1).permute(0, 1, 4, 2, 3).clamp(-64.0, 64.0)
    assert torch.equal(mo, want)
    co, va = co.cpu().numpy()[0], va.cpu().numpy()[0]
    rc, rv, r = G.reproject(c.poses, c.disps, K, c.ii_st, c.jj_st, margins=True)
    band = gc.in_z_band(r["Z"], r["mag"], gc.Z_REPROJECT)
    assert band.sum() <= gc.cap(c.pixels)
    assert np.array_equal(va[~band], rv[~band])
    scale = _proj_scales(r["Kj"], r, r["Zc"])
    e = _units(co, rc, scale, np.broadcast_to(~band[..., None], scale.shape))
    print(f"reproject {c.id} per_frame_K={per_frame_K}: kernel {e:.2f} units of a bound of {G.Z_BAND_C}, band {int(band.sum())}")
    assert e <= G.Z_BAND_C, e


@pytest.mark.parametrize("case", CASES, ids=CASE_IDS)
def test_depth_filter_cases(backends, case):
    """Counts equal to the reference's except at (pixel, neighbour) decisions inside the band of `thresh` or of an
    integer corner (oracle.geom.depth_filter: band), there by at most the number of such neighbours; indices outside
    the buffer -- 8, -1 and 2**32 + 3, which narrowed to 32 bits would be frame 3 -- give zero planes.  Every shape,
    rotation scale and quaternion variant, on disparities that vary from pixel to pixel."""
    torch = _torch()
    dc = gc.depth_filter_case(case)
    args = (_dev(dc["disps"]), _dev(dc["K"]), _dev(dc["ix"]), _dev(dc["thresh"]))
    got = backends.depth_filter(_dev(dc["poses"]), *args)
    assert torch.equal(got, backends.depth_filter(_dev(dc["twin"]), *args))                    # q against -q
    got = got.cpu().numpy()
    ref, band = G.depth_filter(dc["poses"], dc["disps"], dc["K"], dc["ix"], dc["thresh"], margins=True)
    free = band().sum(axis=1)
    assert (free > 0).sum() <= gc.cap(dc["pixels"])
    assert (got[dc["live"]:] == 0).all()
    assert (np.abs(got - ref) <= free).all(), np.argwhere(np.abs(got - ref) > free)[:8]
    print(f"depth_filter {case.id}: {int((got != ref).sum())} counts differ, {int((free > 0).sum())} pixels in the band")


def test_depth_ladder_decides_every_constant_exactly(backends):
    """Z steps through 0.005 ... 1 (geom_cases.LEVELS), 5e-3 from every constant: valid of projmap (0.25) and of
    reproject (0.2), projmap's fall-back (0.01), reproject's depth-1 substitution (0.1) and the frame_distance
    decision that follows from the 0.25 count, each asserted at every pixel.  Fails if two constants are swapped."""
    L = gc.depth_ladder()
    lv = gc.LEVELS[L["level"]]
    args = (_dev(L["poses"]), _dev(L["disps"]), _dev(L["K"]), _dev(L["ii"]), _dev(L["jj"]))
    coords, valid = (a.cpu().numpy() for a in backends.projmap(*args))
    rc, rv, m = G.projmap(L["poses"], L["disps"], L["K"], L["ii"], L["jj"], margins=True)
    assert np.array_equal(valid[..., 0] == 1.0, lv > 0.25) and np.array_equal(valid, rv)
    x, y = np.meshgrid(np.arange(gc.LADDER_W), np.arange(gc.LADDER_H))
    low = L["level"] == 0                                                    # below 0.01: the pixel itself, exactly;
    assert (coords[..., 0] == x)[low].all() and (coords[..., 1] == y)[low].all()   # at 0.015 it is 60 times further out
    assert np.array_equal(m["Z"] <= 0.01, low)
    K = L["K"].astype(np.float64)
    far = np.broadcast_to((m["Z"] > 0.01)[..., None], (*lv.shape, 2))
    assert _units(coords[..., :2], rc[..., :2], _proj_scales(K, m), far) <= G.Z_BAND_C
    co, va = (a.cpu().numpy()[0] for a in backends.reproject(*args))
    rc2, rv2, r = G.reproject(L["poses"], L["disps"], L["K"], L["ii"], L["jj"], margins=True)
    assert np.array_equal(va[..., 0] == 1.0, lv > 0.2) and np.array_equal(va, rv2)
    # the substitution: below 0.1 the coordinate is f X + c, above it f X / Z + c -- at Z = 0.095 / 0.105 a factor 10 apart
    assert _units(co, rc2, _proj_scales(np.broadcast_to(K, (1, 1, 1, 4)), r, r["Zc"]), np.ones(co.shape, bool)) <= G.Z_BAND_C
    n = (lv > 0.25).sum(axis=(1, 2))
    for beta in gc.BETAS:
        got = backends.frame_distance(*args, beta).cpu().numpy()
        ref, share = G.frame_distance_from_parts(G.frame_distance(L["poses"], L["disps"], L["K"], L["ii"], L["jj"], beta,
                                                                  margins=True)[1], beta)
        assert np.array_equal(got == 1000.0, n / lv[0].size < 0.75) and np.array_equal(got == 1000.0, ref == 1000.0)
        ok = ref != 1000.0
        assert np.abs(got - ref)[ok].max() <= 1e-5 * np.abs(ref[ok]).max()   # means of exact counts: far below a swapped constant


@pytest.mark.parametrize("n", gc.MATRIX_N)
@pytest.mark.parametrize("shape", gc.MATRIX_SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_frame_distance_matrix_cases(backends, oracle, n, shape):
    """n frames of a buffer of n + 3 (one, two and three block columns of 32 targets, full and ragged) against the
    fp64 reference (1000 pattern exact; values within 4 x the float32 C oracle's worst relative error on the case,
    floored at the rounding of a coordinate of the size of the image), against frame_distance on the meshgrid
    (1e-5 of the largest entry that is not 1000: the same arithmetic in another kernel, whose FMA contraction is
    the compiler's), and the
    symmetrisation; the output is over-allocated and must stay untouched behind n * n."""
    _check_matrix_case(backends, oracle, n, shape, gc.matrix_case(n, *shape))


def test_frame_distance_matrix_anisotropic_case(backends, oracle):
    """The same checks with fx, fy, cx, cy pairwise different (geom_cases.aniso_K) at n = 33."""
    n, H, W = gc.MATRIX_ANISO
    _check_matrix_case(backends, oracle, n, (H, W), gc.matrix_case(n, H, W, aniso=True))


def _check_matrix_case(backends, oracle, n, shape, mc):
    torch = _torch()
    H, W = shape
    ii, jj, parts, nband = gc.matrix_reference(mc)
    poses, disps, K = _dev(mc["poses"]), _dev(mc["disps"]), _dev(mc["K"])
    lib = backends._lib.load()
    for beta in gc.BETAS:
        out = torch.full((n * n + 67,), -7.0, dtype=torch.float32, device="cuda")
        backends._lib.check(lib.droid_frame_distance_matrix(poses.data_ptr(), disps.data_ptr(), K.data_ptr(), n, mc["nbuf"], H, W,
                                                            float(beta), out.data_ptr(), torch.cuda.current_stream().cuda_stream),
                            "frame_distance_matrix")
        assert (out[n * n:] == -7.0).all()
        d = out[:n * n].view(n, n)
        assert torch.equal(d, backends.frame_distance_matrix(poses, disps, K, n, beta, bidirectional=False))
        assert torch.equal(.5 * (d + d.t()), backends.frame_distance_matrix(poses, disps, K, n, beta, bidirectional=True))
        pair = backends.frame_distance(poses, disps, K, _dev(ii), _dev(jj), beta)
        got = d.reshape(-1)
        assert torch.equal(got == 1000.0, pair == 1000.0)
        live = pair != 1000.0                                   # the flags are equal (above); 1e-5 of the largest flow
        if bool(live.any()):
            assert float((got - pair)[live].abs().max()) <= 1e-5 * float(pair[live].abs().max())
        got = got.cpu().numpy()
        ref, share = G.frame_distance_from_parts(parts, beta)
        flag = ref == 1000.0
        assert np.array_equal(got == 1000.0, flag), (beta, share[(got == 1000.0) != flag])
        f32 = oracle.frame_distance(mc["poses"], mc["disps"], mc["K"], ii, jj, beta, precision="f32")
        clean = ~flag & (nband == 0) & (f32 != 1000.0) & (ii != jj)
        rel32 = float((np.abs(f32 - ref)[clean] / np.abs(ref[clean])).max()) if clean.any() else 0.0
        tol = 4 * np.maximum(rel32 * np.abs(ref), UNIT * (H + W))
        assert (np.abs(got - ref)[clean] <= tol[clean]).all(), (beta, rel32, float(np.abs(got - ref)[clean].max()))
        assert (got[ii == jj] <= 4 * UNIT * (H + W)).all()


def test_more_edges_than_one_grid_dimension_holds(backends):
    """65536 + 5 edges (frames, selections) at 1 x 8: the edge index no longer fits gridDim.y (65535); the launches
    go in slabs.  Checked against the reference everywhere, the last edges included."""
    torch = _torch()
    rng = np.random.default_rng(5)
    c = gc.Case(1, 8, 20.0, "plain")
    E = 65536 + 5
    ii, jj = rng.integers(0, 8, E), rng.integers(0, 8, E)
    jj = np.where(ii == jj, (jj + 1) % 8, jj)
    dev = (_dev(c.poses), _dev(c.disps), _dev(c.K), _dev(ii), _dev(jj))
    coords, valid = (a.cpu().numpy() for a in backends.projmap(*dev))
    rc, rv, m = G.projmap(c.poses, c.disps, c.K, ii, jj, margins=True)
    band = gc.in_z_band(m["Z"], m["mag"], gc.Z_PROJMAP)
    K = c.K.astype(np.float64)
    sel = np.broadcast_to(((m["Z"] > G.PROJMAP_CLAMP) & ~band)[..., None], (*band.shape, 2))
    assert np.array_equal(valid[~band], rv[~band]) and band[-8:].sum() == 0
    assert _units(coords[..., :2], rc[..., :2], _proj_scales(K, m), sel) <= G.Z_BAND_C
    target = rng.uniform(-5, 12, (E, 1, 8, 2)).astype(np.float32)
    co, va, mo = backends.reproject(*dev, _dev(target))
    rc2, rv2, r = G.reproject(c.poses, c.disps, c.K, ii, jj, margins=True)
    band = gc.in_z_band(r["Z"], r["mag"], gc.Z_REPROJECT)
    assert np.array_equal(va.cpu().numpy()[0][~band], rv2[~band])
    scale = _proj_scales(np.broadcast_to(K, (1, 1, 1, 4)), r, r["Zc"])
    assert _units(co.cpu().numpy()[0], rc2, scale, np.broadcast_to(~band[..., None], scale.shape)) <= G.Z_BAND_C
    coords0 = torch.stack([torch.arange(8, device="cuda").float()[None], torch.zeros(1, 8, device="cuda")], -1)
    want = torch.cat([co - coords0, _dev(target)[None] - co], -1).permute(0, 1, 4, 2, 3).clamp(-64.0, 64.0)
    assert torch.equal(mo, want) and float(mo[0, -5:].abs().max()) > 0
    # iproj: 65541 frames; depth_filter: 65541 selections
    f = rng.integers(0, 8, E)
    pts = backends.iproj(_dev(c.poses[f]), _dev(c.disps[f]), _dev(c.K)).cpu().numpy()
    ref, mi = G.iproj(c.poses[f], c.disps[f], c.K, margins=True)
    scale = (mi["mag"] / np.abs(c.disps[f].astype(np.float64)))[..., None] + np.abs(ref)
    assert _units(pts, ref, scale, np.ones(ref.shape, bool)) <= G.Z_BAND_C and np.abs(pts[-5:]).max() > 0
    dc = gc.depth_filter_case(gc.Case(9, 19, 1.0, "plain"))
    ix = rng.integers(0, 8, E)
    th = np.full(E, 0.1, np.float32)
    cnt = backends.depth_filter(_dev(dc["poses"]), _dev(dc["disps"]), _dev(dc["K"]), _dev(ix), _dev(th)).cpu().numpy()
    one, band1 = G.depth_filter(dc["poses"], dc["disps"], dc["K"], np.arange(8), np.full(8, 0.1, np.float32), margins=True)
    assert (np.abs(cnt - one[ix]) <= band1().sum(axis=1)[ix]).all() and cnt[-5:].max() > 0
