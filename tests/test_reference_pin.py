"""The oracle pinned to outputs of the reference's own Python programs (tests/golden/reference_*.npz, written by
tests/golden/make_reference_golden.py from droid_slam/geom/projective_ops.py, geom/ba.py + geom/chol.py, modules/corr.py
and droid_net.py run unchanged in float64 over the stand-ins of tests/refshim/).  CPU only.

  1  the stand-ins against yardsticks that owe them nothing: tests/se3_ref.py (pinned to scipy's expm) and finite
     differences of the reference's own projection
  2  freshness: where the checkout exists, everything is recomputed and compared with the committed files
  3  the oracle (oracle/geom.py, the C code) against the fixtures, at a quarter of the bars the device is held to
  4  the two rules of the CUDA solve that geom/chol.py does not have, carried over in numpy, and proof that each bites
  5  the restatements of the correlation volume, the feature pyramid and convex upsampling against the fixtures

Tests that need the checkout skip without it; 3 to 5 (but for the finite differences) read the fixtures alone.
Figures: profiles/reference_pin.txt.
"""
import importlib.util
import os
import sys

import numpy as np
import pytest

import cvx_upsample_ref as cu
import reference_cases as rc
import reference_programs as rp
import se3_ref
from util import STAGE_BARS, ba_args, scaled_system_errors

needs_checkout = pytest.mark.skipif(not rp.available(), reason=rp.SKIP_REASON)
U64 = 2.0 ** -53


def _shim(name):
    """a stand-in loaded under a private name: `import lietorch` stays impossible outside reference_programs.loaded()"""
    spec = importlib.util.spec_from_file_location(f"_refshim_{name}", os.path.join(rp.SHIM_DIR, name, "__init__.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


@pytest.fixture(scope="module")
def fixtures():
    return {name: rc.load(name) for name in rc.FILES}


# ---- 1: the stand-ins ------------------------------------------------------------------------------------------------
def _records(rng, n, unit=True):
    q = rng.normal(0, 1, (n, 4))
    q /= np.linalg.norm(q, axis=1, keepdims=True)
    a = np.concatenate([rng.normal(0, 2, (n, 3)), q], 1)
    return a if unit else a.astype(np.float32).astype(np.float64)     # float32 quaternions are not unit: used as they are


@pytest.mark.parametrize("unit", [True, False], ids=["unit", "float32-quaternions"])
def test_standin_group_operations_match_se3_ref(unit):
    """mul, inv, the action on homogeneous points, exp and retr against tests/se3_ref.py, in float64.  Bar: every result
    is reached in fewer than 64 roundings of terms no larger than the scale below, so 64 * 2^-53 * scale."""
    import torch
    SE3 = _shim("lietorch").SE3
    rng = np.random.default_rng(5)
    n = 64
    a, b = _records(rng, n, unit), _records(rng, n, unit)
    A, B = SE3(torch.from_numpy(a)), SE3(torch.from_numpy(b))
    xi = rng.normal(0, 1, (n, 6)) * np.repeat([1.0, 1e-3, 1e-7, 3.0], n // 4)[:, None]   # both sides of the series
    xi[0] = 0.0
    pts = rng.normal(0, 3, (n, 4))
    scale = (1 + np.abs(a).max()) * (1 + np.abs(b).max()) * (1 + np.abs(pts).max())
    bar = 64 * U64 * scale
    M = se3_ref.matrix(a)
    want_pts = np.concatenate([np.einsum("nij,nj->ni", M[:, :3, :3], pts[:, :3]) + a[:, :3] * pts[:, 3:], pts[:, 3:]], 1)
    checks = {
        "mul": ((A * B).data.numpy(), se3_ref.mul(a, b)),
        "inv": (A.inv().data.numpy(), se3_ref.inv(a)),
        "act": ((A * torch.from_numpy(pts)).numpy(), want_pts),
        "exp": (SE3.exp(torch.from_numpy(xi)).data.numpy(), se3_ref.exp(xi)),
        "retr": (A.retr(torch.from_numpy(xi)).data.numpy(), se3_ref.mul(se3_ref.exp(xi), a)),
        "broadcast": ((A[None] * B[:, None]).data.numpy(), se3_ref.mul(a[None], b[:, None])),
    }
    for what, (got, want) in checks.items():
        err = float(np.abs(got - want).max())
        print(f"stand-in {what}: {err:.2e} of a bar of {bar:.2e}")
        assert got.dtype == np.float64 and got.shape == want.shape and err <= bar, (what, err, bar)
    assert A[None, torch.tensor([3, 1])].data.shape == (1, 2, 7) and tuple(A[None].shape) == (1, n)
    assert SE3.manifold_dim == 6 and hasattr(_shim("lietorch"), "Sim3")
    a32 = SE3(torch.from_numpy(a.astype(np.float32)))
    assert (a32 * a32.inv()).data.dtype == torch.float32                 # dtype-preserving


def test_standin_scatter_matches_numpy():
    import torch
    ts = _shim("torch_scatter")
    rng = np.random.default_rng(6)
    src = rng.normal(0, 1, (2, 40, 3))
    idx = rng.integers(0, 7, 40)
    idx[idx == 4] = 5                                                    # an empty group
    want = np.zeros((2, 9, 3))
    np.add.at(want, (slice(None), idx), src)
    cnt = np.maximum(np.bincount(idx, minlength=9), 1)[None, :, None]
    got = ts.scatter_sum(torch.from_numpy(src), torch.from_numpy(idx), dim=1, dim_size=9).numpy()
    mean = ts.scatter_mean(torch.from_numpy(src), torch.from_numpy(idx), dim=1, dim_size=9).numpy()
    assert np.abs(got - want).max() <= 40 * U64 * np.abs(src).max() * 40
    assert np.abs(mean - want / cnt).max() <= 40 * U64 * np.abs(src).max() * 40
    assert not got[:, 4].any() and not got[:, 7:].any()


@needs_checkout
def test_loader_leaves_no_trace():
    before, path = set(sys.modules), list(sys.path)
    import torch
    as_tensor = torch.as_tensor
    with rp.loaded() as ref:
        assert "lietorch" in sys.modules and ref.pops.MIN_DEPTH == 0.2
        assert torch.as_tensor([0.1], device="cuda").device.type == "cpu"
    assert sys.path == path and torch.as_tensor is as_tensor
    left = {m for m in set(sys.modules) - before
            if m.split(".")[0] in ("lietorch", "torch_scatter", "geom", "modules", "droid_net", "data_readers")}
    assert not left, left
    assert importlib.util.find_spec("lietorch") is None and importlib.util.find_spec("torch_scatter") is None


@needs_checkout
def test_adjT_through_finite_differences_of_the_reference_projection():
    """Ji, Jj and Jz of pops.projective_transform against central differences of its own coords, per pose and per
    tangent component (the pose moved by retr, so exp, mul, inv, the action and adjT all enter), on the mono graph.
    Bar per entry, from the step h and the differences themselves: h |f(+h) - 2 f(0) + f(-h)| / h^2 -- the step times
    the second derivative, the error of a one-sided difference, of which the central one's is a fraction -- plus the
    rounding of the difference, 8 * 2^-53 max|f| / h."""
    import torch
    from golden import make_reference_golden as gen
    c = dict(rc.geom_cases()["mono"])
    h = 1e-6
    n = c["poses"].shape[0]
    # the formulas are the derivative for unit quaternions; float32 ones are off by 6e-8, which a difference sees
    c["poses"] = c["poses"].astype(np.float64)
    c["poses"][:, 3:] /= np.linalg.norm(c["poses"][:, 3:], axis=1, keepdims=True)
    with rp.loaded() as ref, torch.no_grad():
        base = gen.project(ref, c, jacobian=True)
        f0 = base["coords"]
        rnd = 8 * U64 * np.abs(f0).max() / h
        worst = 0.0

        def moved(k, comp, step):
            xi = torch.zeros(n, 6, dtype=torch.float64)
            xi[k, comp] = step
            poses = ref.SE3(torch.from_numpy(c["poses"])).retr(xi).data.numpy()
            return gen.project(ref, dict(c, poses=poses))["coords"]

        for k in range(n):
            for comp in range(6):
                fp, fm = moved(k, comp, h), moved(k, comp, -h)
                fd = (fp - fm) / (2 * h)
                bar = np.abs(fp - 2 * f0 + fm) / h + rnd
                want = np.zeros_like(fd)
                want[c["ii"] == k] = base["Ji"][c["ii"] == k][..., comp]
                want[c["jj"] == k] = base["Jj"][c["jj"] == k][..., comp]
                assert (np.abs(fd - want) <= bar).all(), (k, comp, float(np.abs(fd - want).max()), float(bar.max()))
                assert np.abs(want).max() > 1e3 * bar.max() or not want.any(), (k, comp)    # the bar decides something
                worst = max(worst, float((np.abs(fd - want) / np.maximum(np.abs(want), 1.0)).max()))
        # every disparity at once: a pixel of an edge depends on the disparity of its own source pixel alone
        dp = gen.project(ref, dict(c, disps=c["disps"].astype(np.float64) + h))["coords"]
        dm = gen.project(ref, dict(c, disps=c["disps"].astype(np.float64) - h))["coords"]
        fd = (dp - dm) / (2 * h)
        bar = np.abs(dp - 2 * f0 + dm) / h + rnd
        assert (np.abs(fd - base["Jz"]) <= bar).all(), float(np.abs(fd - base["Jz"]).max())
        print(f"finite differences at h = {h:g}: poses worst {worst:.2e} relative, Jz {np.abs(fd - base['Jz']).max():.2e} "
              f"absolute (bar up to {bar.max():.2e})")


# ---- 2: freshness ----------------------------------------------------------------------------------------------------
def test_fixtures_are_small_and_computed_from_these_inputs(fixtures):
    for name in rc.FILES:
        assert os.path.getsize(rc.path(name)) <= rc.MAX_BYTES, name
    for name, c in rc.geom_cases().items():
        assert str(fixtures["geom"][f"{name}_sha"]) == rc.geom_digest(c), name
    for name in rc.BA_GRAPHS:
        assert str(fixtures["ba"][f"{name}_sha"]) == rc.ba_digest(rc.ba_problem(name)), name
        # no observation with a weight is so close to the CUDA path's MIN_DEPTH that a float32 depth could decide otherwise
        assert float(fixtures["ba"][f"{name}_rule"][1]) > 1e-4, name
    for name in rc.FULL_BLOCKS:
        assert str(fixtures["ba_blocks"][f"{name}_sha"]) == rc.ba_digest(rc.ba_problem(name)), name
    assert str(fixtures["corr"]["sha"]) == rc.digest(rc.corr_fmaps(), *rc.CORR_EDGES)
    for case, sigma in rc.up_cases():
        p = cu.problem(case, sigma)
        assert str(fixtures["upsample"][f"sha_{rc.up_key(case, sigma)}"]) == rc.digest(p["data"], p["mask16"])


@needs_checkout
def test_fixtures_are_fresh(fixtures):
    """Recomputed in memory, the reference's programs give the committed arrays to 1e-12 of each array's largest entry
    (the summation order of the BLAS is the only thing that may differ between two machines)."""
    from golden import make_reference_golden as gen
    fresh = gen.compute_all()
    assert set(fresh) == set(rc.FILES)
    worst = 0.0
    for name in rc.FILES:
        assert set(fresh[name]) == set(fixtures[name]), name
        for k, want in fixtures[name].items():
            got = np.asarray(fresh[name][k])
            assert got.shape == want.shape and got.dtype == want.dtype, (name, k)
            if want.dtype.kind in "US":
                assert str(got) == str(want), (name, k)
                continue
            if want.dtype.kind in "ui":
                assert np.array_equal(got, want), (name, k)
                continue
            err = float(np.abs(got - want).max()) / max(float(np.abs(want).max()), 1e-300)
            worst = max(worst, err)
            assert err <= 1e-12, (name, k, err)
    print(f"fixtures against a fresh run of the reference: worst {worst:.2e}")


# ---- 3: the oracle against the fixtures ----------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(rc.geom_cases()))
def test_oracle_projection_matches_the_reference(oracle, fixtures, name):
    """oracle/geom.py: coords within a quarter of the 64 units of 2^-24 * coord_scale the device is held to
    (tests/test_gpu_geom.py), valid identical, and Z -- what the MIN_DEPTH rule decides on -- to the same quarter of its
    band.  Where one set of intrinsics and no stereo edge allow it, the C oracle's projmap too."""
    from oracle import geom as G
    c, g = rc.geom_cases()[name], fixtures["geom"]
    poses = rc.unit_poses(c["poses"])
    coords, valid, m = G.reproject(poses, c["disps"], c["K"], c["ii"], c["jj"], margins=True)
    fx, fy, cx, cy = (m["Kj"][..., k] for k in range(4))
    scale = np.stack([G.coord_scale(fx, cx, m["X"][..., 0], m["Zc"], m["mag"]),
                      G.coord_scale(fy, cy, m["X"][..., 1], m["Zc"], m["mag"])], -1)
    units = float((np.abs(coords - g[f"{name}_coords"]) / (G.EPS32 * scale)).max())
    zunits = float((np.abs(m["Z"] - g[f"{name}_Z"]) / (G.EPS32 * m["mag"])).max())
    behind = int((g[f"{name}_Z"] < G.MIN_DEPTH).sum())
    print(f"[{name}] oracle.geom.reproject vs reference: coords {units:.2e} units, Z {zunits:.2e} units (bar "
          f"{G.Z_BAND_C / 4}), valid differs at {int((valid[..., 0] != g[f'{name}_valid']).sum())}, behind MIN_DEPTH {behind}")
    assert units <= G.Z_BAND_C / 4 and zunits <= G.Z_BAND_C / 4
    assert np.array_equal(valid[..., 0], g[f"{name}_valid"].astype(np.float64))
    if name == "hard":
        assert behind > 0.05 * g["hard_Z"].size and (g["hard_Z"] < 0.5 * G.MIN_DEPTH).any()   # both rules decide
    if name == "stereo":
        st = c["ii"] == c["jj"]
        assert st.sum() == 4 and np.abs(coords[st] - g["stereo_coords"][st]).max() < 1e-9      # the fixed baseline
    if c["K"].ndim == 1 and (c["ii"] != c["jj"]).all():
        pc, pv = oracle.projmap(poses, c["disps"], c["K"], c["ii"], c["jj"])
        Z = g[f"{name}_Z"]
        same = Z > 0.5 * G.MIN_DEPTH            # below it the Python program projects with depth 1, the kernel does not
        pu = float((np.abs(pc[..., :2] - g[f"{name}_coords"]) / (G.EPS32 * scale))[same].max())
        print(f"[{name}] C oracle projmap vs reference: coords {pu:.2e} units where Z > {0.5 * G.MIN_DEPTH}")
        assert pu <= G.Z_BAND_C / 4
        clear = np.abs(Z - G.KERNEL_MIN_DEPTH) > G.z_band(m["mag"])
        assert np.array_equal(pv[..., 0][clear], (Z > G.KERNEL_MIN_DEPTH)[clear].astype(np.float64))


def test_oracle_jacobians_match_the_reference(oracle, fixtures):
    """Ji, Jj, Jz of pops.projective_transform at the (edge, pixel) samples the fixture keeps, against the C oracle's
    linearisation.  The oracle only returns sums, so each row is read back from one call with the weight on that row
    alone and a target of 0: bz = w r Jz, Eii = w Jz Ji, Eij = w Jz Jj with w = .001 and r = -coords.  Bar: the
    quantities are reached in well under 1024 roundings: 1024 * 2^-53 of the largest entry of the row."""
    c, g = rc.geom_cases()["mono"], fixtures["geom"]
    E, H, W = g["mono_Z"].shape
    HW = H * W
    poses = rc.unit_poses(c["poses"])
    zero = np.zeros((2, H, W))
    worst, seen = 0.0, 0
    for flat, Ji, Jj, Jz in zip(rc.jac_sample("mono", E, HW), g["mono_Ji"], g["mono_Jj"], g["mono_Jz"]):
        e, k = divmod(int(flat), HW)
        for row in range(2):
            wt = zero.copy()
            wt[row] = 1.0
            lin = oracle.linearize_edge(zero, wt, poses, c["disps"], c["K"], int(c["ii"][e]), int(c["jj"][e]))
            r = -g["mono_coords"][e].reshape(HW, 2)[k, row]
            jz = lin["bz"][k] / (.001 * r)
            got = np.concatenate([lin["Eii"][:, k] / (.001 * jz), lin["Eij"][:, k] / (.001 * jz), [jz]])
            want = np.concatenate([Ji[row], Jj[row], [Jz[row]]])
            assert abs(want[-1]) > 1e-3 and abs(r) > 1e-3, (e, k, row)          # the read-back is well conditioned
            err = float(np.abs(got - want).max() / np.abs(want).max())
            worst, seen = max(worst, err), seen + 1
            assert err <= 1024 * U64, (e, k, row, err)
    print(f"oracle Jacobians vs reference at {seen} rows: worst {worst:.2e} relative (bar {1024 * U64:.2e})")


def _quarter(family):
    return {k: 0.25 * v for k, v in STAGE_BARS[family].items()}


@pytest.mark.parametrize("name", list(rc.BA_GRAPHS))
def test_oracle_system_matches_the_reference(oracle, fixtures, name):
    """The oracle's fp64 reduced system (motion-only: H, v) against the reference's own undamped S, b in
    util.scaled_system_errors, and its per-edge blocks against the reference's where the fixture keeps them (each edge's
    [[Hii Hij] [Hji Hjj]], (vi vj) as a system of two poses in the same metric).  Condition, not tuned: a quarter of
    the family's STAGE_BARS, no stray block, no dead row.  Both sides see the quaternions normalised in float64
    (reference_cases.unit_poses); what the float32 ones add is printed next to it."""
    _, family, motion_only, _ = rc.BA_GRAPHS[name]
    p, g = rc.ba_problem(name), fixtures["ba"]
    n = 6 * (p.t1 - p.t0)
    o = oracle.ba(*ba_args(rc.on_the_sphere(p)), 1, p.lm, p.ep, motion_only, debug=True)
    S = rc.tril_unpack(g[f"{name}_S"], n)
    err = scaled_system_errors(o["H"], o["b"], S, g[f"{name}_b"])
    bar = _quarter(family)
    raw = oracle.ba(*ba_args(p), 1, p.lm, p.ep, motion_only, debug=True)          # the float32 quaternions as they are
    eraw = scaled_system_errors(raw["H"], raw["b"], S, g[f"{name}_b"])
    f32 = oracle.ba(*ba_args(p), 1, p.lm, p.ep, motion_only, debug=True, precision="f32")
    e32 = scaled_system_errors(f32["H"], f32["b"], S, g[f"{name}_b"])
    line = (f"[{name}] oracle fp64 vs reference: H {err['H']:.2e} b {err['b']:.2e} stray {err['stray']} dead {err['dead']}"
            f" | from float32 quaternions: H {eraw['H']:.2e} b {eraw['b']:.2e}"
            f" | oracle fp32 vs reference: H {e32['H']:.2e} b {e32['b']:.2e} | bars H {bar['H']:.2e} b {bar['b']:.2e}")
    if name in rc.EDGE_BLOCKS:
        eh = ev = 0.0
        for e in range(len(p.ii)):
            R, O = g[f"{name}_Hs"][e], o["Hs"][e]
            full = lambda B: np.block([[B[0], B[1]], [B[2], B[3]]])
            ee = scaled_system_errors(full(O), o["vs"][e].reshape(-1), full(R), g[f"{name}_vs"][e].reshape(-1))
            assert ee["dead"] == 0, (name, e)
            eh, ev = max(eh, ee["H"]), max(ev, ee["b"])
        line += f" | per-edge blocks: Hs {eh:.2e} vs {ev:.2e}"
        assert eh <= bar["H"] and ev <= bar["b"], (name, eh, ev)
    print(line)
    assert err["stray"] == 0 and err["dead"] == 0, err
    assert err["H"] <= bar["H"] and err["b"] <= bar["b"], (name, err, bar)


# ---- 4: the two rules of the CUDA solve ------------------------------------------------------------------------------
def rules_bars(blk, name, p, family, dx, A):
    """dx: two backward-stable fp64 solves of one matrix, 8 n 2^-53 cond_2(A) of the largest component.
    dz = Q (w - E^T dx): that error of dx through |Q| |E^T|, plus the distance of the oracle's own Q, w, E from the
    reference's, for which the quarter bar of test 3 stands (entry-wise, relative)."""
    E, C, w = (blk[f"{name}_{k}"] for k in ("E", "C", "w"))
    n = A.shape[0]
    cond = float(np.linalg.cond(A))
    bar_dx = 8 * n * U64 * cond * float(np.abs(dx).max())
    Q = 1.0 / C
    bar_dz = float((Q * (np.abs(E).T @ np.full(n, bar_dx))).max()) \
        + 0.25 * STAGE_BARS[family]["b"] * float((Q * (np.abs(w) + np.abs(E).T @ np.abs(dx))).max())
    return bar_dx, bar_dz, cond


@pytest.mark.parametrize("name", rc.FULL_BLOCKS)
def test_oracle_solve_follows_the_two_cuda_rules(oracle, fixtures, name):
    """The oracle's solve and back-substitution (oracle.BAPhases.finish) of the REFERENCE's reduced system follow the
    reference's H, E, C, v, w with the two CUDA rules applied in numpy; with either rule left out the same comparison
    fails by at least 100 bars, so the fixture tells the two programs apart."""
    _, family, _, _ = rc.BA_GRAPHS[name]
    p, blk, g = rc.ba_problem(name), fixtures["ba_blocks"], fixtures["ba"]
    n = 6 * (p.t1 - p.t0)
    dx, dz, A = rc.cuda_rules(blk, name, p)
    bar_dx, bar_dz, cond = rules_bars(blk, name, p, family, dx, A)
    ph = oracle.BAPhases()
    ph.build(*ba_args(rc.on_the_sphere(p)), 0, p.disps.shape[0], False)
    lm, ep = float(np.float32(p.lm)), float(np.float32(p.ep))
    _, disps, odx = ph.finish(rc.tril_unpack(g[f"{name}_S"], n), g[f"{name}_b"], lm, ep)
    kx = np.unique(p.ii)
    odz = (disps[kx] - p.disps[kx].astype(np.float64)).reshape(-1)
    own = oracle.ba(*ba_args(rc.on_the_sphere(p)), 1, p.lm, p.ep, False)          # its own system: for the record
    ex, ez = float(np.abs(odx.reshape(-1) - dx).max()), float(np.abs(odz - dz).max())
    print(f"[{name}] cond_2 of the damped S {cond:.2e}; oracle vs reference + CUDA rules: dx {ex:.2e} (bar {bar_dx:.2e}), "
          f"dz {ez:.2e} (bar {bar_dz:.2e}); from the oracle's own system: dx {np.abs(own['dx'].reshape(-1) - dx).max():.2e} "
          f"dz {np.abs(own['dz'].reshape(-1) - dz).max():.2e}; max|dx| {np.abs(dx).max():.2e} max|dz| {np.abs(dz).max():.2e}")
    assert ex <= bar_dx and ez <= bar_dz, (ex, bar_dx, ez, bar_dz)
    dx1, dz1, _ = rc.cuda_rules(blk, name, p, damp_schur=False)             # geom/chol.py:56
    dx2, dz2, _ = rc.cuda_rules(blk, name, p, drop_first=False)             # geom/chol.py:69
    ex1, ez1 = float(np.abs(odx.reshape(-1) - dx1).max()), float(np.abs(odz - dz1).max())
    ez2 = float(np.abs(odz - dz2).max())
    print(f"[{name}] damping before the Schur complement instead: dx {ex1 / bar_dx:.1e} bars, dz {ez1 / bar_dz:.1e} bars; "
          f"first window pose kept in the back-substitution: dz {ez2:.2e} = {ez2 / bar_dz:.1e} bars")
    assert ex1 >= 100 * bar_dx and ez2 >= 100 * bar_dz, (ex1, bar_dx, ez2, bar_dz)
    assert np.array_equal(dx2, dx)                                       # the second rule touches dz alone


# ---- 5: correlation and upsampling -----------------------------------------------------------------------------------
def test_corr_volume_restatement_matches_the_reference(fixtures):
    """tests/corr_volume_ref.py against CorrBlock: level 0 inside the interval of the module's own rule with the unit
    roundoff of float64 (the reference ran in float64), levels 1-3 = pool of the level before, whose float32 rounding
    (four inputs, three sums) bounds the distance: 4 * 2^-24 * mean |v|."""
    import corr_volume_ref as cv
    g, s = fixtures["corr"], rc.CORR_SHAPE
    ii, jj = rc.CORR_EDGES
    rows = rc.corr_rows()
    a, b = cv.operands(rc.corr_fmaps(), ii, jj, np.float32)              # half values / 4: exact in float32
    x = cv.level0_exact(a, b)[:, rows]
    beta = (s["C"] + 2) * U64 * cv.abs_products(a, b)[:, rows]
    l0 = g["volume_l0"].reshape(x.shape)
    print(f"all-pairs volume vs CorrBlock.corr: max {np.abs(l0 - x).max():.2e}, bar up to {beta.max():.2e}")
    assert (np.abs(l0 - x) <= beta).all() and np.abs(x).max() > 1.0
    for l in range(s["levels"] - 1):
        lvl = g[f"volume_l{l}"]
        want = g[f"volume_l{l + 1}"]
        got = cv.pool(lvl.astype(np.float32), np.float32)
        assert got.shape == want.shape == (2, len(rows), s["h"] >> (l + 1), s["w"] >> (l + 1))
        mean_abs = cv.pool(np.abs(lvl).astype(np.float32), np.float32).astype(np.float64)
        assert (np.abs(got - want) <= 4 * 2.0 ** -24 * mean_abs * (1 + 2.0 ** -20)).all(), l


def test_alt_pyramid_restatement_matches_the_reference(fixtures):
    """callers.FmapLookup's pyramid against AltCorrBlock.__init__'s, float64: the same sums of exactly representable
    values, so equal to the last bit."""
    import torch
    from callers import FmapLookup
    f = torch.from_numpy(rc.corr_fmaps().astype(np.float64))
    pyr = FmapLookup(f[None], levels=rc.CORR_SHAPE["levels"]).pyramid
    for l, lvl in enumerate(pyr):
        want = fixtures["corr"][f"alt_l{l}"]
        got = lvl[0][torch.from_numpy(rc.ALT_FRAMES)].numpy()
        assert got.shape == want.shape and np.array_equal(got, want), l
    assert np.array_equal(fixtures["corr"]["alt_l0"], rc.corr_fmaps()[rc.ALT_FRAMES].astype(np.float64).transpose(0, 2, 3, 1) / 4)


@pytest.mark.parametrize("case,sigma", rc.up_cases())
def test_cvx_upsample_restatement_matches_the_reference(fixtures, case, sigma):
    """tests/cvx_upsample_ref.ref in float64 against droid_net.upsample_disp (and cvx_upsample itself where kept), at
    the pixels the fixture keeps: the module's bar with the unit roundoff of float64, 32 * 2^-53 * nb, which is far
    inside its BAR."""
    p, g = cu.problem(case, sigma), fixtures["upsample"]
    key, s = rc.up_key(case, sigma), rc.up_sample(case, sigma)
    want = g[f"disp_{key}"]
    got, nb = p["ref64"].reshape(-1)[s], p["nb"].reshape(-1)[s]
    err = float((np.abs(got - want) / nb).max())
    assert want.shape == got.shape and err <= 32 * U64 <= cu.BAR, (case, sigma, err)
    if f"cvx_{key}" in g:
        assert np.array_equal(g[f"cvx_{key}"], want)
