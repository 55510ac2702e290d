"""The HIP kernels against outputs of the reference's own Python programs, with no oracle in between: the fixtures
tests/golden/reference_*.npz (tests/golden/make_reference_golden.py; inputs rebuilt by tests/reference_cases.py and
checked against the recorded SHA-256 by tests/test_reference_pin.py).  Reads tests/golden/ alone.  The bars are those
the same quantities are held to against the oracle elsewhere in the suite; the oracle appears only where those bars are
defined through it (the scale and the band of a depth decision, the float32 variant's own error for projmap).

The reference ran on the float32 inputs widened to float64 with the quaternions normalised there
(reference_cases.unit_poses); the device reads the float32 records, so what it is compared with differs from its own
inputs by that normalisation: up to 5e-9 in H and 8e-8 in b of the scaled metric, inside every bar below.
Figures: profiles/reference_pin.txt.
"""
import numpy as np
import pytest

import corr_volume_ref as cv
import cvx_upsample_ref as cu
import geom_cases as gc
import reference_cases as rc
import se3_ref
import stage_graphs as sg
from oracle import geom as G
from util import (STAGE_BARS, assert_system_close, quat_angle, run_ba_stages, run_hip_ba, scaled_system_errors,
                  slot_classes)

pytestmark = pytest.mark.gpu
DT = {np.float16: "float16", np.float32: "float32"}


def _torch():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    return torch


def _dev(a):
    return _torch().from_numpy(np.ascontiguousarray(a)).cuda()


@pytest.fixture(scope="module")
def fixtures():
    return {name: rc.load(name) for name in rc.FILES}


def _units(got, ref, scale, where):
    with np.errstate(divide="ignore", invalid="ignore"):
        return float(np.nanmax((np.abs(got.astype(np.float64) - ref) / (G.EPS32 * scale))[where])) if where.any() else 0.0


# ---- projection ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(rc.geom_cases()))
def test_reproject_and_projmap_match_the_reference(backends, oracle, fixtures, name):
    """droid_backends.reproject against pops.projective_transform's coords and valid, with the bars of
    tests/test_gpu_geom.py::test_reproject_cases: valid identical outside the band of the two depth thresholds,
    coordinates within 64 units of 2^-24 * coord_scale.  projmap (one set of intrinsics, no stereo rule, MIN_DEPTH
    0.25, no depth-1 substitution: the CUDA kernel's rules) where the case allows it: valid is `Z > 0.25` of the
    reference's depth outside the band, coordinates where the Python program does not substitute (Z > 0.1), within
    4 x the float32 C oracle's own distance from the reference (test_projmap_cases)."""
    c, g = rc.geom_cases()[name], fixtures["geom"]
    rcoords, rvalid, Z = g[f"{name}_coords"], g[f"{name}_valid"].astype(np.float32), g[f"{name}_Z"]
    args = (_dev(c["poses"]), _dev(c["disps"]), _dev(c["K"]), _dev(c["ii"]), _dev(c["jj"]))
    co, va = (a.cpu().numpy()[0] for a in backends.reproject(*args))
    _, _, r = G.reproject(c["poses"], c["disps"], c["K"], c["ii"], c["jj"], margins=True)
    band = gc.in_z_band(r["Z"], r["mag"], gc.Z_REPROJECT)
    fx, fy, cx, cy = (r["Kj"][..., k] for k in range(4))
    scale = np.stack([G.coord_scale(fx, cx, r["X"][..., 0], r["Zc"], r["mag"]),
                      G.coord_scale(fy, cy, r["X"][..., 1], r["Zc"], r["mag"])], -1)
    e = _units(co, rcoords, scale, np.broadcast_to(~band[..., None], scale.shape))
    print(f"[{name}] reproject vs reference: {e:.2f} units of a bar of {G.Z_BAND_C}, band {int(band.sum())}, "
          f"invalid {int((rvalid == 0).sum())}")
    assert band.sum() <= gc.cap(band.size)
    assert np.array_equal(va[..., 0][~band], rvalid[~band])
    assert e <= G.Z_BAND_C, e
    if c["K"].ndim != 1 or (c["ii"] == c["jj"]).any():
        return
    pc, pv = (a.cpu().numpy() for a in backends.projmap(*args))
    _, _, m = G.projmap(c["poses"], c["disps"], c["K"], c["ii"], c["jj"], margins=True)
    band = gc.in_z_band(m["Z"], m["mag"], gc.Z_PROJMAP) | gc.in_z_band(m["Z"], m["mag"], (0.5 * G.MIN_DEPTH,))
    K = c["K"].astype(np.float64)
    pscale = np.stack([G.coord_scale(K[0], K[2], m["X"][..., 0], m["Z"], m["mag"]),
                       G.coord_scale(K[1], K[3], m["X"][..., 1], m["Z"], m["mag"])], -1)
    sel = np.broadcast_to(((Z > 0.5 * G.MIN_DEPTH) & ~band)[..., None], pscale.shape)
    c32, _ = oracle.projmap(c["poses"], c["disps"], c["K"], c["ii"], c["jj"], precision="f32")
    e32, e = _units(c32[..., :2], rcoords, pscale, sel), _units(pc[..., :2], rcoords, pscale, sel)
    allow = min(4 * max(e32, 1.0), float(G.Z_BAND_C))
    print(f"[{name}] projmap vs reference: float32 oracle {e32:.2f} units, kernel {e:.2f}, bar {allow:.2f}")
    assert np.array_equal(pv[..., 0][~band], (Z > G.KERNEL_MIN_DEPTH)[~band].astype(np.float32))
    assert e <= allow, (e, e32)


# ---- bundle adjustment -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(rc.BA_GRAPHS))
def test_ba_system_matches_the_reference(backends, fixtures, name):
    """The system droid_ba_build writes against the reduced system geom/ba.py + geom/chol.py formed themselves (undamped
    S, b; motion-only: H, v), in util.scaled_system_errors at the family's STAGE_BARS, no stray block, no dead row, and
    the Schur classes of stage_graphs.GRAPHS where the graph is in that table."""
    torch = _torch()
    _, family, motion_only, table = rc.BA_GRAPHS[name]
    p, g = rc.ba_problem(name), fixtures["ba"]
    n = 6 * (p.t1 - p.t0)
    st = run_ba_stages(backends, p, torch, motion_only=motion_only)
    got = slot_classes(st, motion_only)
    err = scaled_system_errors(st["system"][:n], st["system"][n], rc.tril_unpack(g[f"{name}_S"], n), g[f"{name}_b"])
    bar = STAGE_BARS[family]
    print(f"[{name}] device vs reference: H {err['H']:.2e} / {bar['H']:.2e}  b {err['b']:.2e} / {bar['b']:.2e}  "
          f"stray {err['stray']} dead {err['dead']} classes {sorted(got, key=str)} "
          f"behind MIN_DEPTH with a weight: {int(g[f'{name}_rule'][0])}")
    assert st["status"] & 15 == 0, st["status"]
    if table is not None:
        assert got == sg.GRAPHS[table][2], (name, got)
    if not motion_only:
        assert st["M"] == p.eta.shape[0]
    assert_system_close(err, bar, name)


@pytest.mark.parametrize("name", rc.FULL_BLOCKS)
def test_public_ba_matches_the_reference_with_the_cuda_rules(backends, fixtures, name):
    """One iteration of droid_backends.ba against: the reference's H, E, C, v, w, solved the way the CUDA path does
    (reference_cases.cuda_rules: damping on the Schur diagonal, the first window pose left out of the
    back-substitution), retracted by tests/se3_ref.py.  Bar: STAGE_BARS[family]["state"]."""
    import copy
    torch = _torch()
    _, family, _, _ = rc.BA_GRAPHS[name]
    p = rc.ba_problem(name)
    dx, dz, _ = rc.cuda_rules(fixtures["ba_blocks"], name, p)
    poses, disps = p.poses.astype(np.float64), p.disps.astype(np.float64)
    poses[p.t0:p.t1] = se3_ref.mul(se3_ref.exp(dx.reshape(-1, 6)), poses[p.t0:p.t1])
    kx = np.unique(p.ii)
    disps[kx] += dz.reshape(len(kx), *disps.shape[1:])
    hip = run_hip_ba(backends, copy.deepcopy(p), torch, 1)
    assert hip["status"] & 15 == 0 and hip["M"] == len(kx)
    et = float(np.abs(hip["poses"][:, :3] - poses[:, :3]).max())
    er = float(quat_angle(hip["poses"][:, 3:].astype(np.float64), poses[:, 3:]).max())
    ed = float(np.abs(hip["disps"] - disps).max())
    edx = float(np.abs(hip["dx"].reshape(-1) - dx).max())
    bar = STAGE_BARS[family]["state"]
    print(f"[{name}] droid_backends.ba vs reference + CUDA rules: t {et:.2e} q {er:.2e} d {ed:.2e} (bar {bar:.2e}), "
          f"dx {edx:.2e} of {np.abs(dx).max():.2e}")
    assert max(et, er, ed) < bar, (et, er, ed)
    assert np.array_equal(hip["poses"][:p.t0], p.poses[:p.t0])


# ---- correlation -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("npdt", [np.float16, np.float32])
def test_corr_volume_pyramid_matches_the_reference(backends, fixtures, npdt):
    """corr_volume_pyramid against CorrBlock's pyramid at the source pixels the fixture keeps.  Level 0: the rule of
    tests/test_gpu_corr_volume.py, T(x - beta) <= dev <= T(x + beta), beta = (C + 2) 2^-24 sum |a||b|, with x the
    reference's value.  Levels 1-3: the reference averages in float64 what the device averages from its own rounded
    level, so the distance is bounded by the mean of the level below's bound plus the roundings of one pooling step
    (three float32 sums, one rounding to T): bound' = mean4(bound) + (4 * 2^-24 + u_T) mean4(|ref| + bound)."""
    torch = _torch()
    g, s = fixtures["corr"], rc.CORR_SHAPE
    ii, jj = rc.CORR_EDGES
    rows = rc.corr_rows()
    fmaps = rc.corr_fmaps().astype(npdt)
    pyr = backends.corr_volume_pyramid(_dev(fmaps), _dev(ii), _dev(jj), s["levels"])
    torch.cuda.synchronize()
    full = [lvl.cpu().numpy() for lvl in pyr]
    dev = [lvl.reshape(2, s["h"] * s["w"], s["h"] >> l, s["w"] >> l)[:, rows] for l, lvl in enumerate(full)]
    a, b = cv.operands(fmaps, ii, jj, npdt)
    x = g["volume_l0"]
    beta = ((s["C"] + 2) * 2.0 ** -24 * cv.abs_products(a, b))[:, rows].reshape(x.shape)
    with np.errstate(over="ignore"):
        lo, hi = (x - beta).astype(npdt), (x + beta).astype(npdt)
    assert np.isfinite(dev[0]).all() and np.all(lo <= dev[0]) and np.all(dev[0] <= hi)
    uT = 2.0 ** -11 if npdt is np.float16 else 2.0 ** -24
    mean4 = lambda v: 0.25 * (v[..., 0::2, 0::2] + v[..., 0::2, 1::2] + v[..., 1::2, 0::2] + v[..., 1::2, 1::2])
    bound = beta + uT * np.abs(x)
    print(f"{DT[npdt]} level 0 vs CorrBlock: max {np.abs(dev[0] - x).max():.2e}, bound up to {bound.max():.2e}")
    for l in range(1, s["levels"]):
        ref_below = g[f"volume_l{l - 1}"]
        H2, W2 = 2 * (ref_below.shape[-2] // 2), 2 * (ref_below.shape[-1] // 2)
        bound = mean4(bound[..., :H2, :W2]) + (4 * 2.0 ** -24 + uT) * mean4((np.abs(ref_below) + bound)[..., :H2, :W2])
        want = g[f"volume_l{l}"]
        d = np.abs(dev[l].astype(np.float64) - want)
        print(f"{DT[npdt]} level {l} vs CorrBlock: max {d.max():.2e}, bound up to {bound.max():.2e}")
        assert dev[l].shape == want.shape and (d <= bound).all(), l
        assert np.array_equal(cv.pool(full[l - 1], npdt).view(np.uint8), full[l].view(np.uint8))   # the suite's own rule


# ---- convex upsampling -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case,sigma", rc.up_cases())
def test_cvx_upsample_matches_the_reference(backends, fixtures, case, sigma):
    """cvx_upsample (half mask) and upsample_disps (float32 mask, frames scattered in a larger buffer) against
    droid_net.upsample_disp at the output pixels the fixture keeps: cvx_upsample_ref.BAR * nb."""
    torch = _torch()
    p, g = cu.problem(case, sigma), fixtures["upsample"]
    key, s = rc.up_key(case, sigma), rc.up_sample(case, sigma)
    want, nb = g[f"disp_{key}"], p["nb"].reshape(-1)[s]
    n, H, W = p["data"].shape
    got = backends.cvx_upsample(_dev(p["data"])[..., None], _dev(p["mask16"]))
    assert tuple(got.shape) == (n, 8 * H, 8 * W, 1)
    e16 = float((np.abs(got.cpu().numpy().reshape(-1)[s].astype(np.float64) - want) / nb).max())
    ix = np.arange(n)[::-1] * 2 + 1                                  # frames 2n-1, ..., 3, 1 of a buffer of 2n + 1
    disps = np.zeros((2 * n + 1, H, W), np.float32)
    disps[ix] = p["data"]
    out = torch.full((2 * n + 1, 8 * H, 8 * W), -1.0, dtype=torch.float32, device="cuda")
    backends.upsample_disps(_dev(disps), _dev(ix.astype(np.int64)), _dev(p["mask32"]), out)
    out = out.cpu().numpy()
    e32 = float((np.abs(out[ix].reshape(-1)[s].astype(np.float64) - want) / nb).max())
    print(f"{cu.CASES[case]} sigma {sigma}: cvx_upsample {e16 / cu.U:.2f} u nb, upsample_disps {e32 / cu.U:.2f} u nb, "
          f"bar {cu.BAR / cu.U:.0f}")
    assert e16 <= cu.BAR and e32 <= cu.BAR, (e16 / cu.U, e32 / cu.U)
    assert (out[::2] == -1.0).all()
