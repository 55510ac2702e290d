"""The BA path around the Cholesky solve, on the device.

* A failed factorisation (lm = 0, ep = -1e6, the device of tests/test_oracle_ba.py) must do what the reference does
  (droid_kernels.cu:1202-1210): status bit 2 and nothing else, dx = 0 exactly, poses untouched, the depth update carried
  out with dx = 0, no NaN anywhere although the factor and x are full of them, and the next ordinary call unaffected.
* The damping diag += ep + lm*diag inside the factor kernel, on its own: a known matrix is written over the system that
  droid_ba_build left in the workspace (motion-only problem with P window frames, so 6P + 1 crosses the 16-double pitch
  and the 64-column tile boundaries) and droid_ba_solve_update's dx is held to float32 of the longdouble solve of the
  damped matrix."""

import numpy as np
import pytest

import chol_cases as C
import chol_ref as R
from util import STAGE_BARS, ba_args, compare_state, run_hip_ba, to_dev

pytestmark = pytest.mark.gpu
TOL = 1e-4      # the usual parity of a `ba` call (tests/test_gpu_ba.py)
CORNER = 3.0


def _torch():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    return torch


@pytest.fixture(scope="module")
def synth():
    from droid_backends import synth
    return synth


def _graph(synth, name):
    import stage_graphs
    if name == "tiny":
        return synth.make_ba_problem(N=3, E=4, H=16, W=24, seed=11), "sparse", False
    if name == "cfg2":
        return synth.make_config("cfg2"), "sparse", False
    return stage_graphs.motion_only(synth), "motion", True


@pytest.mark.parametrize("name", ["tiny", "cfg2", "motion_only"])
def test_failed_factorisation_on_the_device(backends, oracle, synth, name):
    """tiny: per-step kernels (n = 12); cfg2: the single-launch factorisation (n = 378); and a motion-only call."""
    torch = _torch()
    p, family, mo = _graph(synth, name)
    d = to_dev(p, torch)
    dx, dz = backends.ba(d["poses"], d["disps"], d["intrinsics"], d["disps_sens"], d["targets"], d["weights"], d["eta"],
                         d["ii"], d["jj"], p.t0, p.t1, 1, 0.0, -1e6, mo)
    torch.cuda.synchronize()
    st, _ = backends.ba_status()
    assert st & 4, st
    assert st & 11 == 0, st
    dx, dz = dx.cpu().numpy(), dz.cpu().numpy()
    poses, disps = d["poses"].cpu().numpy(), d["disps"].cpu().numpy()
    assert dx.shape == (p.t1 - p.t0, 6) and not np.any(dx), np.abs(dx).max()
    assert np.array_equal(poses.view(np.uint32), np.asarray(p.poses, np.float32).view(np.uint32))
    for arr, what in ((poses, "poses"), (disps, "disps"), (dx, "dx"), (dz, "dz")):
        assert np.all(np.isfinite(arr)), what
    ref = oracle.ba(*ba_args(p), 1, 0.0, -1e6, mo, storage_f32=True)
    assert not np.any(ref["dx"])
    ed = float(np.abs(disps - ref["disps"]).max())
    print(f"[{name}] failed factorisation: status {st}, max |ddisp| vs oracle {ed:.3e} (bar {STAGE_BARS[family]['state']:.1e})")
    assert ed < STAGE_BARS[family]["state"], ed
    if not mo:
        assert np.abs(disps - p.disps).max() > 0       # the depth update did take place
    # the next ordinary call: does not raise (bit 2 is the reference's behaviour, not a violation), usual parity
    hip = run_hip_ba(backends, p, torch, 2, mo)
    good = oracle.ba(*ba_args(p), 2, p.lm, p.ep, mo, storage_f32=True)
    assert hip["status"] & 15 == 0, hip["status"]
    et, er, e2 = compare_state(hip, good, f"{name} after the failure")
    assert et < TOL and er < TOL and e2 < TOL, (et, er, e2)


def _motion_problem(synth, P):
    """Frame 0 fixed, P window frames each observed from it."""
    return synth.make_ba_problem(N=P + 1, H=8, W=16, seed=100 + P, edges=([0] * P, list(range(1, P + 1))))


@pytest.mark.parametrize("P", [7, 11, 63, 64, 107])
def test_damped_solve_of_an_injected_system(backends, synth, P):
    """n = 6P in {42, 66, 378, 384, 642}: below one tile, just past it, cfg2's size, a multiple of 64 (the rhs row is a
    block row of its own) and one row past ten tiles.  dx must equal float32(solve_ld(A + diag(ep + lm diag A), b)) to one
    float32 rounding per component plus the fp64 forward-error bar of tests/test_gpu_chol_accuracy.py on the damped
    system.  A padding that got damped cannot change dx (nothing reads it); a right-hand side or a diagonal entry that got
    damped wrongly does, by an amount that follows (lm, ep) and vanishes at (0, 0): the undamped call tells the two
    apart, and the padding is looked at directly."""
    torch = _torch()
    from droid_backends.ba_binding import BAProblemDev, BaBinding
    p = _motion_problem(synth, P)
    d = BAProblemDev(**to_dev(p, torch))
    nbuf, n = p.disps.shape[0], 6 * P
    bd = BaBinding(status_mirror=False, headroom=(1, 0))
    bd.begin(d, p.t0, p.t1, True)
    bd.buf.zero_()
    ld = (n + 1 + 15) // 16 * 16
    assert bd.system().numel() == (n + 1) * ld
    sysv = bd.system().view(n + 1, ld)
    rng = np.random.default_rng(P)
    A = 1e4 * C.spectrum_matrix(rng, n, np.logspace(0, -6, n))          # diagonal ~ 1e3, kappa 1e6 undamped
    b = rng.normal(size=n)
    b *= 1e-3 / np.abs(np.linalg.solve(C.damp(A, 1e-4, 0.1), b)).max()  # |dx| ~ 1e-3: a retraction like any other
    host = np.zeros((n + 1, ld))
    host[:n, :n] = np.tril(A)
    host[n, :n] = b
    host[n, n] = CORNER      # the rhs row's own "diagonal" entry: a damping loop one row too long would change it
    poses0 = d.poses.clone()
    failures = []
    corner0 = None
    for lm, ep in ((0.0, 0.0), (1e-4, 0.1), (1e-2, 1e-6)):
        d.poses.copy_(poses0)
        bd.prepare(d, (0, nbuf), True)
        bd.build(d, True)
        sysv.copy_(torch.from_numpy(host))
        dx = torch.full((P, 6), float("nan"), dtype=torch.float32, device="cuda")
        bd.solve_update(d, lm, ep, True, dx, None)
        torch.cuda.synchronize()
        st, m = bd.status()
        assert st == 0, st
        Ad = C.damp(A, lm, ep)
        xref, errs = R.cpu_yardstick(Ad, b)
        bar_f = R.bars(errs, (C.SPREAD_FWD, C.SPREAD_OMEGA))[0]
        got = dx.cpu().numpy().reshape(-1).astype(R.LD)
        fp = bar_f * np.abs(xref).max()                      # the fp64 solve, then one float32 rounding of ITS value
        tol = 2.0 ** -24 * (np.abs(xref) + fp) + fp
        excess = float(((np.abs(got - xref) - tol) / np.abs(xref).max()).max())
        after = sysv.cpu().numpy()
        ep32 = float(np.float32(ep))
        pad_damped = ep32 != 0 and bool(np.any(after[:, n + 1:] == ep32))
        print(f"P={P} lm={lm:g} ep={ep:g}: max |dx - x*| / max|x*| {float(np.abs(got - xref).max() / np.abs(xref).max()):.3e}, "
              f"fp64 bar {bar_f:.2e}, |dx|max {float(np.abs(got).max()):.2e}, padding max {np.abs(after[:, n + 1:]).max():.2e}")
        if not np.all(np.isfinite(dx.cpu().numpy())) or excess > 0:
            failures.append((lm, ep, "dx off by %.3e of max|x*| beyond the bar" % excess))
        # S[n, n]: nothing of the solve reads it.  Whatever the factorisation leaves there, it must be what the undamped
        # run (first of the three) left: damped it would differ by ep + lm * CORNER.
        corner = float(after[n, n])
        if corner0 is None:
            corner0 = corner
        print(f"    S[n, n] after the solve {corner!r} (injected {CORNER}, undamped run left {corner0!r})")
        if corner != corner0:
            failures.append((lm, ep, f"S[n, n] = {corner!r}, the undamped run left {corner0!r}: the rhs row was damped"))
        if pad_damped:
            failures.append((lm, ep, "the padding columns hold the damping constant"))
    bd.close()
    assert not failures, failures
