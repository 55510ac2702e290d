"""The end of a Gauss-Newton iteration without a launch of its own.

With depth slots, the pose retraction, dx, the status word and its host mirror are the work of one extra workgroup of
the back-substitution launch (ba_backsub_kernel, blockIdx.x == M, y == 0); the other workgroups read the poses of the
linearisation from a snapshot that a spare workgroup of the linearisation launch leaves in the workspace.  Without
depth slots (motion-only) ba_pose_retr_kernel still ends the iteration.  Everything here goes through the C ABI
(droid_backends.ba / BaBinding) and is held against the fp64 oracle at the bars of tests/test_gpu_ba.py (TOL) and
tests/util.py (STAGE_BARS).
"""
import copy

import numpy as np
import pytest

from util import STAGE_BARS, ba_args, compare_state, run_ba_stages, run_hip_ba, stage_errors, to_dev

pytestmark = pytest.mark.gpu

TOL = 1e-4   # tests/test_gpu_ba.py


def _torch():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    return torch


@pytest.fixture(scope="module")
def synth():
    from droid_backends import synth
    return synth


def _check(backends, oracle, p, iterations, motion_only=False, tag=""):
    """tests/test_gpu_ba.py::_check"""
    torch = _torch()
    hip = run_hip_ba(backends, p, torch, iterations, motion_only)
    ref = oracle.ba(*ba_args(p), iterations, p.lm, p.ep, motion_only, storage_f32=True)
    assert hip["status"] & 11 == 0, f"device status {hip['status']}"
    if not motion_only:
        assert hip["M"] == ref["M"]
    et, er, ed = compare_state(hip, ref, tag)
    assert et < TOL and er < TOL, (et, er)
    assert ed < TOL, ed
    if not motion_only:
        assert np.abs(hip["dz"] - ref["dz"]).max() < 10 * TOL
    return hip, ref


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def _band(N, radius=1):
    e = [(i, j) for i in range(N) for j in (i - radius, i + radius) if 0 <= j < N]
    return np.array([a for a, _ in e]), np.array([b for _, b in e])


# ---- basic parity, and K iterations in one call against K calls -----------------------------------------------------
@pytest.fixture(scope="module")
def small(synth):
    return synth.make_ba_problem(N=5, E=14, H=24, W=32, seed=1)


@pytest.mark.parametrize("K", [1, 2, 3])
def test_basic_parity_and_one_call_equals_k_calls(backends, oracle, small, K):
    torch = _torch()
    hip, _ = _check(backends, oracle, small, K, tag=f"5kf/14e K={K}")
    q = copy.deepcopy(small)
    for _ in range(K):
        one = run_hip_ba(backends, q, torch, 1)
        assert one["status"] & 15 == 0
        q.poses, q.disps = one["poses"], one["disps"]
    dp = int((_bits(hip["poses"]) != _bits(q.poses)).sum())
    dd = int((_bits(hip["disps"]) != _bits(q.disps)).sum())
    print(f"K={K}: words that differ between one call and K calls: poses {dp}, disps {dd}")
    assert dp == 0 and dd == 0
    assert np.array_equal(_bits(hip["dx"]), _bits(one["dx"])) and np.array_equal(_bits(hip["dz"]), _bits(one["dz"]))


# ---- more window poses than a wave, than the old kernel's workgroup ------------------------------------------------
def test_more_than_64_window_poses(backends, oracle, synth):
    """70 keyframes, band edges of radius 1, 8x8: 69 window poses.  Every pose is retracted, by its own dx."""
    torch = _torch()
    N = 70
    p = synth.make_ba_problem(N=N, H=8, W=8, seed=3, edges=_band(N))
    st = run_ba_stages(backends, p, torch)
    assert st["status"] & 15 == 0 and st["M"] == N
    err = stage_errors(oracle, p, st)
    print(f"70 kf: dx {err['dx']:.2e} state {err['state']:.2e} {err['state_parts']}")
    bars = STAGE_BARS["sparse"]
    assert err["dx"] < bars["dx"] and err["state"] < bars["state"], err
    assert st["dx"].shape == (N - 1, 6) and np.all(np.abs(st["dx"]).max(axis=1) > 0)      # dx_out: every row written
    moved = (_bits(st["poses"]) != _bits(p.poses)).any(axis=1)
    assert not moved[0] and moved[1:].all(), np.flatnonzero(~moved)
    # through the one-call entry as well: the same words
    hip = run_hip_ba(backends, p, torch, 1)
    assert np.array_equal(_bits(hip["dx"]), _bits(st["dx"])) and np.array_equal(_bits(hip["poses"]), _bits(st["poses"]))


# ---- the window inside a longer buffer ------------------------------------------------------------------------------
def test_window_inside_buffer(backends, oracle, synth):
    N, t0 = 9, 3
    p = synth.make_ba_problem(N=N, E=34, H=16, W=24, seed=9, nbuf=N + 5, t0=t0)
    hip, _ = _check(backends, oracle, p, 2, tag=f"window t0={t0} nbuf={N + 5}")
    assert np.array_equal(_bits(hip["poses"][:t0]), _bits(p.poses[:t0]))
    assert np.array_equal(_bits(hip["poses"][N:]), _bits(p.poses[N:]))
    assert np.array_equal(_bits(hip["disps"][N:]), _bits(p.disps[N:]))
    assert (_bits(hip["poses"][t0:N]) != _bits(p.poses[t0:N])).any(axis=1).all()


# ---- pixel counts that are no multiple of the workgroup -------------------------------------------------------------
@pytest.mark.parametrize("H,W", [(5, 7), (30, 40)])
def test_ragged_pixel_counts(backends, oracle, synth, H, W):
    """35 pixels: one pixel chunk, most of its lanes idle.  1200: five chunks, so five workgroups share blockIdx.x == M
    and exactly one of them may retract (a second retraction would move every pose twice)."""
    torch = _torch()
    from droid_backends.ba_binding import BaBinding
    p = synth.make_ba_problem(N=4, E=8, H=H, W=W, seed=13)
    b = BaBinding(status_mirror=True, headroom=(1, 0))
    try:
        b.begin(type("D", (), to_dev(p, torch)), p.t0, p.t1, False)
        b.buf.zero_()
        b.mirror.zero_()
        st = run_ba_stages(backends, p, torch, binding=b, fill="keep")
        mirror = [int(x) for x in b.mirror[:4]]
    finally:
        b.close()
    assert st["status"] & 15 == 0
    err = stage_errors(oracle, p, st)
    print(f"{H}x{W}: dx {err['dx']:.2e} state {err['state']:.2e} mirror {mirror}")
    bars = STAGE_BARS["sparse"]
    assert err["dx"] < bars["dx"] and err["state"] < bars["state"], err
    assert mirror[0] == st["status"] and mirror[1] == st["M"] == 4 and mirror[2] == 0 and mirror[3] == 0, mirror
    _check(backends, oracle, p, 2, tag=f"{H}x{W}")


# ---- the step API ---------------------------------------------------------------------------------------------------
def test_step_api_keeps_the_callers_poses_current(backends, oracle, small, synth):
    """prepare, then three times build + solve_update: after every solve_update the caller's tensors hold what the
    one-call path leaves after that many iterations.  Then a problem with a longer buffer on the same binding."""
    torch = _torch()
    from droid_backends.ba_binding import BAProblemDev, BaBinding
    p = small
    want = [run_hip_ba(backends, p, torch, k) for k in (1, 2, 3)]
    b = BaBinding(status_mirror=False)
    try:
        d = BAProblemDev(**to_dev(p, torch))
        E, nbuf, H, W, M, t0, t1 = b.begin(d, p.t0, p.t1, False)
        b.buf.fill_(0xFF)
        dx = torch.zeros((t1 - t0, 6), dtype=torch.float32, device="cuda")
        dz = torch.zeros((M, H * W), dtype=torch.float32, device="cuda")
        b.prepare(d, (0, nbuf), False)
        for k in range(3):
            b.build(d, False)
            b.solve_update(d, p.lm, p.ep, False, dx, dz)
            torch.cuda.synchronize()
            assert b.status()[0] & 15 == 0
            dp = int((_bits(d.poses.cpu().numpy()) != _bits(want[k]["poses"])).sum())
            dd = int((_bits(d.disps.cpu().numpy()) != _bits(want[k]["disps"])).sum())
            print(f"step API after {k + 1} iterations: differing words poses {dp}, disps {dd}")
            assert dp == 0 and dd == 0
            assert np.array_equal(_bits(dx.cpu().numpy()), _bits(want[k]["dx"]))
        # a longer buffer on the same workspace: the snapshot is carved for it, and is written before it is read
        q = synth.make_ba_problem(N=7, E=24, H=24, W=32, seed=4, nbuf=16, t0=2)
        st = run_ba_stages(backends, q, torch, binding=b, fill="keep")
        assert st["status"] & 15 == 0
        err = stage_errors(oracle, q, st)
        bars = STAGE_BARS["sparse"]
        assert err["dx"] < bars["dx"] and err["state"] < bars["state"], err
    finally:
        b.close()


# ---- a factorisation that fails -------------------------------------------------------------------------------------
def test_failed_factorisation_leaves_the_poses(backends, small):
    """A reduced system that is not positive definite (the device's own, its pose block replaced by -I, as
    tests/test_gpu_ba.py::test_chol_failure_flag does for the solver alone): dx = 0, the poses keep every bit, the
    disparities still take dz = Q w, and the status says so."""
    torch = _torch()
    from droid_backends.ba_binding import BAProblemDev, BaBinding
    p = small
    d = BAProblemDev(**to_dev(p, torch))
    b = BaBinding(status_mirror=True, headroom=(1, 0))
    try:
        E, nbuf, H, W, M, t0, t1 = b.begin(d, p.t0, p.t1, False)
        b.buf.zero_()
        b.mirror.zero_()
        n = 6 * (t1 - t0)
        dx = torch.ones((t1 - t0, 6), dtype=torch.float32, device="cuda")
        dz = torch.zeros((M, H * W), dtype=torch.float32, device="cuda")
        b.prepare(d, (0, nbuf), False)
        b.build(d, False)
        S = b.system().view(n + 1, -1)
        S[:n, :n] = -torch.eye(n, dtype=torch.float64, device="cuda")
        b.solve_update(d, p.lm, p.ep, False, dx, dz)
        torch.cuda.synchronize()
        st, m = b.status()
        mirror = [int(x) for x in b.mirror[:4]]
    finally:
        b.close()
    assert st & 4 and not st & 11, st
    assert mirror[0] == st and mirror[1] == m == M, (mirror, st, m)
    assert np.array_equal(_bits(d.poses.cpu().numpy()), _bits(p.poses))
    assert not dx.cpu().numpy().any()
    dzh = dz.cpu().numpy().reshape(M, H, W)
    assert np.isfinite(dzh).all() and np.count_nonzero(dzh) > dzh.size // 2
    kx = np.unique(np.concatenate([np.arange(p.t0, p.t1), p.ii]))          # slot -> frame (synth.make_ba_problem)
    assert np.array_equal(_bits(d.disps.cpu().numpy()[kx]), _bits(p.disps[kx] + dzh))


# ---- no depth slots: ba_pose_retr_kernel ----------------------------------------------------------------------------
@pytest.mark.parametrize("N,t0", [(10, 6), (80, 8)])
def test_motion_only_still_ends_in_its_own_launch(backends, oracle, synth, N, t0):
    """10 / 6: trajectory_filler's call shape (tests/test_gpu_ba.py::test_ba_motion_only), new frames observed from fixed
    keyframes.  80 / 8: 72 window poses, each observed from its two predecessors: two workgroups of the kernel."""
    if N == 10:
        p = synth.make_ba_problem(N=N, E=36, H=16, W=24, seed=7)
        keep = (p.ii < t0) & (p.jj >= t0)
        p.ii, p.jj, p.targets, p.weights = p.ii[keep], p.jj[keep], p.targets[keep], p.weights[keep]
    else:
        e = [(j - d, j) for j in range(t0, N) for d in (1, 2)]
        p = synth.make_ba_problem(N=N, H=16, W=24, seed=7, edges=(np.array([a for a, _ in e]), np.array([b for _, b in e])))
    seen = np.unique(p.jj)                     # the window frames some edge observes: the others have nothing to move by
    assert len(seen) and seen.min() >= t0 and (N == 10 or len(seen) == N - t0)
    p.t0, p.t1 = t0, N
    hip, _ = _check(backends, oracle, p, 2, motion_only=True, tag=f"motion-only {N - t0} poses")
    assert np.array_equal(_bits(hip["poses"][:t0]), _bits(p.poses[:t0]))
    assert (_bits(hip["poses"][seen]) != _bits(p.poses[seen])).any(axis=1).all()
    assert np.array_equal(_bits(hip["disps"]), _bits(p.disps))


# ---- a stream of the caller's ---------------------------------------------------------------------------------------
def test_non_default_stream(backends, oracle, small):
    torch = _torch()
    want = run_hip_ba(backends, small, torch, 2)
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):
        hip, _ = _check(backends, oracle, small, 2, tag="side stream")
    assert np.array_equal(_bits(hip["poses"]), _bits(want["poses"])) and np.array_equal(_bits(hip["disps"]), _bits(want["disps"]))
