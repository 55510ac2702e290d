"""The call sequence of `PoseTrajectoryFiller.__fill` (droid_slam/trajectory_filler.py:43-72) replayed at the extension
boundary, without lietorch and without a host read between the steps: pose_interpolate fills the poses of the new
frames and hands its int64 brackets straight to the edge list, then the motion-only `ba` refines them.  The problem is
the one tests/test_gpu_ba.py::test_ba_motion_only holds to the oracle (10 frames, window [6, 10)), and so is the bar."""
import copy

import numpy as np
import pytest

from test_gpu_ba import TOL
from util import ba_args, compare_state

pytestmark = pytest.mark.gpu

N_KEY, N_ALL = 6, 10


def test_filler_replay_matches_the_oracle(backends, oracle):
    import torch
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    from droid_backends import synth
    import se3_ref

    p = synth.make_ba_problem(N=N_ALL, E=36, H=48, W=64, seed=7)
    stamps = np.float32([0, 3, 5, 8, 12, 15, 16, 19, 21, 26])            # increasing: the new frames follow the keyframes
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()
    poses, disps, tstamp = dev(p.poses), dev(p.disps), dev(stamps)
    poses0, disps0 = poses.clone(), disps.clone()

    # trajectory_filler.py:44-58: brackets and interpolated poses of the frames [6, 10) from the first 6
    Gs, k0, k1 = backends.pose_interpolate(poses, tstamp, N_KEY, tstamp[N_KEY:N_ALL])
    poses[N_KEY:N_ALL] = Gs.data
    ref_G, ref_k0, ref_k1 = se3_ref.interpolate(p.poses, stamps, N_KEY, stamps[N_KEY:])
    assert np.array_equal(k0.cpu().numpy(), ref_k0) and np.array_equal(k1.cpu().numpy(), ref_k1)
    assert np.array_equal(Gs.data.cpu().numpy(), ref_G.astype(np.float32))   # past the last stamp: P[k0] itself
    # :66-68: the edge list, from the operator's outputs as they are
    new = torch.arange(N_KEY, N_ALL, device="cuda")
    ii, jj = torch.cat([k0, k1]), torch.cat([new, new])
    assert ii.dtype == torch.int64 and ii.is_cuda

    q = copy.deepcopy(p)
    q.poses = poses.cpu().numpy()
    q.ii, q.jj = ii.cpu().numpy(), jj.cpu().numpy()
    q.t0, q.t1 = N_KEY, N_ALL
    intr = [float(v) for v in p.intrinsics]
    coords, Z = synth.reproject(p.gt_poses, p.gt_disps, intr, q.ii, q.jj)
    rng = np.random.default_rng(70)
    H, W = p.disps.shape[1:]
    ok = (coords[:, 0] >= 0) & (coords[:, 0] <= W - 1) & (coords[:, 1] >= 0) & (coords[:, 1] <= H - 1) & (Z >= 0.25)
    q.targets = (coords + rng.normal(0, 0.25, coords.shape)).astype(np.float32)
    q.weights = (rng.uniform(0, 1, coords.shape) * ok[:, None]).astype(np.float32)
    assert q.weights.max() > 0

    dx, dz = backends.ba(poses, disps, dev(q.intrinsics), dev(q.disps_sens), dev(q.targets), dev(q.weights), dev(q.eta),
                         ii, jj, q.t0, q.t1, 3, q.lm, q.ep, True)
    torch.cuda.synchronize()
    st, m = backends.ba_status()
    assert st & 11 == 0, f"device status {st}"
    hip = dict(poses=poses.cpu().numpy(), disps=disps.cpu().numpy(), dx=dx.cpu().numpy())
    ref = oracle.ba(*ba_args(q), 3, q.lm, q.ep, True, storage_f32=True)
    et, er, ed = compare_state(hip, ref, "filler replay")
    assert et < TOL and er < TOL, (et, er)
    assert ed < TOL, ed
    assert np.abs(hip["poses"][N_KEY:] - q.poses[N_KEY:]).max() > 1e-3          # the window did move
    assert torch.equal(poses[:N_KEY], poses0[:N_KEY]) and torch.equal(disps, disps0)   # bit-unchanged
