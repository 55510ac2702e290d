"""Residency / concurrency / error-reporting behaviour of the BA solver (VERDICT r01 task 7):

* two full-size solves launched concurrently on two streams are serialised by the library and both correct
  (two spinning grids must never overlap);
* a capped grid (DROID_CHOL_GRID below the tile count), the cooperative launch (DROID_CHOL_COOPERATIVE=1) and the
  per-step kernels (DROID_CHOL_MULTI_LAUNCH=1) all give the same solution (environment switches are read once per
  process, so each runs in a child process);
* contract violations are raised by the NEXT `ba` call without a synchronising read (status mirror), and
  `ba` calls on different streams use separate workspaces;
* index / dtype checks on the host."""
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _torch():
    import torch
    assert torch.cuda.is_available()
    return torch


def _spd(n, seed):
    rng = np.random.default_rng(seed)
    A = rng.normal(size=(n, n + 8))
    return A @ A.T + n * 0.1 * np.eye(n), rng.normal(size=n)


def test_two_concurrent_full_size_solves_on_two_streams(backends):
    """n = 1530 (the headline system): 300 tiles -> every CU holds a workgroup of the first grid when the second
    launch arrives on another stream.  Without serialisation the two spinning grids can hold each other's CUs."""
    torch = _torch()
    lib = backends._lib.load()
    n = 1530
    streams = [torch.cuda.Stream(), torch.cuda.Stream()]
    probs = [_spd(n, 11), _spd(n, 12)]
    dA = [torch.from_numpy(A).cuda() for A, _ in probs]
    db = [torch.from_numpy(b).cuda() for _, b in probs]
    xs = [torch.zeros(n, dtype=torch.float64, device="cuda") for _ in probs]
    scr = [torch.zeros(lib.droid_chol_scratch_doubles(n), dtype=torch.float64, device="cuda") for _ in probs]
    flags = [torch.zeros(1, dtype=torch.int32, device="cuda") for _ in probs]
    torch.cuda.synchronize()
    for rep in range(3):
        for k in (0, 1):
            rc = lib.droid_chol_solve(dA[k].data_ptr(), db[k].data_ptr(), xs[k].data_ptr(), n, scr[k].data_ptr(),
                                      flags[k].data_ptr(), streams[k].cuda_stream)
            assert rc == 0
    torch.cuda.synchronize()
    for k in (0, 1):
        assert int(flags[k].item()) == 0
        ref = np.linalg.solve(*probs[k])
        assert np.abs(xs[k].cpu().numpy() - ref).max() / np.abs(ref).max() < 1e-10


_CHILD = r"""
import sys, numpy as np, torch
sys.path[:0] = [r"%(root)s", r"%(root)s/droid-slam_reserch_amd"]
import droid_backends as db
lib = db._lib.load()
rng = np.random.default_rng(3)
worst = 0.0
for n in (1530, 700):
    A = rng.normal(size=(n, n + 8)); A = A @ A.T + n * 0.1 * np.eye(n); b = rng.normal(size=n)
    dA, dbv = torch.from_numpy(A).cuda(), torch.from_numpy(b).cuda()
    x = torch.zeros(n, dtype=torch.float64, device="cuda")
    scratch = torch.zeros(lib.droid_chol_scratch_doubles(n), dtype=torch.float64, device="cuda")
    flag = torch.zeros(1, dtype=torch.int32, device="cuda")
    assert lib.droid_chol_solve(dA.data_ptr(), dbv.data_ptr(), x.data_ptr(), n, scratch.data_ptr(), flag.data_ptr(),
                                torch.cuda.current_stream().cuda_stream) == 0
    torch.cuda.synchronize()
    assert int(flag.item()) == 0, "solver reported failure"
    ref = np.linalg.solve(A, b)
    worst = max(worst, float(np.abs(x.cpu().numpy() - ref).max() / np.abs(ref).max()))
print("WORST", worst)
"""


@pytest.mark.parametrize("env", [{"DROID_CHOL_GRID": "64"}, {"DROID_CHOL_COOPERATIVE": "1"},
                                 {"DROID_CHOL_MULTI_LAUNCH": "1"}, {"DROID_CHOL_COOPERATIVE": "1", "DROID_CHOL_GRID": "96"},
                                 # cooperative back-substitution refused after a single-launch factorisation: the
                                 # per-step kernels must see the factored diagonal tiles
                                 {"DROID_CHOL_COOPERATIVE": "1", "DROID_CHOL_FORCE_BS_REFUSAL": "1"}])
def test_solver_launch_modes_agree(env):
    """64 resident workgroups for 300 tiles (several tiles per workgroup and step), the cooperative launch and the
    per-step fallback: same answer as numpy to 1e-10."""
    e = dict(os.environ)
    e.update(env)
    out = subprocess.run([sys.executable, "-c", _CHILD % {"root": ROOT}], env=e, capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stderr[-2000:]
    worst = float(out.stdout.strip().split("WORST")[-1])
    assert worst < 1e-10, (env, worst)


@pytest.mark.parametrize("n", [6, 42, 63, 64, 65, 127, 129, 378, 641, 1025, 1530, 1536, 2046])
def test_solver_size_sweep(backends, n):
    """Sizes around the 64-column tile and 16-column strip boundaries (partial last block column, single tile, one
    column past a tile), through the single-launch factorisation and back-substitution: numpy to 1e-10."""
    torch = _torch()
    lib = backends._lib.load()
    A, b = _spd(n, 100 + n)
    dA, dbv = torch.from_numpy(A).cuda(), torch.from_numpy(b).cuda()
    x = torch.zeros(n, dtype=torch.float64, device="cuda")
    scratch = torch.zeros(lib.droid_chol_scratch_doubles(n), dtype=torch.float64, device="cuda")
    flag = torch.zeros(1, dtype=torch.int32, device="cuda")
    assert lib.droid_chol_solve(dA.data_ptr(), dbv.data_ptr(), x.data_ptr(), n, scratch.data_ptr(), flag.data_ptr(),
                                torch.cuda.current_stream().cuda_stream) == 0
    torch.cuda.synchronize()
    assert int(flag.item()) == 0
    ref = np.linalg.solve(A, b)
    assert np.abs(x.cpu().numpy() - ref).max() / np.abs(ref).max() < 1e-10


def test_violation_is_raised_by_the_next_call_without_sync(backends):
    """eta with one row too few: the device flags it (status bit 1 << 1); nothing raises in the offending call
    (no synchronisation on the hot path), the next `ba` on the same stream raises, and the one after is clean."""
    torch = _torch()
    from droid_backends import synth
    from util import to_dev
    assert os.environ.get("DROID_HIP_CHECK", "0") != "1"
    p = synth.make_config("cfg1")
    d = to_dev(p, torch)
    args = lambda eta: (d["poses"], d["disps"], d["intrinsics"], d["disps_sens"], d["targets"], d["weights"], eta,
                        d["ii"], d["jj"], p.t0, p.t1, 1, p.lm, p.ep, False)
    backends.ba(*args(d["eta"]))
    torch.cuda.synchronize()
    backends.ba_status()                       # clean slate
    backends.ba(*args(d["eta"][:-1].contiguous()))
    torch.cuda.synchronize()                   # (only so that the test is deterministic)
    with pytest.raises(RuntimeError, match="earlier call.*eta rows"):
        backends.ba(*args(d["eta"]))
    backends.ba(*args(d["eta"]))               # reported once; this call runs
    torch.cuda.synchronize()
    assert backends.ba_status()[0] & 11 == 0


def test_violation_survives_a_later_clean_call_enqueued_before_the_host_looks(backends):
    """call k violates the eta contract, call k+1 (clean) is enqueued right behind it and resets the
    workspace status before the host has looked -- the report must not be lost: the device-side error count and
    bits in the pinned mirror are sticky, and the next `ba` raises."""
    torch = _torch()
    from droid_backends import synth
    from util import to_dev
    p = synth.make_config("cfg1")
    d = to_dev(p, torch)
    args = lambda eta: (d["poses"], d["disps"], d["intrinsics"], d["disps_sens"], d["targets"], d["weights"], eta,
                        d["ii"], d["jj"], p.t0, p.t1, 1, p.lm, p.ep, False)
    backends.ba(*args(d["eta"]))
    torch.cuda.synchronize()
    backends.ba_status()
    # enqueue the violating call and a clean one behind it while the stream is still busy with earlier work
    filler = torch.randn(4096, 4096, device="cuda")
    for _ in range(20):
        filler = filler @ filler * 1e-4
    backends.ba(*args(d["eta"][:-1].contiguous()))
    backends.ba(*args(d["eta"]))               # nothing to report yet at enqueue time (or at most the count of call k)
    torch.cuda.synchronize()
    raised = False
    try:
        backends.ba(*args(d["eta"]))
    except RuntimeError as e:
        raised = "eta rows" in str(e)
    if not raised:                              # the host happened to look between the two calls: then it raised there
        pytest.skip("the violating call had already finished when the clean one was enqueued")
    backends.ba(*args(d["eta"]))
    torch.cuda.synchronize()
    assert backends.ba_status()[0] & 11 == 0


def test_workspaces_are_per_stream(backends):
    torch = _torch()
    from droid_backends import synth
    from util import to_dev
    p = synth.make_config("cfg1")
    outs = []
    streams = [torch.cuda.Stream(), torch.cuda.Stream()]
    ds = [to_dev(p, torch), to_dev(p, torch)]
    torch.cuda.synchronize()
    for s, d in zip(streams, ds):
        with torch.cuda.stream(s):
            backends.ba(d["poses"], d["disps"], d["intrinsics"], d["disps_sens"], d["targets"], d["weights"], d["eta"],
                        d["ii"], d["jj"], p.t0, p.t1, 2, p.lm, p.ep, False)
    torch.cuda.synchronize()
    keys = [k for k in backends._workspaces if k[1] in (streams[0].cuda_stream, streams[1].cuda_stream)]
    assert len(keys) == 2
    assert backends._workspaces[keys[0]].buf.data_ptr() != backends._workspaces[keys[1]].buf.data_ptr()
    a, b = ds[0]["poses"].cpu().numpy(), ds[1]["poses"].cpu().numpy()
    assert np.abs(a - b).max() < 1e-6 and np.abs(ds[0]["disps"].cpu().numpy() - ds[1]["disps"].cpu().numpy()).max() < 1e-5


def test_index_and_dtype_checks_on_the_host(backends):
    torch = _torch()
    poses = torch.zeros(4, 7, device="cuda")
    poses[:, 6] = 1
    disps = torch.ones(4, 8, 8, device="cuda")
    K = torch.tensor([4.0, 4.0, 4.0, 4.0], device="cuda")
    i32 = torch.zeros(3, dtype=torch.int32, device="cuda")
    i64 = torch.zeros(3, dtype=torch.int64, device="cuda")
    with pytest.raises(RuntimeError, match="int64"):
        backends.frame_distance(poses, disps, K, i32, i64, 0.3)
    with pytest.raises(RuntimeError, match="int64"):
        backends.projmap(poses, disps, K, i64, i32)
    with pytest.raises(RuntimeError, match="int64"):
        backends.depth_filter(poses, disps, K, i32, torch.ones(3, device="cuda"))
    with pytest.raises(RuntimeError, match="float32"):
        backends.depth_filter(poses, disps, K, i64, torch.ones(3, dtype=torch.float64, device="cuda"))
    with pytest.raises(RuntimeError, match="float32"):
        backends.frame_distance(poses.double(), disps, K, i64, i64, 0.3)
    vol = torch.zeros(1, 8, 8, 8, 8, device="cuda")
    with pytest.raises(RuntimeError, match="float32"):
        backends.corr_index_backward(vol, torch.zeros(1, 2, 8, 8, dtype=torch.float64, device="cuda"),
                                     torch.zeros(1, 7, 7, 8, 8, device="cuda"), 3)


def test_launch_hints_name_the_block_pair_class_and_do_not_change_results(backends):
    """The first kernel of a `ba` call tells the host (page-locked words, never waited for) whether the graph has depth slots
    of the block-pair Schur class; with "none" the library leaves that launch out of the iterations it enqueues after the hint
    has arrived.  The hint is right for a graph without and one with such slots, and the result is the same with the hints
    detached (every launch made)."""
    torch = _torch()
    import copy
    import droid_backends as db
    from droid_backends import synth
    from util import run_hip_ba
    key = (torch.cuda.current_device(), torch.cuda.current_stream().cuda_stream)
    for p, expect_slots in ((synth.make_config("cfg2"), False),
                            (synth.make_ba_problem(N=30, E=720, H=15, W=20, seed=78, lm=1e-4, ep=0.1), True)):
        a = run_hip_ba(backends, copy.deepcopy(p), torch, 4)
        w = db._workspaces[key]
        tag0 = int(w.mirror[4])
        assert tag0 >= 1                                            # the hint of the call has arrived
        assert (int(w.mirror[5]) > 0) == expect_slots, (int(w.mirror[5]), expect_slots)
        w.attach_hints(False)
        b = run_hip_ba(backends, copy.deepcopy(p), torch, 4)
        assert int(w.mirror[4]) == tag0                             # detached: not written
        w.attach_hints()
        assert np.abs(a["poses"] - b["poses"]).max() < 1e-6 and np.abs(a["disps"] - b["disps"]).max() < 1e-6
