"""droid_chol_solve against an 80-bit reference, with the room correct fp64 CPU solvers need and no more.

For every non-failing case of tests/chol_cases.py (and the reduced camera systems of the oracle) the device solution is
held, in forward error and in componentwise backward error omega, to the per-metric spread times the WORST of three CPU
fp64 solvers on that very case (tests/chol_ref.py; tests/test_chol_ref.py pins all of it on the CPU).  The bars come from
the reference side only.  Failing cases must raise the failure flag (1, never the stall value 2), return, and leave the
scratch fit for the next solve.  The launch modes run a reduced table in child processes (the switches are read once per
process).  Two solves of one system must be bit-identical: chol.hip has no floating-point atomics (atomicMax on the
integer failure word is its only atomic read-modify-write), so any difference is a stale or torn hand-off.

With DROID_CHOL_ACCURACY_TABLE set to a file name, the per-case lines are appended to it (profiles/chol_accuracy.txt is
such a run on an MI355X).  A stalled grid (flag 2) ends the session at once: nothing more is started on a GPU that showed one."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import chol_cases as C
import chol_device
import chol_ref as R

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HERE = os.path.dirname(os.path.abspath(__file__))


def _torch():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    return torch


@pytest.fixture(scope="module")
def synth():
    from droid_backends import synth
    return synth


def device_solve(lib, torch, A, b, scratch=None):
    """chol_device.solve; a stalled grid (flag 2) ends the session."""
    rc, fl, x, scratch = chol_device.solve(lib, torch, A, b, scratch)
    if fl == 2:
        pytest.exit("droid_chol_solve reported a stalled grid (flag 2): find the cause before anything runs again", 3)
    return rc, fl, x, scratch


def _emit(line):
    print(line)
    path = os.environ.get("DROID_CHOL_ACCURACY_TABLE")
    if path:
        with open(path, "a") as f:
            f.write(line + "\n")


def check_case(lib, torch, case, A, b, scratch=None, tag=""):
    """Solve on the device, print the line of the table, return (list of violations, x, scratch)."""
    xref, errs = R.cpu_yardstick(A, b)
    bar_f, bar_w = R.bars(errs, (C.SPREAD_FWD, C.SPREAD_OMEGA))
    rc, fl, x, scratch = device_solve(lib, torch, A, b, scratch)
    bad = []
    if rc != 0 or fl != 0:
        bad.append(f"rc {rc} flag {fl}")
    if not np.all(np.isfinite(x)):
        bad.append("x not finite")
        ef = ew = float("nan")
    else:
        ef, ew = R.both_metrics(A, x, b, xref)
        if not ef <= bar_f:
            bad.append(f"forward error {ef:.3e} > bar {bar_f:.3e}")
        if not ew <= bar_w:
            bad.append(f"omega {ew:.3e} > bar {bar_w:.3e}")
    wf, ww = (max(R.clamp(e[m]) for e in errs.values()) for m in (0, 1))
    _emit(f"{tag}{case:36s} fwd " + " ".join(f"{k} {errs[k][0]:.2e}" for k in R.SOLVERS) + f" hip {ef:.2e} "
          f"(x{ef / wf:.2f} of worst)  omega " + " ".join(f"{k} {errs[k][1]:.2e}" for k in R.SOLVERS) +
          f" hip {ew:.2e} (x{ew / ww:.2f})" + ("  FAIL: " + "; ".join(bad) if bad else ""))
    return bad, x, scratch


@pytest.mark.parametrize("family", C.FAMILIES)
def test_device_within_the_spread_of_cpu_solvers(backends, oracle, synth, family):
    torch = _torch()
    lib = backends._lib.load()
    cases = C.camera_cases(oracle, synth) if family == "camera" else [c for c in C.SOLVABLE if c.family == family]
    assert cases
    failures = {}
    sols = {}
    for c in cases:
        A, b = c.build()
        bad, x, _ = check_case(lib, torch, c.name, A, b)
        sols[c.name] = x
        if bad:
            failures[c.name] = bad
    if family == "pow2":    # reported, not asserted: is the solve invariant under an even power-of-two scaling?
        A, b = C.BY_NAME["spectrum/n378/k1e+06"].build()
        _, _, x0, _ = device_solve(lib, torch, A, b)
        for name, x in sols.items():
            _emit(f"{name:36s} bit-identical to the unscaled solve: {np.array_equal(x, x0)} "
                  f"(max rel diff {np.abs(x - x0).max() / np.abs(x0).max():.2e})")
    assert not failures, failures


def test_failing_cases_raise_the_flag_and_leave_the_scratch_usable(backends):
    """Each failing case once: rc 0, flag 1 (2 would be a stalled grid), the call returns; the next, well-posed solve
    of the same size on the same scratch meets its bars."""
    torch = _torch()
    lib = backends._lib.load()
    failures = {}
    for c in C.FAILING:
        A, b = c.build()
        rc, fl, x, scratch = device_solve(lib, torch, A, b)
        _emit(f"{c.name:36s} rc {rc} flag {fl}")
        if rc != 0 or fl != 1:
            failures[c.name] = [f"rc {rc} flag {fl}, expected 0 / 1"]
            continue
        rng = np.random.default_rng(c.n)
        bad, _, _ = check_case(lib, torch, c.name, C._well(rng, c.n), rng.normal(size=c.n), scratch, tag="  after ")
        if bad:
            failures[c.name + " (following solve)"] = bad
    assert not failures, failures


@pytest.mark.parametrize("n", [64, 65, 129, 378, 641, 1025, 1530, 1536, 2046])
def test_repeated_solves_are_bit_identical(backends, n):
    torch = _torch()
    lib = backends._lib.load()
    A, b = C.spectrum_matrix(np.random.default_rng(n), n, np.logspace(0, -6, n)), np.random.default_rng(n + 1).normal(size=n)
    rc, fl, x0, scratch = device_solve(lib, torch, A, b)
    assert rc == 0 and fl == 0 and np.all(np.isfinite(x0))
    for rep in range(6):
        rc, fl, x, scratch = device_solve(lib, torch, A, b, scratch if rep % 2 else None)
        assert rc == 0 and fl == 0
        assert np.array_equal(x.view(np.uint64), x0.view(np.uint64)), (n, rep, float(np.abs(x - x0).max()))


# ------------------------------------------------------------------------------------------------- launch modes
REDUCED = ["spectrum/n378/k1e+10", "spectrum/n1530/k1e+10", "scaled/n378/k1e+10/s4", "scaled/n1530/k1e+10/s4",
           "hard_block/n378/b22", "hard_block/n1530/b94", "pow2/n378/k1e+06/e+200", "definite_edge/n378",
           "definite_edge/n1530", "camera/cfg2/damped", "camera/cfg3/damped"]
REDUCED_FAILING = ["indefinite/n1530/neg_at1529", "indefinite/n641/neg_at640"]

_CHILD = r"""
import json, sys, numpy as np, torch
sys.path[:0] = [r"%(root)s", r"%(root)s/droid-slam_reserch_amd", r"%(here)s"]
import chol_device
import chol_ref as R
import droid_backends as db
lib = db._lib.load()
data = np.load(sys.argv[1], allow_pickle=False)
names = json.loads(str(data["names"]))
out = {}
def solve(A, b, scratch):
    rc, fl, x, _ = chol_device.solve(lib, torch, A, b, scratch)
    return rc, fl, x
for i, name in enumerate(names):
    A, b, xref = data[f"A{i}"], data[f"b{i}"], data[f"x{i}"]
    n = len(b)
    scratch = torch.zeros(lib.droid_chol_scratch_doubles(n), dtype=torch.float64, device="cuda")
    if f"B{i}" in data.files:      # a failing system first, on the same scratch
        rc, fl, _ = solve(data[f"B{i}"], b, scratch)
        out[name + " (failing)"] = dict(rc=rc, flag=fl)
        if fl == 2:
            break
    rc, fl, x = solve(A, b, scratch)
    fin = bool(np.all(np.isfinite(x)))
    ef, ew = R.both_metrics(A, x, b, xref) if fin else (float("nan"), float("nan"))
    out[name] = dict(rc=rc, flag=fl, finite=fin, fwd=ef, omega=ew)
    if fl == 2:
        break
print("RESULT", json.dumps(out))
"""


@pytest.fixture(scope="module")
def reduced_table(oracle, synth, tmp_path_factory):
    """The reduced table with its references and bars, computed once and handed to the children as one .npz."""
    cam = {c.name: c for c in C.camera_cases(oracle, synth, ("cfg2", "cfg3"))}
    arrays, names, bars = {}, [], {}
    for name in REDUCED + REDUCED_FAILING:
        i = len(names)
        if name in REDUCED_FAILING:
            c = C.BY_NAME[name]
            arrays[f"B{i}"], b = c.build()
            rng = np.random.default_rng(c.n)
            A = C._well(rng, c.n)
        else:
            A, b = (cam[name] if name in cam else C.BY_NAME[name]).build()
        xref, errs = R.cpu_yardstick(A, b)
        arrays[f"A{i}"], arrays[f"b{i}"], arrays[f"x{i}"] = np.ascontiguousarray(A), b, xref
        bars[name] = R.bars(errs, (C.SPREAD_FWD, C.SPREAD_OMEGA))
        names.append(name)
    path = str(tmp_path_factory.mktemp("chol") / "reduced.npz")
    np.savez(path, names=np.array(json.dumps(names)), **arrays)
    return path, names, bars


@pytest.mark.parametrize("env", [{"DROID_CHOL_GRID": "64"}, {"DROID_CHOL_COOPERATIVE": "1"},
                                 {"DROID_CHOL_MULTI_LAUNCH": "1"}, {"DROID_CHOL_COOPERATIVE": "1", "DROID_CHOL_GRID": "96"},
                                 {"DROID_CHOL_COOPERATIVE": "1", "DROID_CHOL_FORCE_BS_REFUSAL": "1"}],
                         ids=lambda e: ",".join(f"{k[11:]}={v}" for k, v in e.items()))
def test_launch_modes_meet_the_same_bars(reduced_table, env):
    """The environments of test_gpu_robustness.py::test_solver_launch_modes_agree, one child each, one after another."""
    path, names, bars = reduced_table
    e = dict(os.environ)
    e.update(env)
    out = subprocess.run([sys.executable, "-c", _CHILD % {"root": ROOT, "here": HERE}, path], env=e, capture_output=True,
                         text=True, timeout=600)
    assert out.returncode == 0, out.stderr[-3000:]
    res = json.loads(out.stdout.split("RESULT", 1)[1])
    failures = {}
    for name in names:
        r = res.get(name)
        assert r is not None, (name, "not run: an earlier case stalled", res)
        bar_f, bar_w = bars[name]
        _emit(f"  [{','.join(f'{k[11:]}={v}' for k, v in env.items())}] {name:34s} fwd {r['fwd']:.2e} (bar {bar_f:.2e}) "
              f"omega {r['omega']:.2e} (bar {bar_w:.2e})")
        if name in REDUCED_FAILING:
            f = res[name + " (failing)"]
            if f["rc"] != 0 or f["flag"] != 1:
                failures[name + " (failing)"] = f
        if not (r["rc"] == 0 and r["flag"] == 0 and r["finite"] and r["fwd"] <= bar_f and r["omega"] <= bar_w):
            failures[name] = (r, bar_f, bar_w)
    assert not failures, (env, failures)
