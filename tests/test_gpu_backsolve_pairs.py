"""The back-substitution with two block columns per workgroup (chol_backsolve_pairs_kernel, the default after a
single-launch factorisation) against the one with one column per workgroup (DROID_CHOL_BS_PAIRS=0) and against the
CPU yardstick of tests/chol_ref.py, at the sizes where the pairing has an edge (tests/bs_pairs_cases.py).

Both settings solve every system once, each in one child process (the switch is read once per process); the tests
compare what the children left.  Bars: 1e-10 of max |x| between the two paths on the well-conditioned matrix (the bar
and the matrix of test_gpu_robustness.py::test_solver_launch_modes_agree); forward error and componentwise backward
error within the spread of tests/chol_cases.py times the worst of three CPU fp64 solvers, as
tests/test_gpu_chol_accuracy.py holds every other solve.  Two behaviour cases at n = 193 (four block columns: two
pairs) and the host-side pairing against a restatement, which needs no GPU."""
import ctypes
import os
import subprocess
import sys

import numpy as np
import pytest

import bs_pairs_cases as B
import chol_cases as C
import chol_device
import chol_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HERE = os.path.dirname(os.path.abspath(__file__))
gpu = pytest.mark.gpu


def _torch():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    return torch


@pytest.fixture(scope="module")
def solutions(tmp_path_factory):
    """{setting: npz of the child's solutions} for the default path ("pairs") and DROID_CHOL_BS_PAIRS=0 ("single")."""
    res = {}
    for tag, val in (("pairs", None), ("single", "0")):
        e = dict(os.environ)
        e.pop("DROID_CHOL_BS_PAIRS", None)
        if val is not None:
            e["DROID_CHOL_BS_PAIRS"] = val
        path = str(tmp_path_factory.mktemp("bs_pairs") / f"{tag}.npz")
        out = subprocess.run([sys.executable, "-c", B.CHILD % {"root": ROOT, "here": HERE}, path], env=e,
                             capture_output=True, text=True, timeout=600)
        assert out.returncode == 0, out.stderr[-3000:]
        res[tag] = dict(np.load(path))
        if any(int(v[1]) == 2 for k, v in res[tag].items() if k.startswith("rcfl_")):
            pytest.exit(f"droid_chol_solve reported a stalled grid (flag 2) [{tag}]: find the cause before anything runs again", 3)
    return res


def _solution(solutions, tag, kind, n):
    k = B.key(kind, n)
    assert k in solutions[tag], (tag, k, "not solved")
    rc, fl = (int(v) for v in solutions[tag]["rcfl_" + k])
    assert rc == 0 and fl == 0, (tag, k, rc, fl)
    x = solutions[tag][k]
    assert np.all(np.isfinite(x)), (tag, k)
    return x


@gpu
@pytest.mark.parametrize("n", B.SIZES)
def test_pairs_agree_with_one_column_per_workgroup(solutions, n):
    xp, xs = _solution(solutions, "pairs", "well", n), _solution(solutions, "single", "well", n)
    rel = float(np.abs(xp - xs).max() / np.abs(xs).max())
    print(f"n {n}: pairs against single columns {rel:.3e}")
    assert rel < 1e-10, (n, rel)


@gpu
@pytest.mark.parametrize("kind", B.KINDS)
@pytest.mark.parametrize("n", B.SIZES)
def test_pairs_within_the_spread_of_cpu_solvers(solutions, n, kind):
    A, b = B.build(kind, n)
    xref, errs = R.cpu_yardstick(A, b)
    bar_f, bar_w = R.bars(errs, (C.SPREAD_FWD, C.SPREAD_OMEGA))
    ef, ew = R.both_metrics(A, _solution(solutions, "pairs", kind, n), b, xref)
    es, ws = R.both_metrics(A, _solution(solutions, "single", kind, n), b, xref)
    print(f"{kind} n {n}: fwd {ef:.2e} (bar {bar_f:.2e}, single columns {es:.2e})  omega {ew:.2e} (bar {bar_w:.2e}, "
          f"single columns {ws:.2e})")
    assert ef <= bar_f and ew <= bar_w, (kind, n, ef, bar_f, ew, bar_w)


@gpu
@pytest.mark.parametrize("col", [0, 100, 192])
def test_not_positive_definite_raises_the_flag_and_returns(backends, col):
    """A negative diagonal entry in the first pair, in the second, and in the ragged last column: the factorisation
    reports 1 (the caller's dx = 0 path), and the back-substitution behind it ends without the stall value."""
    torch = _torch()
    lib = backends._lib.load()
    rng = np.random.default_rng(193 + col)
    A, b = C._well(rng, 193), rng.normal(size=193)
    A[col, col] = -1.0
    rc, fl, x, scratch = chol_device.solve(lib, torch, A, b)
    if fl == 2:
        pytest.exit("droid_chol_solve reported a stalled grid (flag 2): find the cause before anything runs again", 3)
    assert rc == 0 and fl == 1, (rc, fl)
    A, b = B.build("well", 193)   # and the scratch is fit for the next solve
    rc, fl, x, _ = chol_device.solve(lib, torch, A, b, scratch)
    ref = np.linalg.solve(A, b)
    assert rc == 0 and fl == 0 and np.abs(x - ref).max() / np.abs(ref).max() < 1e-10


@gpu
@pytest.mark.parametrize("at", [0, 130, 192])
def test_nan_in_the_right_hand_side_comes_back_as_nan(backends, at):
    """x is its own arrival flag (all-ones bytes = not there yet): a NaN that is DATA must travel down the chain as a
    value.  From `at` on the forward substitution makes y NaN, so every x is NaN; no stall is reported."""
    torch = _torch()
    lib = backends._lib.load()
    A, b = B.build("well", 193)
    b = b.copy()
    b[at] = np.nan
    rc, fl, x, _ = chol_device.solve(lib, torch, A, b)
    if fl == 2:
        pytest.exit("droid_chol_solve read a NaN as 'never arrived' (flag 2): find the cause before anything runs again", 3)
    assert rc == 0 and fl == 0, (rc, fl)
    assert np.all(np.isnan(x)), np.flatnonzero(~np.isnan(x))[:8]


def test_host_side_pairing_of_block_columns(backends):
    """Workgroup J owns the block columns 2J and 2J+1; with an odd count the top workgroup owns one.  Held against
    this restatement for 1..40 block columns (no GPU: host arithmetic of the launcher)."""
    lib = ctypes.CDLL(backends._lib.LIB_PATH)
    fn = lib.droid_debug_bs_pairs_map
    fn.restype, fn.argtypes = ctypes.c_int, [ctypes.c_int, ctypes.POINTER(ctypes.c_int)]
    for nb in range(1, 41):
        owner = (ctypes.c_int * nb)()
        grid = fn(nb, owner)
        owner = list(owner)
        assert grid == (nb + 1) // 2
        assert owner == [j // 2 for j in range(nb)]
        cols = {J: [j for j in range(nb) if owner[j] == J] for J in range(grid)}
        for J in range(grid):
            want = [2 * J, 2 * J + 1] if 2 * J + 1 < nb else [2 * J]
            assert cols[J] == want, (nb, J, cols[J])
        assert [J for J in cols if len(cols[J]) == 1] == ([grid - 1] if nb % 2 else [])
