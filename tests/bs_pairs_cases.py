"""The systems of tests/test_gpu_backsolve_pairs.py and the child process that solves them all under one setting of
DROID_CHOL_BS_PAIRS (the switch is read once per process).  Matrices from tests/chol_cases.py, rebuilt from their names
on either side instead of being shipped between the processes.

Sizes: the edges of the pairing of block columns (64 wide) in the back-substitution that follows a single-launch
factorisation -- two columns (second ragged / full), three (a lone top column above one pair), four, five, the headline
n = 1530 (24 columns), one column more (25, the last a single matrix column wide) and the largest of the existing sweep."""
import zlib

import numpy as np

import chol_cases as C

SIZES = (65, 128, 129, 192, 193, 256, 257, 1530, 1531, 2046)
# "well": G G^T + 0.1 n I, the matrix of test_gpu_robustness.py::test_solver_launch_modes_agree, whose 1e-10 bar the two
# back-substitutions are held to against each other (kappa ~ 10: n kappa u < 1e-11 at n = 2046, so two correct fp64
# solves differ by less).  "k1e6": a logarithmic spectrum of condition 1e6, for the LAPACK-relative bar only.
KINDS = ("well", "k1e6")


def build(kind, n):
    rng = np.random.default_rng(zlib.crc32(f"bs_pairs/{kind}/n{n}".encode()))
    A = C._well(rng, n) if kind == "well" else C.spectrum_matrix(rng, n, C._logspace(n, 1e6))
    return A, rng.normal(size=n)


def key(kind, n):
    return f"{kind}_n{n}"


CHILD = r"""
import sys, numpy as np, torch
sys.path[:0] = [r"%(root)s", r"%(root)s/droid-slam_reserch_amd", r"%(here)s"]
import bs_pairs_cases as B
import chol_device
import droid_backends as db
lib = db._lib.load()
out = {}
for n in B.SIZES:
    for kind in B.KINDS:
        A, b = B.build(kind, n)
        rc, fl, x, _ = chol_device.solve(lib, torch, A, b)
        out[B.key(kind, n)] = x
        out["rcfl_" + B.key(kind, n)] = np.array([rc, fl])
        if fl == 2:      # a stalled grid: nothing more runs on this GPU
            np.savez(sys.argv[1], **out)
            sys.exit(0)
np.savez(sys.argv[1], **out)
"""
