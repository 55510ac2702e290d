"""One table of named, seeded systems for the Cholesky-solve accuracy tests.  A case is built on demand
(`case.build()` -> A [n,n] fp64 symmetric, b [n] fp64); nothing here needs a GPU.

Sizes come from the boundaries of the kernels (chol.hip): 6..64 one block column (per-step kernels), 65 / 129 one column
past a 64-column tile, 378 (cfg2), 641, 1025, 1530 / 1536 (cfg3; at 1536 the rhs row is a block row of its own), 2046.

Families
  spectrum       A = Q diag(lambda) Q^T, lambda log-spaced, kappa_2 in {1e2, 1e6, 1e10, 1e12}
  scaled         D A D of the same, D = diag(10^U(-s, s)), s in {3, 4}: metres against radians against pixels
  hard_block     a well-conditioned matrix whose Cholesky factor gets ONE 16-column diagonal block replaced by the factor
                 of a kappa = 1e10 block: after the elimination of the columns before it, exactly that block is what the
                 device factors and inverts explicitly.  (kappa_2 of the whole matrix is then >= 1e10 as well -- a
                 principal block of a Schur complement cannot be worse conditioned than the matrix -- but every other
                 diagonal block, and the matrix without this block, has kappa of a few tens.)
  pow2           one spectrum case times 2^+-200
  definite_edge  lambda_min = +EDGE_M n u lambda_max  (u = 2^-53): must NOT fail
  indefinite     lambda_min = -EDGE_M n u lambda_max: must fail; and planted bad pivots: a negative diagonal entry at
                 columns 0, 15, 16, 63, 64, n-1 (n-1 lies in a partial last block for n = 65, 641), an exact zero on the
                 diagonal of a diagonal matrix
  camera         the damped / undamped reduced camera systems of the BA oracle (`camera_cases`, needs the oracle)

EDGE_M: a Cholesky factorisation in fp64 succeeds when lambda_min > c n u lambda_max and must break down when
lambda_min < -c n u lambda_max, c of order 1 (Higham, Accuracy and Stability, thm 10.7; in practice c << 1).  8 leaves a
factor of 8 to that bound on either side; tests/test_chol_ref.py checks that the three CPU solvers succeed on every
definite_edge case and that LAPACK potrf raises on every indefinite one.

SPREAD_FWD, SPREAD_OMEGA: how far correct fp64 solvers lie apart.  Over all non-failing cases of this table (camera
systems included), per metric, the largest ratio between the worst and the best of the three CPU solvers
(tests/chol_ref.py), each clamped below at 2^-53, rounded up to the next power of two.  Measured, not chosen
(test_chol_ref.py::test_spread_constants_cover_the_table recomputes them with BLAS pinned to one thread: 70.2 and 13.9;
with 2, 4, 8 threads the same table gave 12.1 / 47.7 / 15.7 and 15.1 / 15.8 / 14.0).  The forward-error figure is set by
the definite_edge cases, where kappa ~ 1e12 and the error of any one solver is luck within two orders; omega by LU with
partial pivoting on the scaled cases, which is not scaling-invariant.  The device may lie this factor above the WORST of
the three on the same case, no further.  SPREAD is the single figure over both metrics; keeping the two apart only makes
the omega bar tighter.
"""
import zlib
from dataclasses import dataclass, field
from typing import Callable, Optional

import numpy as np

U = 2.0 ** -53
EDGE_M = 8
SPREAD_FWD = 128.0
SPREAD_OMEGA = 16.0
SPREAD = max(SPREAD_FWD, SPREAD_OMEGA)
KAPPAS = (1e2, 1e6, 1e10, 1e12)


@dataclass
class Case:
    name: str
    family: str
    n: int
    build: Callable = field(repr=False)
    kappa: Optional[float] = None       # what the name claims (of the unscaled matrix / of the hard block)
    fails: bool = False
    bad_col: Optional[int] = None       # planted bad pivot
    block: Optional[int] = None         # hard_block: index of the 16-column block
    unscale: Optional[Callable] = field(default=None, repr=False)   # scaled: -> the D of D A D


def _rng(name):
    return np.random.default_rng(zlib.crc32(name.encode()))


def _orth(rng, n):
    q, r = np.linalg.qr(rng.normal(size=(n, n)))
    return q * np.sign(np.diag(r))


def spectrum_matrix(rng, n, lam):
    q = _orth(rng, n)
    A = (q * lam) @ q.T
    return 0.5 * (A + A.T)


def _logspace(n, kappa):
    return np.logspace(0.0, -np.log10(kappa), n) if n > 1 else np.ones(1)


def _spectrum(name, n, kappa):
    def build():
        rng = _rng(name)
        return spectrum_matrix(rng, n, _logspace(n, kappa)), rng.normal(size=n)
    return build


def _scale_vector(name, n, s):
    return 10.0 ** np.random.default_rng(zlib.crc32((name + "/D").encode())).uniform(-s, s, size=n)


def _scaled(name, n, kappa, s):
    def build():
        rng = _rng(name)
        A, b = spectrum_matrix(rng, n, _logspace(n, kappa)), rng.normal(size=n)
        d = _scale_vector(name, n, s)
        A = d[:, None] * A * d[None, :]
        return 0.5 * (A + A.T), d * b
    return build


def _well(rng, n):
    G = rng.normal(size=(n, n + 8))
    return G @ G.T + 0.1 * n * np.eye(n)


def _hard_block(name, n, blk, kappa):
    def build():
        rng = _rng(name)
        L = np.linalg.cholesky(_well(rng, n))
        k, e = 16 * blk, min(16 * blk + 16, n)
        w = e - k
        scale = float(np.mean(np.diag(L)[k:e] ** 2))
        B = spectrum_matrix(rng, w, scale * _logspace(w, kappa))
        L[k:e, k:e] = np.linalg.cholesky(B)
        A = L @ L.T
        return 0.5 * (A + A.T), rng.normal(size=n)
    return build


def _pow2(name, base, n, kappa, e):
    def build():
        A, b = _spectrum(base, n, kappa)()
        return np.ldexp(A, e), np.ldexp(b, e)
    return build


def _edge(name, n, sign):
    def build():
        rng = _rng(name)
        lam = np.concatenate([np.logspace(0.0, -2.0, n - 1), [sign * EDGE_M * n * U]])
        return spectrum_matrix(rng, n, lam), rng.normal(size=n)
    return build


def _planted(name, n, col):
    def build():
        rng = _rng(name)
        A, b = _well(rng, n), rng.normal(size=n)
        A[col, col] = -1.0
        return A, b
    return build


def _zero_diag(name, n, col):
    def build():
        rng = _rng(name)
        d = rng.uniform(1.0, 2.0, size=n)
        d[col] = 0.0
        return np.diag(d), rng.normal(size=n)
    return build


def _table():
    t = []
    for n in (6, 63, 64, 65, 129, 378, 1530):
        for k in KAPPAS:
            name = f"spectrum/n{n}/k{k:.0e}"
            t.append(Case(name, "spectrum", n, _spectrum(name, n, k), kappa=k))
    for n in (42, 641, 1025, 1536, 2046):
        for k in (1e6, 1e12):
            name = f"spectrum/n{n}/k{k:.0e}"
            t.append(Case(name, "spectrum", n, _spectrum(name, n, k), kappa=k))
    for n in (42, 65, 378, 1025, 1530):
        for k, s in ((1e6, 3), (1e10, 4)):
            name = f"scaled/n{n}/k{k:.0e}/s{s}"
            t.append(Case(name, "scaled", n, _scaled(name, n, k, s), kappa=k,
                          unscale=(lambda nm=name, nn=n, ss=s: _scale_vector(nm, nn, ss))))
    # block 0, the 4th block of a tile, the last full block, the partial last block (378 = 23*16+10, 1530 = 95*16+10)
    for n, blocks in ((129, (0, 3, 7)), (378, (0, 3, 22, 23)), (1530, (0, 3, 94, 95))):
        for blk in blocks:
            name = f"hard_block/n{n}/b{blk}"
            t.append(Case(name, "hard_block", n, _hard_block(name, n, blk, 1e10), kappa=1e10, block=blk))
    for e in (200, -200):
        name = f"pow2/n378/k1e+06/e{e:+d}"
        t.append(Case(name, "pow2", 378, _pow2(name, "spectrum/n378/k1e+06", 378, 1e6, e), kappa=1e6))
    for n in (64, 129, 378, 1530):
        name = f"definite_edge/n{n}"
        t.append(Case(name, "definite_edge", n, _edge(name, n, +1.0), kappa=1.0 / (EDGE_M * n * U)))
        name = f"indefinite/n{n}"
        t.append(Case(name, "indefinite", n, _edge(name, n, -1.0), fails=True))
    for n, cols in ((129, (0, 15, 16, 63, 64, 128)), (1530, (0, 15, 16, 63, 64, 1529)), (65, (64,)), (641, (640,)),
                    (42, (41,))):
        for c in cols:
            name = f"indefinite/n{n}/neg_at{c}"
            t.append(Case(name, "indefinite", n, _planted(name, n, c), fails=True, bad_col=c))
    for n, c in ((42, 17), (130, 64)):
        name = f"indefinite/n{n}/zero_at{c}"
        t.append(Case(name, "indefinite", n, _zero_diag(name, n, c), fails=True, bad_col=c))
    return t


CASES = _table()
BY_NAME = {c.name: c for c in CASES}
assert len(BY_NAME) == len(CASES)
SOLVABLE = [c for c in CASES if not c.fails]
FAILING = [c for c in CASES if c.fails]
FAMILIES = ("spectrum", "scaled", "camera", "hard_block", "pow2", "definite_edge")


def damp(H, lm, ep):
    """diag += ep + lm*diag in fp64, lm / ep rounded to float32 like the C ABI's arguments."""
    lm, ep = float(np.float32(lm)), float(np.float32(ep))
    A = np.tril(H) + np.tril(H, -1).T
    A[np.diag_indices_from(A)] += ep + lm * np.diag(A)
    return A


# graphs of the camera family: the BA configurations plus one dense graph of tests/stage_graphs.py
CAMERA_GRAPHS = ("cfg1", "cfg2", "cfg3", "dense36_syrk")


_CAMERA_SYSTEMS = {}      # graph name -> (H, b, lm, ep) of the oracle's first iteration: computed once per process


def camera_cases(oracle, synth, graphs=CAMERA_GRAPHS):
    """The reduced camera systems of the oracle's first iteration, damped as the solver damps them and undamped."""
    from stage_graphs import GRAPHS
    from util import ba_args
    out = []
    for g in graphs:
        if g not in _CAMERA_SYSTEMS:
            p = GRAPHS[g][0](synth)
            ref = oracle.ba(*ba_args(p), 1, p.lm, p.ep, False, debug=True)
            _CAMERA_SYSTEMS[g] = (np.asarray(ref["H"], np.float64), np.asarray(ref["b"], np.float64), p.lm, p.ep)
        H, b, plm, pep = _CAMERA_SYSTEMS[g]
        n = H.shape[0]
        for tag, lm, ep in (("damped", plm, pep), ("undamped", 0.0, 0.0)):
            A = damp(H, lm, ep)
            out.append(Case(f"camera/{g}/{tag}", "camera", n, (lambda A=A, b=b: (A, b))))
    return out
