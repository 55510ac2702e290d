"""The yardsticks of the Cholesky-solve accuracy tests (tests/test_chol_ref.py pins them, tests/test_gpu_chol_accuracy.py
uses them).  Plain numpy / scipy, no GPU.

* `solve_ld`: the reference solution, a textbook Cholesky solve in 80-bit `numpy.longdouble` (unit roundoff 5.4e-20, 3.3
  decimal digits below fp64).  `solve_ld_refined` reaches the same numbers for the large cases by iterative refinement in
  longdouble around a LAPACK fp64 factor; `solve_ld` stays the definition and the two are compared in the CPU tests.
* `cpu_solvers`: three independent, correct fp64 solutions of the same problem.  Their errors, not an a-priori bound, say
  what a correct fp64 solver delivers on a given system.
* `forward_error`, `omega`: the two metrics, evaluated in longdouble.

Every routine reads the LOWER triangle of A only, like droid_chol_solve."""
import numpy as np

LD = np.longdouble
assert np.finfo(LD).eps < 1e-18, "numpy.longdouble is not an extended type here: the reference would be fp64 itself"
FLOOR = 2.0 ** -53     # no fp64 result can be asked to beat one rounding
NB = 16                # block width of the restated algorithm class


def sym_lower(A, dtype=None):
    """Full symmetric matrix from the lower triangle."""
    A = np.asarray(A) if dtype is None else np.asarray(A, dtype)
    return np.tril(A) + np.tril(A, -1).T


def solve_ld(A, b):
    """x of A x = b by the textbook Cholesky algorithm in longdouble (row-wise Cholesky-Banachiewicz, then the two
    substitutions).  Raises LinAlgError on a non-positive pivot."""
    L = np.tril(np.asarray(A, LD))
    b = np.asarray(b, LD)
    n = L.shape[0]
    for i in range(n):
        for j in range(i):
            L[i, j] = (L[i, j] - L[i, :j] @ L[j, :j]) / L[j, j]
        d = L[i, i] - L[i, :i] @ L[i, :i]
        if not d > 0:
            raise np.linalg.LinAlgError(f"pivot {i} is not positive")
        L[i, i] = np.sqrt(d)
    y = np.zeros(n, LD)
    for i in range(n):
        y[i] = (b[i] - L[i, :i] @ y[:i]) / L[i, i]
    x = np.zeros(n, LD)
    for i in range(n - 1, -1, -1):
        x[i] = (y[i] - L[i + 1:, i] @ x[i + 1:]) / L[i, i]
    return x


def solve_ld_columns(A, b):
    """The same algorithm with the inner loop over j vectorised (column-wise, left-looking): O(n) numpy calls per column
    instead of O(n^2) in all.  Same operations up to the order of the sums; used where `solve_ld` takes minutes."""
    L = np.tril(np.asarray(A, LD))
    b = np.asarray(b, LD)
    n = L.shape[0]
    for j in range(n):
        d = L[j, j] - L[j, :j] @ L[j, :j]
        if not d > 0:
            raise np.linalg.LinAlgError(f"pivot {j} is not positive")
        L[j, j] = np.sqrt(d)
        L[j + 1:, j] = (L[j + 1:, j] - L[j + 1:, :j] @ L[j, :j]) / L[j, j]
    y = np.zeros(n, LD)
    for i in range(n):
        y[i] = (b[i] - L[i, :i] @ y[:i]) / L[i, i]
    x = np.zeros(n, LD)
    for i in range(n - 1, -1, -1):
        x[i] = (y[i] - L[i + 1:, i] @ x[i + 1:]) / L[i, i]
    return x


def solve_ld_refined(A, b, max_iter=80):
    """The longdouble solution by iterative refinement: LAPACK fp64 factor, residual and update in longdouble.  Each
    step contracts the error by about kappa * 2^-53, so it converges for every system the fp64 factor exists for; the
    fixed point has the residual of a longdouble solve.  Raises LinAlgError when the fp64 factorisation fails or the
    iteration does not settle."""
    import scipy.linalg as sla
    A64 = sym_lower(A, np.float64)
    Ald = A64.astype(LD)
    b = np.asarray(b, LD)
    c = sla.cho_factor(A64, lower=True, check_finite=False)
    x = sla.cho_solve(c, np.asarray(b, np.float64), check_finite=False).astype(LD)
    last = np.inf
    for _ in range(max_iter):
        r = b - Ald @ x
        # the residual is far below fp64's range of b on the power-of-two cases: scale it to 1 before rounding to fp64
        s = np.abs(r).max()
        if s == 0:
            return x
        dx = sla.cho_solve(c, np.asarray(r / s, np.float64), check_finite=False).astype(LD) * s
        step = float(np.abs(dx).max() / np.abs(x).max())
        if step > 0.5 * last:
            break           # no longer contracting: the updates are the rounding of the longdouble residual
        x = x + dx
        last = step
    # accepted only with the componentwise backward error of a longdouble solve (a few of its roundings; 1e-17 = 180)
    if not omega(A, x, b, Ald) < 1e-17:
        raise np.linalg.LinAlgError("iterative refinement did not converge")
    return x


def reference(A, b):
    """The reference solution of a case: `solve_ld` itself where it is affordable, else the refinement variant."""
    return solve_ld_columns(A, b) if np.shape(A)[0] <= 130 else solve_ld_refined(A, b)


# ------------------------------------------------------------------------------------------------- fp64 solvers
def solve_potrf(A, b):
    import scipy.linalg as sla
    c = sla.cho_factor(np.asarray(A, np.float64), lower=True, check_finite=False)
    return sla.cho_solve(c, np.asarray(b, np.float64), check_finite=False)


def solve_lu(A, b):
    return np.linalg.solve(sym_lower(A, np.float64), np.asarray(b, np.float64))


def _potrf_inv_block(D, rsqrt=None):
    """Cholesky of one diagonal block by column operations (scale column j by 1/sqrt(pivot), subtract its multiples from
    the later columns), applied to the identity stacked below as well: the identity rows end as L^-T.  Returns L and
    W = L^-1.  A non-positive pivot raises.  `rsqrt`: a replacement for d -> 1/sqrt(d) (the sensitivity experiments of
    tests/test_chol_ref.py put a deliberately inexact one here)."""
    w = D.shape[0]
    T = np.vstack([np.tril(D) + np.tril(D, -1).T, np.eye(w)])
    for j in range(w):
        d = T[j, j]
        if not d > 0:
            raise np.linalg.LinAlgError("pivot is not positive")
        T[:, j] *= 1.0 / np.sqrt(d) if rsqrt is None else rsqrt(d)
        for c in range(j + 1, w):
            T[:, c] -= T[c, j] * T[:, j]
    return np.tril(T[:w]), T[w:].T.copy()


def solve_blockinv(A, b, nb=NB, rsqrt=None):
    """fp64 restatement of the device solver's ALGORITHM CLASS, not of its code: right-looking blocked Cholesky of the
    matrix augmented by the right-hand side as one more row, `nb`-column blocks; the panel below a factored diagonal
    block is solved by MULTIPLYING with the explicitly inverted block, and so is every block of the backward
    substitution.  Multiplying by an explicit inverse is not unconditionally backward stable: where this routine needs
    more room than LAPACK, the class does."""
    A = np.asarray(A, np.float64)
    n = A.shape[0]
    S = np.zeros((n + 1, n))
    S[:n] = np.tril(A)
    S[n] = np.asarray(b, np.float64)
    W = []
    for k in range(0, n, nb):
        e = min(k + nb, n)
        L, Wk = _potrf_inv_block(S[k:e, k:e], rsqrt)
        W.append(Wk)
        S[k:e, k:e] = L
        S[e:, k:e] = S[e:, k:e] @ Wk.T                     # panel and rhs row: times L^-T
        P = S[e:, k:e]
        S[e:n, e:] -= np.tril(P[:n - e] @ P[:n - e].T)     # trailing lower triangle
        S[n, e:] -= P[n - e] @ P[:n - e].T                 # rhs row: the forward substitution rides along
    x = np.zeros(n)
    for bi in range(len(W) - 1, -1, -1):
        k = bi * nb
        e = min(k + nb, n)
        x[k:e] = W[bi].T @ (S[n, k:e] - S[e:n, k:e].T @ x[e:])
    return x


SOLVERS = {"potrf": solve_potrf, "lu": solve_lu, "blockinv": solve_blockinv}


def cpu_solvers(A, b):
    """name -> x for the three fp64 solvers."""
    return {k: f(A, b) for k, f in SOLVERS.items()}


# ------------------------------------------------------------------------------------------------------ metrics
def forward_error(x, xref):
    """||x - x*||inf / ||x*||inf in longdouble."""
    x, xref = np.asarray(x, LD), np.asarray(xref, LD)
    return float(np.abs(x - xref).max() / np.abs(xref).max())


def omega(A, x, b, Ald=None):
    """Componentwise (Oettli-Prager) backward error max_i |b - A x|_i / (|A||x| + |b|)_i in longdouble: the smallest
    relative perturbation of the ENTRIES of A and b for which x is exact; invariant under diagonal scaling."""
    if Ald is None:
        Ald = sym_lower(A, LD)
    x, b = np.asarray(x, LD), np.asarray(b, LD)
    r = np.abs(b - Ald @ x)
    den = np.abs(Ald) @ np.abs(x) + np.abs(b)
    ok = den > 0
    assert np.all(r[~ok] == 0)
    return float((r[ok] / den[ok]).max())


def both_metrics(A, x, b, xref, Ald=None):
    return forward_error(x, xref), omega(A, x, b, Ald)


def clamp(v):
    return max(float(v), FLOOR)


def cpu_yardstick(A, b, xref=None):
    """(xref, {solver: (forward error, omega)}) of one case."""
    if xref is None:
        xref = reference(A, b)
    Ald = sym_lower(A, LD)
    return xref, {k: both_metrics(A, x, b, xref, Ald) for k, x in cpu_solvers(A, b).items()}


def bars(errs, spread):
    """The device's bars on one case, (forward, omega): spread[metric] times the worst of the CPU solvers, each clamped
    at one rounding."""
    return tuple(spread[m] * max(clamp(e[m]) for e in errs.values()) for m in (0, 1))
