"""CPU tests that pin the yardsticks of the Cholesky-solve accuracy tests before the device is measured with them:
the longdouble reference (`chol_ref.solve_ld`) on problems whose solution is known without a solver, against mpmath at
50 digits and against its own fast variants; the case table (`chol_cases`) against what its names claim; and the spread
between three correct fp64 CPU solvers, which is the room the device gets (`chol_cases.SPREAD`).  No GPU.
Wall time of the module: about 50 s on one core, most of it the three solvers on the n >= 1025 cases."""
import numpy as np
import pytest

import chol_cases as C
import chol_ref as R

LD = R.LD
U_LD = float(np.finfo(LD).eps) / 2


@pytest.fixture(scope="module")
def synth():
    from droid_backends import synth
    return synth


def _integer_problem(n, seed):
    rng = np.random.default_rng(seed)
    L = np.tril(rng.integers(-3, 4, size=(n, n))).astype(np.float64)
    L[np.diag_indices(n)] = rng.integers(1, 5, size=n)
    x = rng.integers(-9, 10, size=n).astype(np.float64)
    A = L @ L.T                     # integers below 2^53: exact
    return A, A @ x, x


@pytest.mark.parametrize("n", [1, 2, 5, 16, 17, 40])
def test_solve_ld_is_exact_on_integer_problems(n):
    """A = L L^T with a small integer L, b = A x with an integer x: every intermediate of the factorisation and of the
    substitutions is an integer (the pivots are perfect squares), so the longdouble solve returns x itself."""
    A, b, x = _integer_problem(n, 7 + n)
    assert np.array_equal(R.solve_ld(A, b), x.astype(LD))
    assert np.array_equal(R.solve_ld_columns(A, b), x.astype(LD))
    assert R.forward_error(R.solve_ld_refined(A, b), x) < 64 * U_LD * np.linalg.cond(A)
    assert R.omega(A, x, b) == 0.0
    # the upper triangle is never read
    junk = A + np.triu(np.full((n, n), 1e30), 1)
    assert np.array_equal(R.solve_ld(junk, b), x.astype(LD))
    for name, f in R.SOLVERS.items():
        assert R.forward_error(f(junk, b), x) < 64 * n * 2.0 ** -53 * np.linalg.cond(A), name


def test_solve_ld_rejects_a_non_positive_pivot():
    A = np.diag([1.0, 2.0, -1.0, 3.0])
    for f in (R.solve_ld, R.solve_ld_columns, R.solve_ld_refined, R.solve_potrf, R.solve_blockinv):
        with pytest.raises(np.linalg.LinAlgError):
            f(A, np.ones(4))


@pytest.mark.parametrize("name", ["spectrum/n6/k1e+02", "spectrum/n6/k1e+12", "scaled/n42/k1e+10/s4",
                                  "camera40"])
def test_solve_ld_against_mpmath(name):
    """50-digit LU in mpmath on the fp64 data, n <= 42.  A longdouble Cholesky solve has a forward error of at most about
    n kappa u_ld (Higham thm 10.4 with cond <= kappa); it is asserted with that bound, and with a componentwise
    backward error of a handful of longdouble roundings measured in mpmath itself."""
    import mpmath as mp
    if name == "camera40":
        rng = np.random.default_rng(40)
        A, b = C.spectrum_matrix(rng, 40, np.logspace(0, -6, 40)), rng.normal(size=40)
    else:
        A, b = C.BY_NAME[name].build()
    n = len(b)
    x = R.solve_ld(A, b)
    with mp.workdps(50):
        Am = mp.matrix([[mp.mpf(float(v)) for v in row] for row in R.sym_lower(A)])
        bm = mp.matrix([mp.mpf(float(v)) for v in b])
        xm = mp.lu_solve(Am, bm)
        xl = mp.matrix([mp.mpf(int(m)) * mp.mpf(2) ** int(e) for m, e in
                        (_mant_exp(v) for v in x)])
        err = max(abs(xl[i] - xm[i]) for i in range(n)) / max(abs(xm[i]) for i in range(n))
        r = Am * xl - bm
        den = [sum(abs(Am[i, j]) * abs(xl[j]) for j in range(n)) + abs(bm[i]) for i in range(n)]
        om = max(abs(r[i]) / den[i] for i in range(n))
    kappa = np.linalg.cond(_jacobi(A))      # scaling-invariant bound: Cholesky's error follows the scaled matrix
    print(f"{name}: forward error vs mpmath {float(err):.2e} (n kappa u_ld = {n * kappa * U_LD:.2e}), omega {float(om):.2e}")
    assert float(om) < 2 * n * U_LD
    assert float(err) < n * kappa * U_LD * max(1.0, float(np.abs(_dscale(A)).max()))
    # and the module's own longdouble metrics say the same as mpmath's
    assert abs(R.omega(A, x, b) - float(om)) <= 0.5 * float(om) + U_LD


def _mant_exp(v):
    """longdouble -> (integer mantissa, exponent), exactly."""
    m, e = np.frexp(v)
    hi = np.floor(np.ldexp(m, 32))
    lo = np.ldexp(m, 32) - hi
    return int(hi) * 2 ** 32 + int(np.ldexp(lo, 32)), int(e) - 64


def _jacobi(A):
    d = 1.0 / np.sqrt(np.diag(A))
    return d[:, None] * R.sym_lower(A) * d[None, :]


def _dscale(A):
    """Spread of the diagonal scaling: forward errors in the max norm pick up the ratio of the scales."""
    d = np.sqrt(np.diag(A))
    return d.max() / d


@pytest.mark.parametrize("name", ["spectrum/n129/k1e+06", "spectrum/n378/k1e+10", "scaled/n378/k1e+06/s3",
                                  "hard_block/n378/b23", "definite_edge/n129", "pow2/n378/k1e+06/e-200"])
def test_refinement_variant_reaches_the_plain_solve(name):
    """n <= 400: the textbook solve, its column-vectorised form and the refinement around LAPACK agree to the accuracy a
    longdouble solve has on that system, and all three have the backward error of a longdouble solve."""
    A, b = C.BY_NAME[name].build()
    n = len(b)
    x0, x1, x2 = R.solve_ld(A, b), R.solve_ld_columns(A, b), R.solve_ld_refined(A, b)
    kappa = np.linalg.cond(_jacobi(A))
    bound = n * kappa * U_LD * float(np.abs(_dscale(A)).max())
    e1, e2 = R.forward_error(x1, x0), R.forward_error(x2, x0)
    oms = [R.omega(A, x, b) for x in (x0, x1, x2)]
    print(f"{name}: columns vs plain {e1:.2e}, refined vs plain {e2:.2e} (bound {bound:.2e}); omega {oms}")
    assert e1 < bound and e2 < bound
    assert max(oms) < 2 * n * U_LD
    # the references differ from each other by less than a tenth of the BEST fp64 solver's error: forward errors
    # measured against either are good to 10 %, the bars they feed have a factor SPREAD of room
    best64 = min(R.forward_error(x, x0) for x in R.cpu_solvers(A, b).values())
    assert max(e1, e2) < 0.1 * max(best64, R.FLOOR)


def test_table_covers_the_kernel_boundaries():
    sizes = {c.n for c in C.CASES}
    assert {6, 42, 63, 64, 65, 129, 378, 641, 1025, 1530, 1536, 2046} <= sizes
    fams = {c.family for c in C.CASES}
    assert fams == {"spectrum", "scaled", "hard_block", "pow2", "definite_edge", "indefinite"}
    planted = {(c.n, c.bad_col) for c in C.FAILING if c.bad_col is not None}
    for n in (129, 1530):
        assert {(n, col) for col in (0, 15, 16, 63, 64, n - 1)} <= planted
    assert {(65, 64), (641, 640)} <= planted
    assert {c.block for c in C.CASES if c.family == "hard_block" and c.n == 378} == {0, 3, 22, 23}
    a, _ = C.BY_NAME["spectrum/n65/k1e+06"].build()
    b, _ = C.BY_NAME["spectrum/n65/k1e+06"].build()
    assert np.array_equal(a, b)                     # seeded by name: reproducible


@pytest.mark.parametrize("case", [c for c in C.SOLVABLE if c.family in ("spectrum", "scaled", "pow2")],
                         ids=lambda c: c.name)
def test_spectrum_cases_have_the_kappa_they_claim(case):
    A, _ = case.build()
    if case.unscale is not None:
        d = case.unscale()
        assert d.max() / d.min() > 10.0 ** (1.5 * float(case.name[-1]))   # the scales really spread
        A = A / d[:, None] / d[None, :]
    ev = np.linalg.eigvalsh(A / np.abs(A).max())    # eigvalsh's error is u lambda_max: 1e-4 of lambda_min at kappa 1e12
    kappa = ev[-1] / ev[0]
    assert ev[0] > 0 and 0.9 < kappa / case.kappa < 1.1, (case.name, kappa)


@pytest.mark.parametrize("case", [c for c in C.CASES if c.family == "hard_block"], ids=lambda c: c.name)
def test_hard_block_is_hard_after_elimination(case):
    """The 16-column diagonal block the device factors and inverts, i.e. the Schur complement of the columns before it,
    has kappa 1e10; the neighbouring diagonal blocks and the matrix without the block's rows have a kappa of tens."""
    A, _ = case.build()
    n, k = case.n, 16 * case.block
    e = min(k + 16, n)

    def schur_block(k, e):
        S = A[k:e, k:e].copy()
        if k:
            S -= A[k:e, :k] @ np.linalg.solve(A[:k, :k], A[:k, k:e])
        return S
    kb = np.linalg.cond(schur_block(k, e))
    assert 0.5 < kb / case.kappa < 2.0, (case.name, kb)
    other = 16 * (case.block - 1) if case.block else 16
    assert np.linalg.cond(schur_block(other, other + 16)) < 1e3
    keep = np.r_[0:k, e:n]
    assert np.linalg.cond(A[np.ix_(keep, keep)]) < 1e3


def test_edge_cases_sit_where_their_names_say():
    """definite_edge: lambda_min = +EDGE_M n u lambda_max and every CPU solver succeeds; indefinite: the mirror image and
    LAPACK potrf raises; every planted bad pivot fails in LAPACK.  Conditions on the inputs, not tolerances."""
    import scipy.linalg as sla
    for c in C.CASES:
        if c.family not in ("definite_edge", "indefinite"):
            continue
        A, b = c.build()
        if c.bad_col is None:
            ev = np.linalg.eigvalsh(A)
            want = (-1.0 if c.fails else 1.0) * C.EDGE_M * c.n * C.U
            # eigvalsh itself errs by about u lambda_max, an eighth of n u at n = 64 and far less beyond
            assert 0.5 < (ev[0] / ev[-1]) / want < 2.0, (c.name, ev[0] / ev[-1], want)
        if c.fails:
            with pytest.raises(np.linalg.LinAlgError):
                sla.cho_factor(A, lower=True)
            with pytest.raises(np.linalg.LinAlgError):
                R.solve_blockinv(A, b)
        else:
            for name, x in R.cpu_solvers(A, b).items():
                assert np.all(np.isfinite(x)), (c.name, name)


def test_spread_constants_cover_the_table(oracle, synth):
    """The room the device gets.  For every non-failing case (the camera systems of the oracle included) both metrics of
    the three CPU solvers against the longdouble reference, each clamped below at 2^-53; spread = the largest
    worst-to-best ratio per metric.  The stored constants must cover it (how tightly is printed, not asserted: the figures move
    with the BLAS build).  BLAS is pinned to one thread: the blocking, and with it the rounding, of LAPACK follows the thread count."""
    import threadpoolctl
    worst, at = [0.0, 0.0], [None, None]
    with threadpoolctl.threadpool_limits(limits=1):
        for c in C.SOLVABLE + C.camera_cases(oracle, synth):
            A, b = c.build()
            _, errs = R.cpu_yardstick(A, b)
            line = []
            for m, tag in ((0, "fwd"), (1, "omega")):
                v = [R.clamp(e[m]) for e in errs.values()]
                ratio = max(v) / min(v)
                line.append(f"{tag} " + " ".join(f"{e[m]:.1e}" for e in errs.values()) + f" ratio {ratio:.1f}")
                if ratio > worst[m]:
                    worst[m], at[m] = ratio, c.name
                # omega of a backward-stable solver is a modest multiple of u whatever kappa is: that is what makes it
                # a yardstick (Higham thm 10.4: gamma_{3n+1} normwise; in practice a few u componentwise)
                if m == 1:
                    assert max(v) < 64 * C.U, (c.name, errs)
            print(f"{c.name:34s} " + " | ".join(line))
    print(f"spread: forward {worst[0]:.2f} at {at[0]} (stored {C.SPREAD_FWD}), omega {worst[1]:.2f} at {at[1]} "
          f"(stored {C.SPREAD_OMEGA})")
    assert worst[0] <= C.SPREAD_FWD
    assert worst[1] <= C.SPREAD_OMEGA
    assert C.SPREAD == max(C.SPREAD_FWD, C.SPREAD_OMEGA)


SENSITIVITY_CASES = ["spectrum/n6/k1e+02", "spectrum/n64/k1e+02", "spectrum/n65/k1e+06", "spectrum/n378/k1e+06",
                     "spectrum/n378/k1e+12", "scaled/n378/k1e+10/s4", "scaled/n42/k1e+06/s3", "hard_block/n378/b3",
                     "hard_block/n129/b0", "definite_edge/n378", "pow2/n378/k1e+06/e+200", "spectrum/n1025/k1e+06"]


def _inexact_rsqrt(kind, seed):
    """1/sqrt(d) the way a damaged pivot reciprocal of the device would return it.  `seed`: the 24-bit hardware seed
    alone; `1e-11`: a relative error of 1e-11; `halley2`: seed error delta, e = 2 delta, and the second-order term of
    the Halley step dropped, y (1 - 3/8 e^2): at most 2^-47.4, a quarter of that on average."""
    rng = np.random.default_rng(seed)

    def f(d):
        y = 1.0 / np.sqrt(d)
        delta = rng.uniform(-2.0 ** -24, 2.0 ** -24)
        if kind == "seed":
            return y * (1.0 + delta)
        if kind == "1e-11":
            return y * (1.0 + 1e-11 * np.sign(delta))
        return y * (1.0 - 0.375 * (2.0 * delta) ** 2)
    return f


def test_what_loss_the_bars_resolve():
    """The bars of tests/test_gpu_chol_accuracy.py, applied to the CPU restatement with a damaged pivot reciprocal: what
    size of loss do they see?  Asserted: the 24-bit seed alone and a relative error of 1e-11 per pivot (the older tests'
    1e-10 bar passes the latter) miss the omega bar on EVERY case.  Reported, not asserted: the Halley step without its
    second-order term (about 2^-48 per pivot, 3.6e-15) stays UNDER the bars on all twelve cases -- three correct fp64 solvers
    lie up to 16 apart in omega, and a loss of a few tens of roundings per pivot is inside that."""
    seen = {"seed": 0, "1e-11": 0, "halley2": 0}
    for name in SENSITIVITY_CASES:
        A, b = C.BY_NAME[name].build()
        xref, errs = R.cpu_yardstick(A, b)
        bar_f, bar_w = R.bars(errs, (C.SPREAD_FWD, C.SPREAD_OMEGA))
        line = []
        for kind in seen:
            try:
                x = R.solve_blockinv(A, b, rsqrt=_inexact_rsqrt(kind, len(name)))
                ef, ew = R.both_metrics(A, x, b, xref)
            except np.linalg.LinAlgError:
                ef = ew = float("inf")
            caught = not (ef <= bar_f and ew <= bar_w)
            seen[kind] += caught
            line.append(f"{kind}: fwd {ef:.1e} omega {ew:.1e} {'CAUGHT' if caught else 'passes'}")
            if kind != "halley2":
                assert not ew <= bar_w, (name, kind, ew, bar_w)
        print(f"{name:28s} bars fwd {bar_f:.1e} omega {bar_w:.1e} | " + " | ".join(line))
    print(f"caught of {len(SENSITIVITY_CASES)}: {seen}")
