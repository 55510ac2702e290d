"""The pose algebra on the device (droid_se3_unary, droid_se3_mul, droid_pose_interpolate; droid_backends.se3) against
the float64 restatement tests/se3_ref.py, over the table of tests/se3_cases.py, component by component:

    |out - ref| <= 2^-23 |ref| + 2^-36 S

S = 1 + the largest |translation component| among the inputs and the reference output of the record; for the
interpolation S is multiplied by 1 + |t - ts[k0]| / dt.  The bound is derived, not measured: the first term is one
float32 rounding of the result with one unit of slack for a tie; the second is fewer than 200 fp64 operations on
intermediates below about 25 S (the factors of V and V^-1), each with 2^-53 relative error -- about 2^-41 S -- times 32
for the device's fp64 sin / cos / atan.  It lies 2^12 below what an fp32 evaluation loses in the same cancellations, so
it also checks that the arithmetic is what the contract says.  Every output is written into a buffer with a canary
region before and after it.  The C ABI is called directly (the Python class allocates its own outputs); the class is
checked against those bits."""
import numpy as np
import pytest

import se3_cases
import se3_ref

pytestmark = pytest.mark.gpu

INV, LOG, EXP, MATRIX = 0, 1, 2, 3
WIDTH_IN = {INV: 7, LOG: 7, EXP: 6, MATRIX: 7}
WIDTH_OUT = {INV: 7, LOG: 6, EXP: 7, MATRIX: 16}
PAD = 64
CANARY_F, CANARY_I = -1234.5, -77


def _torch():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    return torch


class Guarded:
    """A device buffer of `numel` elements between two canary regions."""

    def __init__(self, torch, numel, dtype=None):
        dtype = dtype or torch.float32
        self.canary = CANARY_F if dtype.is_floating_point else CANARY_I
        self.numel = numel
        self.big = torch.full((numel + 2 * PAD,), self.canary, dtype=dtype, device="cuda")
        self.view = self.big[PAD:PAD + numel]

    def ptr(self):
        return self.view.data_ptr()

    def result(self, *shape):
        """The payload on the host, after checking that neither canary region was touched."""
        host = self.big.cpu().numpy()
        assert (host[:PAD] == self.canary).all() and (host[PAD + self.numel:] == self.canary).all(), "canary overwritten"
        return host[PAD:PAD + self.numel].reshape(shape).copy()


def _stream(torch):
    return torch.cuda.current_stream().cuda_stream


def _dev(torch, a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def run_unary(backends, x, op):
    torch = _torch()
    lib = backends._lib.load()
    n = len(x)
    d = _dev(torch, x)
    out = Guarded(torch, n * WIDTH_OUT[op])
    assert lib.droid_se3_unary(d.data_ptr(), out.ptr(), n, op, _stream(torch)) == 0, lib.droid_last_error()
    return out.result(n, WIDTH_OUT[op])


def run_mul(backends, a, b, sa=7, sb=7, n=None):
    torch = _torch()
    lib = backends._lib.load()
    n = max(len(a), len(b)) if n is None else n
    da, db = _dev(torch, a), _dev(torch, b)
    out = Guarded(torch, n * 7)
    assert lib.droid_se3_mul(da.data_ptr(), sa, db.data_ptr(), sb, out.ptr(), n, _stream(torch)) == 0, lib.droid_last_error()
    return out.result(n, 7)


def run_interpolate(backends, poses, ts, N, query):
    torch = _torch()
    lib = backends._lib.load()
    M = len(query)
    dp, dt, dq = _dev(torch, poses), _dev(torch, ts), _dev(torch, np.asarray(query, dtype=np.float32))
    out, k0, k1 = Guarded(torch, M * 7), Guarded(torch, M, torch.int64), Guarded(torch, M, torch.int64)
    rc = lib.droid_pose_interpolate(dp.data_ptr(), dt.data_ptr(), N, dq.data_ptr() if M else None, M, out.ptr(), k0.ptr(),
                                    k1.ptr(), _stream(torch))
    assert rc == 0, lib.droid_last_error()
    return out.result(M, 7), k0.result(M), k1.result(M)


def assert_within_bound(got, ref, S, tag):
    """|got - ref| <= 2^-23 |ref| + 2^-36 S per component; NaN exactly where the reference has NaN."""
    assert got.dtype == np.float32 and got.shape == ref.shape, (tag, got.dtype, got.shape, ref.shape)
    nan = np.isnan(ref)
    assert np.array_equal(np.isnan(got), nan), tag
    with np.errstate(invalid="ignore"):
        err = np.abs(got.astype(np.float64) - ref)
        bound = 2.0 ** -23 * np.abs(ref) + 2.0 ** -36 * np.asarray(S, dtype=np.float64).reshape(-1, 1)
        ratio = np.where(nan, 0.0, err / bound)
    worst = np.unravel_index(ratio.argmax(), ratio.shape) if ratio.size else None
    print(f"[{tag}] n = {len(ref)}: worst error / bound = {ratio.max() if ratio.size else 0:.3f}")
    assert (ratio <= 1.0).all(), (tag, worst, float(err[worst]), float(bound[worst]), ref[worst[0]])


REF_UNARY = {INV: se3_ref.inv, LOG: se3_ref.log, EXP: se3_ref.exp, MATRIX: lambda a: se3_ref.matrix(a).reshape(-1, 16)}


def _translations(op, x, ref):
    """The translation components among input and reference output ([n, 3] each)."""
    return x[:, :3], (ref[:, [3, 7, 11]] if op == MATRIX else ref[:, :3])


@pytest.fixture(scope="module")
def tables():
    return {"poses": se3_cases.poses(), "tangents": se3_cases.tangents()}


@pytest.mark.parametrize("op,name", [(INV, "inv"), (LOG, "log"), (EXP, "exp"), (MATRIX, "matrix")])
def test_unary_ops_over_the_table(backends, tables, op, name):
    table = tables["tangents" if op == EXP else "poses"]
    for x in se3_cases.batches(table):
        got = run_unary(backends, x, op)
        ref = REF_UNARY[op](x)
        assert_within_bound(got, ref, se3_cases.translation_scale(*_translations(op, x, ref)), name)
        assert np.array_equal(run_unary(backends, x, op), got), "two runs differ"
    if op == MATRIX:
        assert np.array_equal(got[:, 12:], np.tile(np.float32([0, 0, 0, 1]), (len(got), 1)))


def test_log_of_minus_q_and_of_scaled_q_on_the_device(backends, tables):
    """log(c q) = log(q) for c = -1, 0.5, 2: the log of the scaled record is held to the reference log of the
    UNSCALED one, at the same bound -- except at exactly w = 0, where +pi v/n follows the sign of v."""
    a = tables["poses"]
    ref = se3_ref.log(a)
    la = run_unary(backends, a, LOG)
    flip = a[:, 6] == 0
    for c in (-1.0, 0.5, 2.0):
        b = a.copy()
        b[:, 3:] *= np.float32(c)     # exact in float32
        lb = run_unary(backends, b, LOG)
        keep = ~flip if c < 0 else np.ones(len(a), bool)
        assert_within_bound(lb[keep], ref[keep], se3_cases.translation_scale(a[keep], ref[keep]), f"log({c} q)")
        if c < 0:
            assert np.array_equal(lb[flip, 3:], -la[flip, 3:])
    assert np.linalg.norm(la[:, 3:].astype(np.float64), axis=1).max() <= np.pi * (1 + 2.0 ** -23)


def test_mul_over_the_table(backends, tables):
    table = tables["poses"]
    for a in se3_cases.batches(table):
        b = np.roll(a, 5, axis=0)[::-1].copy()
        got = run_mul(backends, a, b)
        ref = se3_ref.mul(a, b)
        assert_within_bound(got, ref, se3_cases.translation_scale(a, b, ref), "mul")
        assert np.array_equal(run_mul(backends, a, b), got), "two runs differ"


def test_mul_broadcasts_one_record_bit_for_bit(backends, tables):
    a = tables["poses"][:257]
    one = tables["poses"][300:301]
    assert np.array_equal(run_mul(backends, a, one, 7, 0), run_mul(backends, a, np.repeat(one, len(a), 0)))
    assert np.array_equal(run_mul(backends, one, a, 0, 7), run_mul(backends, np.repeat(one, len(a), 0), a))
    both = run_mul(backends, one, a[:1], 0, 0, n=65)
    assert np.array_equal(both, np.repeat(run_mul(backends, one, a[:1]), 65, 0))


def test_in_place_gives_the_bits_of_out_of_place(backends, tables):
    torch = _torch()
    lib = backends._lib.load()
    a, b = tables["poses"][:257], tables["poses"][100:357]
    s = _stream(torch)
    d = _dev(torch, a)
    assert lib.droid_se3_unary(d.data_ptr(), d.data_ptr(), len(a), INV, s) == 0
    assert np.array_equal(d.cpu().numpy(), run_unary(backends, a, INV))
    want = run_mul(backends, a, b)
    da, db = _dev(torch, a), _dev(torch, b)
    assert lib.droid_se3_mul(da.data_ptr(), 7, db.data_ptr(), 7, da.data_ptr(), len(a), s) == 0      # out == a
    assert np.array_equal(da.cpu().numpy(), want)
    da = _dev(torch, a)
    assert lib.droid_se3_mul(da.data_ptr(), 7, db.data_ptr(), 7, db.data_ptr(), len(a), s) == 0      # out == b
    assert np.array_equal(db.cpu().numpy(), want)
    da = _dev(torch, a)
    assert lib.droid_se3_mul(da.data_ptr(), 7, da.data_ptr(), 7, da.data_ptr(), len(a), s) == 0      # a == b == out
    assert np.array_equal(da.cpu().numpy(), run_mul(backends, a, a))
    torch.cuda.synchronize()


def test_the_class_matches_the_abi(backends, tables):
    """droid_backends.SE3: every method gives the bits of the direct call; indexing, cat and broadcasting."""
    torch = _torch()
    from droid_backends import se3
    SE3 = backends.SE3
    a = tables["poses"][:130]
    P = SE3(_dev(torch, a).view(2, 65, 7))
    assert tuple(P.shape) == (2, 65) and len(P) == 2 and P.device.type == "cuda"
    assert np.array_equal(P.inv().data.cpu().numpy().reshape(-1, 7), run_unary(backends, a, INV))
    assert np.array_equal(P.log().cpu().numpy().reshape(-1, 6), run_unary(backends, a, LOG))
    M = P.matrix()
    assert tuple(M.shape) == (2, 65, 4, 4)
    assert np.array_equal(M.cpu().numpy().reshape(-1, 16), run_unary(backends, a, MATRIX))
    xi = tables["tangents"][:65]
    G = SE3.exp(_dev(torch, xi))
    assert isinstance(G, SE3) and np.array_equal(G.data.cpu().numpy(), run_unary(backends, xi, EXP))
    # products: equal shapes, one record on either side, an indexed operand (a non-contiguous view made contiguous)
    prod = (P[0] * P[1]).data.cpu().numpy()
    assert np.array_equal(prod, run_mul(backends, a[:65], a[65:]))
    T = P[1, 7]
    assert tuple(T.shape) == () and tuple((T * P).shape) == (2, 65)
    assert np.array_equal((T * P).data.cpu().numpy().reshape(-1, 7), run_mul(backends, a[72:73], a, 0, 7))
    assert np.array_equal((P * T[None]).data.cpu().numpy().reshape(-1, 7), run_mul(backends, a, a[72:73], 7, 0))
    col = P[:, 3]
    assert np.array_equal((col * col.inv()).data.cpu().numpy(),
                          run_mul(backends, a[[3, 68]], run_unary(backends, a[[3, 68]], INV)))
    idx = torch.tensor([64, 0, 3], device="cuda")
    assert np.array_equal(P[1][idx].inv().data.cpu().numpy(), run_unary(backends, a[65:][[64, 0, 3]], INV))
    both = se3.cat([P[0], P[1]], 0)
    assert tuple(both.shape) == (130,) and np.array_equal(both.data.cpu().numpy(), a)
    with pytest.raises(RuntimeError, match="neither match nor hold a single record"):
        P[0][:3] * P[1][:4]
    with pytest.raises(TypeError, match="droid_backends.reproject"):
        P * torch.zeros((2, 65, 3), device="cuda")
    empty = SE3(torch.zeros((0, 7), device="cuda"))
    assert tuple(empty.inv().data.shape) == (0, 7) and tuple(empty.matrix().shape) == (0, 4, 4)
    assert tuple((empty * empty).data.shape) == (0, 7)
    # the visualiser's and terminate's lines
    Ps = SE3(P.data[0]).inv().matrix().cpu().numpy()
    assert np.array_equal(Ps.reshape(-1, 16), run_unary(backends, run_unary(backends, a[:65], INV), MATRIX))


# ---- interpolation --------------------------------------------------------------------------------------------------

def _check_interpolation(backends, P, ts, N, query, tag):
    got, k0, k1 = run_interpolate(backends, P, ts, N, query)
    ref, r0, r1 = se3_ref.interpolate(P, ts, N, query)
    assert k0.dtype == np.int64 and np.array_equal(k0, r0) and np.array_equal(k1, r1), (tag, k0, r0, k1, r1)
    ts64, q64 = np.asarray(ts, np.float32).astype(np.float64), np.asarray(query, np.float32).astype(np.float64)
    with np.errstate(invalid="ignore"):
        ratio = np.abs(q64 - ts64[r0]) / (ts64[r1] - ts64[r0] + 1e-3)
        live = (r1 != r0) & np.isfinite(ratio)
        assert (ratio[live] <= 4.0).all(), (tag, "input condition |t - ts[k0]| / dt <= 4", ratio)
        rel = se3_ref.log(se3_ref.mul(P[r1], se3_ref.inv(P[r0])))[:, 3:]
        assert (np.linalg.norm(rel[live], axis=1) <= 3.0).all(), (tag, "input condition: relative rotation <= 3 rad")
        S = se3_cases.translation_scale(P[r0], P[r1], np.nan_to_num(ref)) * (1.0 + np.nan_to_num(ratio))
    assert_within_bound(got, ref, S, tag)
    same = r0 == r1
    finite = same & ~np.isnan(ref).any(-1)
    assert np.array_equal(got[finite], P[r0[finite]]), (tag, "k1 == k0 must return P[k0] itself")
    got2, k0b, k1b = run_interpolate(backends, P, ts, N, query)
    assert np.array_equal(got2, got, equal_nan=True) and np.array_equal(k0b, k0) and np.array_equal(k1b, k1), "two runs differ"
    return got, k0, k1


def test_interpolate_single_keyframe(backends):
    P = se3_cases.trajectory(3, seed=11)
    ts = np.float32([5.0, 6.0, 7.0])                      # N = 1: the rows beyond N are never read into the result
    got, k0, k1 = _check_interpolation(backends, P, ts, 1, [0.0, 5.0, 9.0, np.nan], "N=1")
    assert k0.tolist() == [0, 0, 0, 0] and k1.tolist() == [0, 0, 0, 0]
    assert np.array_equal(got[:3], np.repeat(P[:1], 3, 0)) and np.isnan(got[3]).all()


def test_interpolate_two_keyframes_wide_bracket(backends):
    """N = 2, a relative rotation of 2.9 rad at translation scale 100, extrapolated to 3.75 brackets backwards."""
    xi = np.concatenate([[30.0, -20.0, 10.0], 2.9 * np.array([0.6, -0.64, 0.48])])
    P0 = np.concatenate([[100.0, -80.0, 60.0], [0.1, 0.2, -0.3, np.sqrt(1 - 0.14)]])
    P = np.stack([P0, se3_ref.mul(se3_ref.exp(xi), P0)]).astype(np.float32)
    ts = np.float32([10.0, 12.0])
    got, k0, k1 = _check_interpolation(backends, P, ts, 2, [2.5, 4.0, 10.0, 11.0, 11.999, 12.0, 12.5, 18.0], "N=2")
    assert k0.tolist() == [0, 0, 0, 0, 0, 1, 1, 1] and k1.tolist() == [1, 1, 1, 1, 1, 1, 1, 1]


def test_interpolate_filler_brackets_with_nan(backends):
    P = se3_cases.trajectory(5, seed=3)
    ts = np.float32(se3_cases.FILLER_STAMPS)
    query = list(se3_cases.FILLER_QUERIES) + [np.nan]
    got, k0, k1 = _check_interpolation(backends, P, ts, 5, query, "N=5")
    assert list(zip(k0.tolist(), k1.tolist())) == list(se3_cases.FILLER_BRACKETS) + [(0, 1)]
    assert np.isnan(got[-1]).all() and not np.isnan(got[:-1]).any()
    ts_nan = ts.copy()
    ts_nan[2] = np.nan                                     # never counted; a bracket that touches it is NaN
    got, k0, k1 = _check_interpolation(backends, P, ts_nan, 5, query, "N=5, NaN stamp")
    assert list(zip(k0.tolist(), k1.tolist())) == [(0, 1), (0, 1), (0, 1), (1, 2), (1, 2), (2, 3), (3, 4), (3, 4), (0, 1)]
    assert np.isnan(got[[3, 4, 5, 8]]).all() and not np.isnan(got[[0, 1, 2, 6, 7]]).any()


def test_interpolate_long_buffer(backends):
    """N = 4097: the count takes 65 passes of the wave over the stamps; M = 16 queries, a filler chunk."""
    N = 4097
    P = se3_cases.trajectory(N, seed=5)
    ts = np.arange(N, dtype=np.float32) * 2
    rng = np.random.default_rng(6)
    query = np.concatenate([rng.uniform(0, 2 * (N - 1), 10), [-3.0, 0.0, 127.0, 128.0, 8192.0, 8200.0]]).astype(np.float32)
    got, k0, k1 = _check_interpolation(backends, P, ts, N, query, "N=4097")
    assert k0[-6:].tolist() == [0, 0, 63, 64, 4096, 4096] and k1[-6:].tolist() == [1, 1, 64, 65, 4096, 4096]
    assert len(set(k0.tolist()) & set(range(64, 4096))) >= 8            # beyond the first pass of the wave


def test_interpolate_no_queries(backends):
    P = se3_cases.trajectory(4, seed=8)
    got, k0, k1 = run_interpolate(backends, P, np.float32([0, 1, 2, 3]), 4, [])
    assert got.shape == (0, 7) and k0.shape == (0,) and k1.shape == (0,)


def test_python_interpolate_takes_any_real_query(backends):
    torch = _torch()
    P = se3_cases.trajectory(6, seed=9)
    ts = np.float32([0, 3, 5, 8, 13, 21])
    query = [1, 4, 6, 13, 30]
    want, r0, r1 = run_interpolate(backends, P, ts, 6, query)
    big = torch.zeros((512, 7), device="cuda")            # the buffers of DepthVideo are longer than the counter
    big[:6] = _dev(torch, P)
    stamps = torch.zeros(512, device="cuda")
    stamps[:6] = _dev(torch, ts)
    for q in (query, np.asarray(query, dtype=np.int64), np.asarray(query, dtype=np.float64),
              torch.tensor(query, dtype=torch.int32), torch.tensor(query, dtype=torch.float64, device="cuda")):
        G, k0, k1 = backends.pose_interpolate(big, stamps, 6, q)
        assert isinstance(G, backends.SE3) and tuple(G.shape) == (5,)
        assert k0.dtype == torch.int64 and k0.is_cuda and k1.dtype == torch.int64
        assert np.array_equal(G.data.cpu().numpy(), want)
        assert np.array_equal(k0.cpu().numpy(), r0) and np.array_equal(k1.cpu().numpy(), r1)
    G, k0, k1 = backends.pose_interpolate(big, stamps, 6, [])
    assert tuple(G.data.shape) == (0, 7) and tuple(k0.shape) == (0,)
    with pytest.raises(RuntimeError, match="n = 600"):
        backends.pose_interpolate(big, stamps, 600, query)
    # without k0 / k1 (NULL) the poses are the same
    lib = backends._lib.load()
    out = torch.empty((5, 7), device="cuda")
    dq = torch.tensor(query, dtype=torch.float32, device="cuda")
    assert lib.droid_pose_interpolate(big.data_ptr(), stamps.data_ptr(), 6, dq.data_ptr(), 5, out.data_ptr(), None, None,
                                      _stream(torch)) == 0
    assert np.array_equal(out.cpu().numpy(), want)
