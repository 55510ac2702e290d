"""Pins the yardstick of the pose-algebra tests before it judges the device: tests/se3_ref.py (numpy float64) against
scipy's matrix exponential and against the group identities, over the angle list of tests/se3_cases.py (theta -> 0, the
series thresholds, theta -> pi), all within 1e-12 * max(1, translation scale); then the brackets of the interpolation.
No GPU, no product code."""
import numpy as np
import pytest
from scipy.linalg import expm

import se3_cases
import se3_ref

TOL = 1e-12


def _scale(*arrays):
    return np.maximum(1.0, np.max([np.abs(np.asarray(a, np.float64)[..., :3]).max(-1) for a in arrays], axis=0))


def _twist(xi):
    tx, ty, tz, px, py, pz = xi
    return np.array([[0, -pz, py, tx], [pz, 0, -px, ty], [-py, px, 0, tz], [0, 0, 0, 0]], dtype=np.float64)


@pytest.fixture(scope="module")
def xis():
    return se3_cases.tangents().astype(np.float64)


def test_exp_is_the_matrix_exponential(xis):
    got = se3_ref.matrix(se3_ref.exp(xis))
    worst = 0.0
    for xi, M in zip(xis, got):
        err = np.abs(M - expm(_twist(xi))).max() / _scale(xi)
        worst = max(worst, err)
        assert err <= TOL, (xi, err)
    print(f"matrix(exp(xi)) against scipy expm: worst {worst:.1e} of the translation scale")


def test_unit_quaternions_out_of_exp(xis):
    q = se3_ref.exp(xis)[:, 3:]
    assert np.abs((q * q).sum(-1) - 1).max() < 1e-15


def test_log_inverts_exp_below_pi(xis):
    assert np.linalg.norm(xis[:, 3:], axis=1).max() < np.pi
    back = se3_ref.log(se3_ref.exp(xis))
    err = np.abs(back - xis).max(-1) / _scale(xis)
    print(f"log(exp(xi)) - xi: worst {err.max():.1e}")
    assert err.max() <= TOL, xis[err.argmax()]


def test_exp_inverts_log_up_to_the_sign_of_q():
    a = se3_cases.poses().astype(np.float64)
    a[:, 3:] /= np.linalg.norm(a[:, 3:], axis=1, keepdims=True)
    xi = se3_ref.log(a)
    assert np.linalg.norm(xi[:, 3:], axis=1).max() <= np.pi * (1 + 1e-15)
    back = se3_ref.exp(xi)
    sign = np.sign((back[:, 3:] * a[:, 3:]).sum(-1, keepdims=True))
    back[:, 3:] *= sign
    err = np.abs(back - a).max(-1) / _scale(a)
    assert err.max() <= TOL, a[err.argmax()]


def test_product_and_inverse_are_the_matrix_ones(xis):
    a = se3_ref.exp(xis)                       # unit to 1e-16: R(q) is a homomorphism only on unit quaternions
    b = se3_ref.exp(np.roll(xis, 7, axis=0))
    s = _scale(a, b, se3_ref.mul(a, b))
    err = np.abs(se3_ref.matrix(se3_ref.mul(a, b)) - se3_ref.matrix(a) @ se3_ref.matrix(b)).max((-1, -2)) / s
    assert err.max() <= TOL, err.max()
    ident = np.array([0, 0, 0, 0, 0, 0, 1.0])
    for prod in (se3_ref.mul(a, se3_ref.inv(a)), se3_ref.mul(se3_ref.inv(a), a)):
        err = np.abs(prod - ident).max(-1) / _scale(a, se3_ref.inv(a))
        assert err.max() <= TOL, err.max()
    err = np.abs(se3_ref.matrix(se3_ref.inv(a)) - np.linalg.inv(se3_ref.matrix(a))).max((-1, -2)) / _scale(a, se3_ref.inv(a))
    assert err.max() <= TOL, err.max()


def test_matrix_layout():
    M = se3_ref.matrix(np.array([1, 2, 3, 0, 0, np.sin(0.25), np.cos(0.25)]))   # 0.5 rad about z
    want = np.array([[np.cos(0.5), -np.sin(0.5), 0, 1], [np.sin(0.5), np.cos(0.5), 0, 2], [0, 0, 1, 3], [0, 0, 0, 1]])
    assert np.abs(M - want).max() < 1e-15


@pytest.mark.parametrize("c", [-1.0, 0.5, 2.0])
def test_log_ignores_the_scale_and_sign_of_q(c):
    a = se3_cases.poses().astype(np.float64)
    b = a.copy()
    b[:, 3:] *= c
    la, lb = se3_ref.log(a), se3_ref.log(b)
    # exactly w = 0 is the one place where the rotation vector of least norm is not unique (+pi v/n and -pi v/n are the
    # same rotation): the contract picks +pi v/n, so there -q gives -phi
    flip = (a[:, 6] == 0) & (c < 0)
    assert flip.sum() == (24 if c < 0 else 0)
    assert np.array_equal(lb[flip, 3:], -la[flip, 3:])
    err = np.abs(lb - la).max(-1)[~flip] / _scale(a)[~flip]
    assert err.max() <= TOL, (c, a[~flip][err.argmax()])


def test_log_at_w_zero_is_plus_pi_along_v():
    for v in ([1.0, 0, 0], [0.6, 0, 0.8], [-2.0, 0, 0]):
        phi = se3_ref.log(np.array([0, 0, 0] + v + [0.0]))[3:]
        assert np.abs(phi - np.pi * np.array(v) / np.linalg.norm(v)).max() < 1e-15
    phi = se3_ref.log(np.array([0, 0, 0, 1.0, 0, 0, -0.0]))[3:]   # w == 0 whatever its sign bit
    assert phi[0] == np.pi


def test_interpolation_brackets():
    ts = np.array(se3_cases.FILLER_STAMPS, dtype=np.float32)
    P = se3_cases.trajectory(len(ts), seed=3)
    G, k0, k1 = se3_ref.interpolate(P, ts, len(ts), se3_cases.FILLER_QUERIES)
    assert list(zip(k0.tolist(), k1.tolist())) == list(se3_cases.FILLER_BRACKETS)
    assert k0.dtype == np.int64 and k1.dtype == np.int64
    same = k0 == k1
    assert same.sum() == 2
    assert np.array_equal(G[same], P[k0[same]].astype(np.float64))        # exactly P[k0]
    on = [1, 3, 5]   # queries on a stamp: d = 0, so exp(0) P[k0] = P[k0]
    assert np.array_equal(G[on], P[k0[on]].astype(np.float64))
    # between the stamps 0 and 4 at t = 2: half of the relative motion, up to the 1e-3 of dt
    half = se3_ref.mul(se3_ref.exp(se3_ref.log(se3_ref.mul(P[1], se3_ref.inv(P[0]))) * (2.0 / 4.001)), P[0])
    assert np.abs(G[2] - half).max() < 1e-14
    # before the first stamp: extrapolated backwards from the first bracket, not wrapped to the last keyframe
    back = se3_ref.mul(se3_ref.exp(se3_ref.log(se3_ref.mul(P[1], se3_ref.inv(P[0]))) * (-1.0 / 4.001)), P[0])
    assert np.abs(G[0] - back).max() < 1e-14


def test_interpolation_single_keyframe_and_nan():
    P = se3_cases.trajectory(3, seed=4)
    G, k0, k1 = se3_ref.interpolate(P, np.array([5.0, 6.0, 7.0], np.float32), 1, [0.0, 5.0, 9.0])
    assert k0.tolist() == [0, 0, 0] and k1.tolist() == [0, 0, 0]
    assert np.array_equal(G, np.repeat(P[:1].astype(np.float64), 3, 0))
    G, k0, k1 = se3_ref.interpolate(P, np.array([5.0, np.nan, 7.0], np.float32), 3, [np.nan, 7.5])
    assert k0.tolist() == [0, 1] and k1.tolist() == [1, 2]    # the NaN stamp is not counted; the NaN query counts nothing
    assert np.isnan(G).all()                                   # a NaN query, and a bracket that starts on the NaN stamp
