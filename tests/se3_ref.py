"""numpy float64 restatement of the pose algebra of include/droid_backends_hip.h ("pose algebra"): exp, log, inv, mul,
matrix on batches of records (tx ty tz qx qy qz qw) and tangents (tau, phi), and the filler's interpolation written as
the reference's lines (droid_slam/trajectory_filler.py:44-58) with the clamp of k0.  A test helper: the yardstick of
tests/test_gpu_se3.py, itself pinned by tests/test_se3_ref.py (scipy's expm, group identities).  Quaternions are used
as they are, never renormalised.  Inputs of any float dtype are widened to float64 first; nothing is rounded here."""
import numpy as np

SERIES = 1e-4   # squared angle below which V, V^-1 and sin(theta/2)/theta use their series (next term < 1e-22 relative)


def _f64(x):
    return np.asarray(x, dtype=np.float64)


def rotate(q, X):
    """act_so3: X + w uv + v x uv with uv = 2 v x X."""
    v, w = q[..., :3], q[..., 3:4]
    uv = 2.0 * np.cross(v, X)
    return X + w * uv + np.cross(v, uv)


def inv(a):
    a = _f64(a)
    q = np.concatenate([-a[..., 3:6], a[..., 6:7]], -1)
    return np.concatenate([-rotate(q, a[..., :3]), q], -1)


def mul(a, b):
    a, b = np.broadcast_arrays(_f64(a), _f64(b))
    ax, ay, az, aw = (a[..., i] for i in (3, 4, 5, 6))
    bx, by, bz, bw = (b[..., i] for i in (3, 4, 5, 6))
    q = np.stack([aw * bx + ax * bw + ay * bz - az * by,
                  aw * by + ay * bw + az * bx - ax * bz,
                  aw * bz + az * bw + ax * by - ay * bx,
                  aw * bw - ax * bx - ay * by - az * bz], -1)
    return np.concatenate([a[..., :3] + rotate(a[..., 3:], b[..., :3]), q], -1)


def matrix(a):
    a = _f64(a)
    x, y, z, w = (a[..., i] for i in (3, 4, 5, 6))
    M = np.zeros(a.shape[:-1] + (4, 4))
    M[..., 0, 0] = 1 - 2 * (y * y + z * z); M[..., 0, 1] = 2 * (x * y - z * w); M[..., 0, 2] = 2 * (x * z + y * w)
    M[..., 1, 0] = 2 * (x * y + z * w); M[..., 1, 1] = 1 - 2 * (x * x + z * z); M[..., 1, 2] = 2 * (y * z - x * w)
    M[..., 2, 0] = 2 * (x * z - y * w); M[..., 2, 1] = 2 * (y * z + x * w); M[..., 2, 2] = 1 - 2 * (x * x + y * y)
    M[..., :3, 3] = a[..., :3]
    M[..., 3, 3] = 1
    return M


def exp(xi):
    xi = _f64(xi)
    tau, phi = xi[..., :3], xi[..., 3:]
    with np.errstate(invalid="ignore", divide="ignore"):
        th2 = (phi * phi).sum(-1, keepdims=True)
        th = np.sqrt(th2)
        small = th2 < SERIES
        safe = np.where(small, 1.0, th)
        imag = np.where(small, 0.5 - th2 / 48 + th2 ** 2 / 3840 - th2 ** 3 / 645120, np.sin(0.5 * safe) / safe)
        a = np.where(small, 0.5 - th2 / 24 + th2 ** 2 / 720 - th2 ** 3 / 40320, 2 * np.sin(0.5 * safe) ** 2 / safe ** 2)
        b = np.where(small, 1 / 6 - th2 / 120 + th2 ** 2 / 5040 - th2 ** 3 / 362880, (safe - np.sin(safe)) / safe ** 3)
        u = np.cross(phi, tau)
        t = tau + a * u + b * np.cross(phi, u)
        out = np.concatenate([t, imag * phi, np.cos(0.5 * th)], -1)
    return out + 0.0 * th2   # a NaN angle is a NaN record (np.where above would have picked a branch)


def log(a):
    a = _f64(a)
    t, v, w = a[..., :3], a[..., 3:6], a[..., 6:7]
    with np.errstate(invalid="ignore", divide="ignore"):
        n = np.sqrt((v * v).sum(-1, keepdims=True))
        tiny = n * n < 1e-10 * w * w
        sn = np.where(tiny | (n == 0), 1.0, n)
        sw = np.where(w == 0, 1.0, w)
        f = np.where(w == 0, np.pi / sn, np.where(tiny, 2 / sw - (2 / 3) * n * n / sw ** 3, 2 * np.arctan(n / sw) / sn))
        phi = f * v
        th2 = (phi * phi).sum(-1, keepdims=True)
        th = np.sqrt(th2)
        small = th2 < SERIES
        sth2 = np.where(small, 1.0, th2)
        c = np.where(small, 1 / 12 + th2 / 720 + th2 ** 2 / 30240 + th2 ** 3 / 1209600,
                     (1 - 0.5 * th * np.abs(w) / sn) / sth2)
        u = np.cross(phi, t)
        tau = t - 0.5 * u + c * np.cross(phi, u)
    return np.concatenate([tau, phi], -1)


def brackets(tstamp, N, query):
    """(k0, k1) int64: k0 = max(#{k < N : tstamp[k] <= t} - 1, 0), k1 = k0 + 1 if k0 < N - 1 else k0.  The comparison
    is the reference's: a float32 stamp against the float32 query; NaN on either side is not counted."""
    ts = np.asarray(tstamp, dtype=np.float32)[:N]
    q = np.asarray(query, dtype=np.float32).reshape(-1)
    with np.errstate(invalid="ignore"):
        k0 = np.array([max(int((ts <= t).sum()) - 1, 0) for t in q], dtype=np.int64).reshape(-1)
    k1 = np.where(k0 < N - 1, k0 + 1, k0)
    return k0, k1


def interpolate(poses, tstamp, N, query):
    """trajectory_filler.py:44-58 in float64: returns (Gs [M,7], k0, k1).  For k1 == k0 the relative pose is the exact
    identity (not P P^-1 with its 1e-16 of rounding), so the result is P[k0] exactly."""
    Ps = _f64(np.asarray(poses, dtype=np.float32))[:N]
    ts = _f64(np.asarray(tstamp, dtype=np.float32))[:N]
    tt = _f64(np.asarray(query, dtype=np.float32).reshape(-1))
    t0, t1 = brackets(tstamp, N, query)
    dt = ts[t1] - ts[t0] + 1e-3
    dP = mul(Ps[t1], inv(Ps[t0]))
    v = np.where((t1 == t0)[:, None], 0.0, log(dP)) / dt[:, None]
    w = v * (tt - ts[t0])[:, None]
    Gs = mul(exp(w), Ps[t0])
    return Gs, t0, t1
