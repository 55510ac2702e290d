"""The case table of the pose-algebra tests (tests/test_se3_ref.py on the host, tests/test_gpu_se3.py on the device).

Rotation angles across every branch point of exp and log (theta -> 0, the series thresholds, theta -> pi), exactly
w = 0, random and axis-aligned axes, translation scales 1e-3, 1 and 100.  Every record is run as q, as -q and with q
scaled by 1 +- 1e-5 (a pose buffer that is never renormalised).  Batch sizes: the tails of a wave and of a block."""
import numpy as np

ANGLES = (0.0, 1e-9, 1e-5, 9.9e-5, 1.1e-4, 1e-3, 1e-2, 0.1, 1.0, 3.0, np.pi - 1e-3, np.pi - 1e-6)
SCALES = (1e-3, 1.0, 100.0)
QUAT_VARIANTS = (1.0, -1.0, 1.0 + 1e-5, 1.0 - 1e-5)
BATCHES = (1, 63, 64, 65, 257)


def _axes(rng):
    a = rng.normal(size=(2, 3))
    a /= np.linalg.norm(a, axis=1, keepdims=True)
    return [np.array([1.0, 0.0, 0.0]), a[0], a[1]]


def tangents(seed=0):
    """[K, 6] float32 (tau, phi): every angle x axis x translation scale."""
    rng = np.random.default_rng(seed)
    axes = _axes(rng)
    rows = [np.concatenate([s * rng.uniform(-1, 1, 3), th * ax]) for th in ANGLES for ax in axes for s in SCALES]
    return np.asarray(rows, dtype=np.float32)


def poses(seed=1):
    """[K, 7] float32 records: every angle x axis x scale x quaternion variant, then exactly w = 0 (q = (1,0,0,0) and
    a general axis whose float32 components are used as they are) x scale x variant."""
    rng = np.random.default_rng(seed)
    axes = _axes(rng)
    rows = []
    for th in ANGLES:
        for ax in axes:
            for s in SCALES:
                t = s * rng.uniform(-1, 1, 3)
                q = np.concatenate([np.sin(0.5 * th) * ax, [np.cos(0.5 * th)]])
                rows += [np.concatenate([t, c * q]) for c in QUAT_VARIANTS]
    for v in (np.array([1.0, 0.0, 0.0]), axes[1]):
        for s in SCALES:
            t = s * rng.uniform(-1, 1, 3)
            rows += [np.concatenate([t, c * v, [0.0]]) for c in QUAT_VARIANTS]
    return np.asarray(rows, dtype=np.float32)


def batches(table):
    """The whole table once, then for every batch size n of BATCHES n rows of it, starting where the last one ended."""
    yield table
    at = 0
    for n in BATCHES:
        yield table[(at + np.arange(n)) % len(table)]
        at += n


def translation_scale(*arrays):
    """S of the error bound, per row: 1 + the largest |translation component| among the given [n, >= 3] arrays (the
    first three columns of records and tangents; pass the fourth column of matrices as [n, 3])."""
    return 1.0 + np.max([np.abs(np.asarray(a, dtype=np.float64)[..., :3]).max(-1) for a in arrays], axis=0)


def trajectory(N, seed, step_rot=0.05, step_trans=0.1, t_scale=1.0):
    """[N, 7] float32 keyframe poses: a random walk whose steps rotate by at most step_rot * sqrt(3) rad, so that the
    relative rotation of every bracket stays far below 3 rad."""
    import se3_ref
    rng = np.random.default_rng(seed)
    P = np.zeros((N, 7))
    P[0] = np.concatenate([t_scale * rng.uniform(-1, 1, 3), [0, 0, 0, 1]])
    xi = np.concatenate([step_trans * rng.uniform(-1, 1, (N, 3)), step_rot * rng.uniform(-1, 1, (N, 3))], 1)
    for k in range(1, N):
        P[k] = se3_ref.mul(se3_ref.exp(xi[k]), P[k - 1])
    return P.astype(np.float32)


FILLER_STAMPS = (0.0, 4.0, 4.0, 9.0, 15.0)
FILLER_QUERIES = (-1.0, 0.0, 2.0, 4.0, 8.999, 9.0, 15.0, 20.0)
FILLER_BRACKETS = ((0, 1), (0, 1), (0, 1), (2, 3), (2, 3), (3, 4), (4, 4), (4, 4))
