"""Inputs of the fixtures tests/golden/reference_*.npz: what the reference's own Python programs were run on
(tests/golden/make_reference_golden.py).  Everything here is rebuilt from seeds -- droid_backends.synth and the case
builders of the other suites -- and nothing needs the reference: the fixtures hold its outputs and a SHA-256 of the
float32 inputs below, which the tests assert before they compare anything.  All tiny: a fixture is at most as large as
the largest one committed before (ba_golden.npz), so large outputs are kept at seeded samples (see each case)."""
import functools
import hashlib
import os

import numpy as np

import cvx_upsample_ref as cu
import geom_cases as gc
import hard_scenes as hs
import stage_graphs as sg
from droid_backends import synth

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
FILES = ("geom", "ba", "ba_blocks", "corr", "upsample")
MAX_BYTES = 372339          # tests/golden/ba_golden.npz, the largest fixture before these


def path(name):
    return os.path.join(GOLDEN, f"reference_{name}.npz")


def digest(*arrays):
    """SHA-256 over dtype, shape and bytes of every array, in order"""
    h = hashlib.sha256()
    for a in arrays:
        a = np.ascontiguousarray(a)
        h.update(f"{a.dtype.str}{a.shape}".encode())
        h.update(a.tobytes())
    return h.hexdigest()


def unit_poses(poses):
    """float32 records widened to float64, their quaternions normalised there.  What the reference's programs are given:
    a float32 quaternion is off the unit sphere by up to 6e-8, and there the group operations are not one thing -- the
    stand-in composes the relative pose as lietorch's operators do, t_j - R(q_j) R(q_i)^T t_i, the CUDA path as
    t_j - R(q_j q_i^-1) t_i (droid_kernels.cu:96-107), equal only on the sphere -- and lietorch itself is not here to say.
    On the sphere the oracle and the reference agree to 1e-15; off it by 5e-10 .. 8e-9 in H and 3e-9 .. 1e-7 in b
    (profiles/reference_pin.txt)."""
    p = np.array(poses, np.float64)
    p[..., 3:] /= np.linalg.norm(p[..., 3:], axis=-1, keepdims=True)
    return p


def on_the_sphere(p):
    """a copy of BAProblem `p` with unit_poses: what the reference saw"""
    import copy
    q = copy.copy(p)
    q.poses = unit_poses(p.poses)
    return q


def load(name):
    with np.load(path(name), allow_pickle=False) as z:
        return {k: z[k] for k in z.files}


# ---- projection ------------------------------------------------------------------------------------------------------
HARD_SCENE = "win9x19-rot20-plain"     # anisotropic intrinsics, 20 degree poses, live points behind MIN_DEPTH
JAC_SAMPLES = 48                       # (edge, pixel) pairs whose Jacobians the fixture keeps


def mono():
    return synth.make_ba_problem(N=8, E=32, H=8, W=16, seed=0)


@functools.lru_cache(maxsize=None)
def geom_cases():
    """name -> dict(poses [n,7], disps [n,H,W], K [4] or [n,4], ii, jj), float32 / int64.
    mono: the graph of the first BA fixture; frameK: per-frame anisotropic intrinsics; hard: a scene of
    tests/hard_scenes.py; stereo: four edges ii == jj first (coords and valid only: the fixed baseline)."""
    out = {}
    p = mono()
    out["mono"] = dict(poses=p.poses, disps=p.disps, K=p.intrinsics, ii=p.ii, jj=p.jj)
    p = synth.make_ba_problem(N=5, E=14, H=7, W=11, seed=41)
    out["frameK"] = dict(poses=p.poses, disps=p.disps, K=gc.aniso_K_frames(7, 11, 5), ii=p.ii, jj=p.jj)
    p = hs.SCENES[HARD_SCENE].problem()
    out["hard"] = dict(poses=p.poses, disps=p.disps, K=p.intrinsics, ii=p.ii, jj=p.jj)
    p = synth.make_ba_problem(N=4, E=12, H=6, W=10, stereo=True, seed=43)
    out["stereo"] = dict(poses=p.poses, disps=p.disps, K=p.intrinsics, ii=p.ii, jj=p.jj)
    for c in out.values():
        for k in ("poses", "disps", "K"):
            c[k] = np.ascontiguousarray(c[k], np.float32)
        for k in ("ii", "jj"):
            c[k] = np.ascontiguousarray(c[k], np.int64)
    return out


def geom_digest(c):
    return digest(c["poses"], c["disps"], c["K"], c["ii"], c["jj"])


def jac_sample(name, E, HW):
    """flat (edge * HW + pixel) indices of the Jacobians kept for case `name`, sorted"""
    rng = np.random.default_rng(sum(map(ord, name)))
    return np.sort(rng.choice(E * HW, size=min(JAC_SAMPLES, E * HW), replace=False)).astype(np.int64)


# ---- bundle adjustment -----------------------------------------------------------------------------------------------
def _band24():
    p = sg.variant(synth, "rgbd")
    p.disps_sens = np.zeros_like(p.disps_sens)      # geom/ba.py has no sensor-depth term
    return p


def _mono_aniso():
    """the mono graph seen through intrinsics with fx, fy, cx, cy pairwise different (the generator's are all W / 2):
    the targets stay, so the residuals are large, which the linear system does not mind"""
    p = mono()
    p.intrinsics = gc.aniso_K(*p.disps.shape[1:])
    return p


# name -> (builder, family of util.STAGE_BARS, motion-only, name in stage_graphs.GRAPHS or None)
BA_GRAPHS = {
    "mono": (mono, "sparse", False, None),
    "mono_anisoK": (_mono_aniso, "sparse", False, None),
    "window_t0_3": (lambda: synth.make_ba_problem(N=9, E=40, H=4, W=8, seed=3, t0=3), "sparse", False, None),
    "band24": (_band24, "dense", False, "variant_rgbd"),
    "motion_only": (lambda: sg.motion_only(synth), "motion", True, "motion_only"),
    "dense30_block_pair": (lambda: sg.GRAPHS["dense30_block_pair"][0](synth), "dense", False, "dense30_block_pair"),
    "dense20_few_stages": (lambda: sg.GRAPHS["dense20_few_stages"][0](synth), "dense", False, "dense20_few_stages"),
}
EDGE_BLOCKS = ("mono", "motion_only")          # graphs whose per-edge blocks the fixture keeps
FULL_BLOCKS = ("mono", "window_t0_3")          # graphs whose H, E, C, v, w it keeps (reference_ba_blocks.npz)


@functools.lru_cache(maxsize=None)
def ba_problem(name):
    """The BAProblem of graph `name`, checked against what geom/ba.py can express: no sensor depths, the window ends
    with the buffer, and (full BA) every window frame is the source of an edge, so that unique(ii) are the depth slots."""
    build, _, motion_only, _ = BA_GRAPHS[name]
    p = build()
    assert not p.disps_sens.any() and p.t1 == p.disps.shape[0], name
    assert (p.ii != p.jj).all(), name
    if not motion_only:
        assert set(range(p.t0, p.t1)) <= set(p.ii.tolist()), name
        assert (p.ii == p.t0).any(), name                       # the first window pose has rows in E
        assert p.eta.shape[0] == len(np.unique(p.ii)), name
    return p


def ba_digest(p):
    return digest(p.poses, p.disps, p.intrinsics, p.targets, p.weights, p.eta, p.ii, p.jj,
                  np.array([p.t0, p.t1], np.int64))


def tril_pack(A):
    return A[np.tril_indices(A.shape[0])]


def tril_unpack(v, n):
    """the symmetric matrix whose lower triangle `tril_pack` packed"""
    A = np.zeros((n, n), v.dtype)
    A[np.tril_indices(n)] = v
    return A + np.tril(A, -1).T


def cuda_rules(blk, name, p, damp_schur=True, drop_first=True):
    """dx [6P], dz [M HW] and the damped matrix from the reference's H, E, C, v, w, the way src/droid_kernels.cu solves:
    the damping ep + lm diag on the diagonal of the REDUCED matrix (dk:1192-1213; geom/chol.py:56 damps H before the
    Schur complement), and the first window pose left out of the back-substitution (dk:1105 `idx <= 0`; chol.py:69
    includes it).  lm, ep rounded to float32 like the arguments of the C ABI (util.damped_solve)."""
    n = 6 * (p.t1 - p.t0)
    H = tril_unpack(blk[f"{name}_H"], n)
    E, C, v, w = (blk[f"{name}_{k}"] for k in ("E", "C", "v", "w"))
    lm, ep = float(np.float32(p.lm)), float(np.float32(p.ep))
    Q = 1.0 / C
    EQ = E * Q
    if damp_schur:
        A = H - EQ @ E.T
        A[np.diag_indices(n)] += ep + lm * np.diag(A)
    else:
        A = H.copy()
        A[np.diag_indices(n)] += ep + lm * np.diag(A)
        A -= EQ @ E.T
    dx = np.linalg.solve(A, v - EQ @ w)
    Eb = E.copy()
    if drop_first:
        Eb[:6] = 0.0
    return dx, Q * (w - Eb.T @ dx), A


# ---- correlation -----------------------------------------------------------------------------------------------------
CORR_SHAPE = dict(nbuf=3, C=32, h=16, w=24, levels=4)
CORR_EDGES = (np.array([0, 2], np.int64), np.array([1, 0], np.int64))
CORR_ROWS = 12                          # source pixels of the all-pairs volume the fixture keeps, per edge
ALT_FRAMES = np.array([0, 2])           # frames of the feature pyramid it keeps


@functools.lru_cache(maxsize=None)
def corr_fmaps():
    """[3, 32, 16, 24] N(0, 1) generated as half: the fp32 and the f16 path read the same values"""
    s = CORR_SHAPE
    f = np.random.default_rng(2024).normal(0, 1, (s["nbuf"], s["C"], s["h"], s["w"])).astype(np.float16)
    f.setflags(write=False)
    return f


def corr_rows():
    """source pixels (y * w + x) kept: the four corners and seeded others, sorted"""
    s = CORR_SHAPE
    hw = s["h"] * s["w"]
    corners = [0, s["w"] - 1, hw - s["w"], hw - 1]
    rest = np.random.default_rng(7).choice(np.setdiff1d(np.arange(hw), corners), CORR_ROWS - 4, replace=False)
    return np.sort(np.concatenate([corners, rest])).astype(np.int64)


# ---- convex upsampling -----------------------------------------------------------------------------------------------
UP_SAMPLES = 1536                       # output pixels kept per (case, sigma) where the case has more


def up_cases():
    return [(c, s) for c in range(len(cu.CASES)) for s in cu.SIGMAS]


def up_sample(case, sigma):
    """flat indices into [n, 8H, 8W] of the output pixels kept, sorted: all of them, or a seeded UP_SAMPLES"""
    n, H, W = cu.CASES[case]
    total = n * 64 * H * W
    if total <= UP_SAMPLES:
        return np.arange(total, dtype=np.int64)
    rng = np.random.default_rng(500 + 10 * case + int(sigma))
    return np.sort(rng.choice(total, UP_SAMPLES, replace=False)).astype(np.int64)


def up_key(case, sigma):
    return f"c{case}_s{int(sigma)}"
