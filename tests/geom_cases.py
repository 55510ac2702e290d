"""Inputs of the geometry parity tests (tests/test_gpu_geom.py) and the rule they are judged by.  Plain helpers, no
fixtures: tests/test_geom_cases.py proves on the CPU, from the fp64 reference alone, that every case generated here
exercises what it claims to and stays inside the cap of the band rule; the GPU tests then run the same cases.

The band rule.  A float32 kernel may take a DECISION (valid flag, clamp branch, 1000 flag, one count) differently
from the fp64 reference only at pixels where the reference's own quantity lies within the float32 rounding of the
threshold: for a depth test |Z - threshold| <= 64 * 2^-24 * (|X0| + |X1| + 1 + |d| ||t||_1), the 64 counted from the
operations of transform_pixel (oracle/geom.py, Z_BAND_C).  Outside the band decisions are identical and values meet
the value tolerance.  The cap is a condition on the case: at most max(2, 2e-4 * pixels) of its pixels lie in a band.
"""
import numpy as np

from droid_backends import synth
from oracle import geom

SHAPES = [(1, 1), (1, 64), (9, 19), (17, 24), (30, 40), (31, 41), (48, 64), (96, 128)]
ROT_DEG = (1.0, 20.0, 60.0)
VARIANTS = ("negated", "nonunit", "shifted")
ANISO = "anisoK"          # plain poses, intrinsics with fx, fy, cx, cy pairwise different (every other case: fx == fy == cx)
PUSH = -3.0
BETAS = (0.0, 0.3, 1.0)
# depth thresholds: projmap's fall-back, reproject's depth-1 substitution, reproject's valid, projmap / frame_distance valid
Z_PROJMAP = (geom.PROJMAP_CLAMP, geom.KERNEL_MIN_DEPTH)
Z_REPROJECT = (0.5 * geom.MIN_DEPTH, geom.MIN_DEPTH)


def cap(pixels):
    return max(2, int(2e-4 * pixels))


def aniso_K(H, W):
    """fx, fy, cx, cy pairwise at least 10 % apart (of the larger) at every shape of the suites, none centred: a kernel
    that reads one for another is wrong by that much."""
    return np.array([0.9 * W, 0.62 * W, 0.38 * W + 0.5, 0.36 * H - 0.75], np.float32)


def aniso_K_frames(H, W, n):
    """per-frame intrinsics, each anisotropic, no frame a common multiple of another"""
    f = np.arange(n)
    s = np.stack([1.0 + 0.03 * (f % 5), 1.0 - 0.02 * (f % 3), 1.0 + 0.015 * (f % 4), 1.0 - 0.025 * (f % 7)], axis=1)
    return (aniso_K(H, W)[None].astype(np.float64) * s).astype(np.float32)


def wild_poses(prob, rng, rot_deg, push, variant="plain", push_frame=3):
    """Poses of `prob` with a random se3_exp (rotation sigma rot_deg, translation sigma 0.3) composed onto every one
    and frame `push_frame` moved by `push` along z, so that a share of the points ends behind or close to the camera.
    variant: "negated" every second quaternion * -1 (the same rotations), "nonunit" every third quaternion scaled by
    1.001 or 0.999, "shifted" the whole trajectory moved by (100, -40, 60)."""
    poses = np.asarray(prob.poses, np.float64).copy()
    n = poses.shape[0]
    xi = np.concatenate([rng.normal(0, 0.3, (n, 3)), rng.normal(0, np.deg2rad(rot_deg), (n, 3))], axis=1)
    dt, dq = synth.se3_exp(xi)
    t, q = synth.se3_mul(dt, dq, poses[:, :3], poses[:, 3:])
    q = q / np.linalg.norm(q, axis=-1, keepdims=True)
    t[push_frame % n, 2] += push
    if variant == "negated":
        q[1::2] *= -1.0
    elif variant == "nonunit":
        q[0::3] *= np.where(np.arange(len(q[0::3])) % 2 == 0, 1.001, 0.999)[:, None]
    elif variant == "shifted":
        # world-to-camera poses of a trajectory moved by s in the world: t' = t - R s
        t = t - synth.quat_rot(q, np.broadcast_to(np.array([100.0, -40.0, 60.0]), t.shape))
    else:
        assert variant == "plain", variant
    return np.concatenate([t, q], axis=1).astype(np.float32)


class Case:
    """One input of the geometry operators: 8 frames, 32 edges (three of them stereo edges for reproject)."""

    def __init__(self, H, W, rot_deg, variant, seed=None):
        self.H, self.W, self.rot_deg, self.variant = H, W, rot_deg, variant
        self.id = f"{H}x{W}-rot{rot_deg:g}-{variant}"
        # the variants of one (shape, rotation) share their base poses
        seed = (H * 1009 + W * 31 + int(rot_deg) * 7) if seed is None else seed
        prob = synth.make_ba_problem(N=8, E=32, H=H, W=W, seed=seed)
        rng = np.random.default_rng(seed + 1)
        self.poses = wild_poses(prob, rng, rot_deg, PUSH, "plain" if variant == ANISO else variant)
        self.disps = prob.disps
        if variant == ANISO:
            self.K, self.K_frames = aniso_K(H, W), aniso_K_frames(H, W, 8)
        else:
            self.K = prob.intrinsics.astype(np.float32)
            self.K_frames = np.stack([self.K * np.float32(1.0 + 0.01 * (f % 7)) for f in range(8)]).astype(np.float32)
        self.ii, self.jj = prob.ii, prob.jj
        st = np.array([2, 7, 4])
        self.ii_st = np.concatenate([prob.ii[:-3], st])          # reproject: the last three become stereo edges
        self.jj_st = np.concatenate([prob.jj[:-3], st])
        self.target = rng.uniform(-20.0, 1.5 * max(H, W), (32, H, W, 2)).astype(np.float32)
        self.pixels = 32 * H * W

    def twin(self):
        """The same case with the quaternion of every second frame negated: the same rotations, and the relative
        quaternion of an edge between an odd and an even frame changes sign."""
        c = Case.__new__(Case)
        c.__dict__.update(self.__dict__)
        c.poses = self.poses.copy()
        c.poses[1::2, 3:] *= np.float32(-1.0)
        return c


def all_cases():
    """Every shape at every rotation scale, and the three quaternion variants and the anisotropic intrinsics at a
    shape below one workgroup and at the 12-workgroup shape of the other suites."""
    out = [Case(H, W, r, "plain") for (H, W) in SHAPES for r in ROT_DEG]
    out += [Case(H, W, r, v) for (H, W) in ((9, 19), (48, 64)) for r in ROT_DEG for v in VARIANTS]
    out += [Case(H, W, r, ANISO) for (H, W) in ((9, 19), (48, 64)) for r in ROT_DEG]
    return out


def in_z_band(Z, mag, thresholds):
    """Pixels whose fp64 depth lies within the float32 rounding of one of `thresholds` (a nan counts as inside)."""
    band = geom.z_band(mag)
    m = np.zeros(Z.shape, bool)
    for thr in thresholds:
        m |= ~(np.abs(Z - thr) > band)
    return m


def share_margin(n_band, pixels):
    """How far from 0.75 the valid share of an edge has to be for the 1000 flag to be decided: the pixels of the
    edge inside the Z band may flip (n_band / pixels); `valid` and `total` are float32 sums, each thread adding
    2 * ceil(pixels / 256) terms, then 6 wave steps and 3 additions (relative error below (2 pixels / 256 + 11) * 2^-24
    each); beta, 1 - beta, total + 1e-8 and the quotient round once more each."""
    return n_band / pixels + (2.0 * (2.0 * pixels / 256.0 + 11.0) + 4.0) * geom.EPS32


# ---------------------------------------------------------------------------------------------------------------------
# The depth ladder: identity rotations, a pure z translation per edge, disparities chosen per pixel so that
# Z = 1 + d tz steps through LEVELS.  Every constant of the kernels (0.01, 0.1, 0.2, 0.25) is 5e-3 from its neighbours,
# about 1e5 float32 roundings: no band applies, every decision is asserted exactly.
LEVELS = np.array([0.005, 0.015, 0.095, 0.105, 0.195, 0.205, 0.245, 0.255, 0.3, 1.0])
LADDER_H, LADDER_W = 13, 21      # 273 pixels: one full workgroup and 17 threads of the next


def depth_ladder():
    """poses [6,7], disps [6,H,W], K [4], ii, jj, and level [E,H,W] = index into LEVELS of every pixel of every edge.
    Edge patterns (20 pixels long, repeated): "even" every level twice (valid share 0.3 at 0.25: flagged 1000);
    "a" 14 pixels at 0.3 / 1, two at 0.255, four lower: share 0.8 with the threshold at 0.25, 0.7 at 0.26 or above;
    "b" 14 at 0.3 / 1, two at 0.245, four lower: share 0.7 with the threshold at 0.25, 0.8 at 0.24 or below."""
    H, W = LADDER_H, LADDER_W
    tz = np.array([0.0, -1.0, -2.0, -0.5, -3.0, 1.0])            # frame f sits at z = tz[f]; frame 0 is the source
    pat = dict(even=[0, 1, 2, 3, 4, 5, 6, 7, 8, 9] * 2,
               a=[8, 9] * 7 + [7, 7, 0, 2, 4, 6],
               b=[8, 9] * 7 + [6, 6, 0, 2, 4, 5])
    edges = [(1, "even"), (2, "even"), (3, "even"), (4, "even"), (1, "a"), (2, "a"), (1, "b"), (4, "b"), (5, "even")]
    # one source frame per edge, so that each edge has disparities of its own; the targets follow
    ns = len(edges)
    all_poses = np.zeros((ns + 6, 7), np.float32)
    all_poses[:, 6] = 1.0
    all_poses[ns:, 2] = tz
    disps = np.ones((ns + 6, H, W), np.float32)
    level = np.zeros((ns, H, W), np.int64)
    k = np.arange(H * W)
    for e, (j, name) in enumerate(edges):
        lv = np.array(pat[name])[(k + 3 * e) % 20].reshape(H, W)
        if tz[j] > 0:
            lv = np.full((H, W), 9)                               # moving forward: Z = 1 + d: every pixel valid
            disps[e] = 0.5
        else:
            disps[e] = ((1.0 - LEVELS[lv]) / -tz[j]).astype(np.float32)
        level[e] = lv
    K = np.array([W / 2.0, W / 2.0, W / 2.0, H / 2.0], np.float32)
    ii = np.arange(ns, dtype=np.int64)
    jj = np.array([ns + j for j, _ in edges], dtype=np.int64)
    forward = np.array([tz[j] > 0 for j, _ in edges])
    # projmap returns the pixel itself below 0.01 (level 0) -- and, trivially, where the disparity is 0 (Z = 1)
    itself = (level == 0) | ((level == 9) & ~forward[:, None, None])
    return dict(poses=all_poses, disps=disps, K=K, ii=ii, jj=jj, level=level, forward=forward, itself=itself)


# ---------------------------------------------------------------------------------------------------------------------
# frame_distance_matrix
MATRIX_N = (1, 2, 31, 32, 33, 65)
MATRIX_SHAPES = ((9, 19), (48, 64))
MATRIX_ANISO = (33, 9, 19)       # one instance with aniso_K: two block columns of targets, the second ragged


def matrix_case(n, H, W, aniso=False):
    """n frames in use of a buffer of n + 3: wild poses at 20 degrees, one frame pushed, the spare frames filled too.
    aniso: the intrinsics of aniso_K instead of the generator's (fx == fy == cx)."""
    nbuf = n + 3
    seed = 4000 + 10 * n + H
    prob = synth.make_ba_problem(N=nbuf, H=H, W=W, seed=seed, edges=(np.arange(1, nbuf), np.arange(nbuf - 1)))
    rng = np.random.default_rng(seed + 1)
    poses = wild_poses(prob, rng, 20.0, PUSH, "plain", push_frame=min(3, n - 1))
    # a trajectory this wild overlaps nowhere: pull the frames together so that both outcomes of the 0.75 test occur
    poses[:, :3] *= np.float32(0.35)
    K = aniso_K(H, W) if aniso else prob.intrinsics.astype(np.float32)
    return dict(poses=poses, disps=prob.disps, K=K, n=n, nbuf=nbuf)


def matrix_reference(mc, chunk=128):
    """fp64 per-pair sums of the n x n pairs (oracle.geom.frame_distance margins), computed in chunks of edges, and
    the number of pixels of each pair inside the Z band of 0.25."""
    n = mc["n"]
    ii, jj = (a.reshape(-1) for a in np.meshgrid(np.arange(n), np.arange(n), indexing="ij"))
    keys = ("a_full", "a_trans", "n_full", "n_trans")
    parts = {k: np.zeros(n * n) for k in keys}
    nband = np.zeros(n * n)
    for s in range(0, n * n, chunk):
        _, m = geom.frame_distance(mc["poses"], mc["disps"], mc["K"], ii[s:s + chunk], jj[s:s + chunk], 0.5, margins=True)
        for k in keys:
            parts[k][s:s + chunk] = m[k]
        band = in_z_band(m["Z"], m["mag"], (geom.KERNEL_MIN_DEPTH,)) | in_z_band(m["Zt"], m["mag"], (geom.KERNEL_MIN_DEPTH,))
        nband[s:s + chunk] = band.sum(axis=(1, 2))
        parts["pixels"] = m["pixels"]
    return ii, jj, parts, nband


# ---------------------------------------------------------------------------------------------------------------------
# depth_filter runs on the poses of every Case with disparities of its own: smooth per-pixel maps (one low-frequency
# pattern per frame, about 20 % of variation across the map).  Neighbouring corners then differ by little, so a
# projection within rounding of an integer corner rarely stands next to a corner that decides differently, and the wild
# poses spread | 1/dj - 1/d | over several units, so few pixels sit within rounding of `thresh`: the cap holds at every
# shape (tests/test_geom_cases.py), with disparities that vary from pixel to pixel.
DF_IX = np.array([0, 1, 2, 3, 4, 5, 6, 7, 8, -1, 2 ** 32 + 3], dtype=np.int64)       # all frames, then outside the buffer
DF_THRESH = np.array([0.05, 0.1, 0.2, 0.02] * 2 + [0.1, 0.1, 0.1], dtype=np.float32)
DF_LIVE = 8


def smooth_disps(H, W, n, rng, amp=0.2):
    y, x = np.meshgrid(np.arange(H) / H, np.arange(W) / W, indexing="ij")
    out = []
    for _ in range(n):
        a, b, c, _ = rng.uniform(0, 2 * np.pi, 4)
        s = np.sin(2 * np.pi * x + a) * np.cos(np.pi * y + b) + 0.5 * np.sin(np.pi * x + 2 * np.pi * y + c)
        out.append(np.exp(amp * s + rng.normal(0, 0.15)))
    return np.array(out, np.float32)


def depth_filter_case(case):
    """Inputs of depth_filter for a Case: its poses (twin: the same with every second quaternion negated), smooth
    disparities, every frame selected -- the ends of the buffer miss neighbours -- and three indices outside it."""
    disps = smooth_disps(case.H, case.W, 8, np.random.default_rng(case.H * 7 + case.W))
    return dict(poses=case.poses, twin=case.twin().poses, disps=disps, K=case.K, ix=DF_IX, thresh=DF_THRESH, live=DF_LIVE,
                pixels=DF_LIVE * case.H * case.W)
