"""Inputs of the point-cloud tests (tests/test_gpu_point_cloud.py) and the cap they are judged by.  Plain helpers;
tests/test_point_cloud_cases.py proves on the CPU, from the fp64 reference alone, that every case does what it claims.

The wild poses of tests/geom_cases.py are useless here: few of their neighbours agree, almost nothing is kept and the
disparity rule never fires.  This is a two-plane scene whose depths are consistent across the frames by construction:
the world plane n.X = c seen from the world-to-camera pose (t, q) has the depth Z = (c + (R n).t) / ((R n).ray) along
the pixel's ray.  A near plane (c = 3) fills the view except where the far plane's (c = 9) intersection lies beyond a
world x: those pixels fail the disparity rule, the others pass it.  Then the depths are perturbed so that every count
0 .. 6 occurs: a band of rows of frame 2 (x 1.35), the left half of that band in frame 5 (x 0.7), and the left columns
of every frame by a per-pixel draw from {1, 1, 1.25, 0.8}."""
import numpy as np

import geom_cases
from droid_backends import synth

NBUF = 9
PLANE_N = np.array([0.15, -0.1, 1.0])
C_NEAR, C_FAR = 3.0, 9.0
# unsorted, a duplicate (3), both ends of the buffer, three entries outside it (2^32 + 3 is not frame 3)
INDEX = np.array([5, 0, 8, 3, 3, -1, 2, 9, 2 ** 32 + 3, 6, 1, 4, 7], dtype=np.int64)
LIVE = 10
#         H   W   K        thresh
TABLE = [(8, 8, "iso", 0.1), (9, 19, "iso", 0.1), (17, 24, "aniso", 0.1), (31, 41, "iso", 0.05), (48, 64, "aniso", 0.1),
         (48, 64, "iso", 0.02)]
MIN_COUNT, DISP_RATIO = 2, 0.5


def cap(live_pixels):
    """Most undecided pixels a case may have: about 4x what the reference alone needs on these inputs."""
    return max(2, int(1e-3 * live_pixels))


def iso_K(H, W):
    return np.array([W, W, W / 2 - 0.5, H / 2 - 0.5], np.float32)


def plane_depth(pose, K, H, W, c):
    """Depth along every pixel's ray of the plane n.X = c seen from the float32 pose, and the world points hit."""
    t, q = pose[:3].astype(np.float64), pose[3:].astype(np.float64)
    fx, fy, cx, cy = K.astype(np.float64)
    v, u = np.meshgrid(np.arange(H, dtype=np.float64), np.arange(W, dtype=np.float64), indexing="ij")
    ray = np.stack([(u - cx) / fx, (v - cy) / fy, np.ones((H, W))], -1)
    Rn = synth.quat_rot(q, PLANE_N)
    Z = (c + Rn @ t) / (ray @ Rn)
    world = synth.quat_rot(synth.quat_inv(q), Z[..., None] * ray - t)
    return Z, world


class Case:
    def __init__(self, H, W, kind, thresh):
        self.H, self.W, self.kind, self.thresh = H, W, kind, float(thresh)
        self.id = f"{H}x{W}-{kind}-t{thresh:g}"
        rng = np.random.default_rng(H * 1009 + W * 31 + (7 if kind == "aniso" else 0))
        self.K = geom_cases.aniso_K(H, W) if kind == "aniso" else iso_K(H, W)
        xi = 0.5 * np.cumsum(np.concatenate([rng.normal(0, 0.08, (NBUF, 3)), rng.normal(0, np.deg2rad(3.0), (NBUF, 3))], 1), 0)
        t, q = synth.se3_exp(xi)
        q = q / np.linalg.norm(q, axis=-1, keepdims=True)
        self.poses = np.concatenate([t, q], 1).astype(np.float32)
        x_far = 0.45 * C_FAR * (W / 2) / float(self.K[0]) * 0.6
        disps = np.zeros((NBUF, H, W))
        for f in range(NBUF):
            Zn, _ = plane_depth(self.poses[f], self.K, H, W, C_NEAR)
            Zf, world = plane_depth(self.poses[f], self.K, H, W, C_FAR)
            disps[f] = 1.0 / np.where(world[..., 0] > x_far, Zf, Zn)
        r0, r1 = H // 3, H // 3 + max(1, H // 4)
        disps[2, r0:r1] *= 1.35
        disps[5, r0:r1, :W // 2] *= 0.7
        cols = max(1, W // 6)
        disps[:, :, :cols] *= rng.choice(np.array([1.0, 1.0, 1.25, 0.8]), (NBUF, H, cols))
        self.disps = disps.astype(np.float32)
        self.images = rng.integers(0, 256, (NBUF, 3, 8 * H, 8 * W), dtype=np.uint8)
        self.index = INDEX
        self.live_pixels = LIVE * H * W


def all_cases():
    return [Case(*row) for row in TABLE]
