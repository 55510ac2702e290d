"""numpy float64 restatement of the contract of droid_point_cloud (include/droid_backends_hip.h, "point cloud"): the
yardstick of tests/test_gpu_point_cloud.py, itself pinned by tests/test_point_cloud_ref.py against the stock lines of
the viewers written independently.  A test helper; nothing here is rounded except the colours, which are float32 by
contract.

Per selection b with i = index[b]; i outside [0, nbuf) yields no point and an all-zero matrix.  Otherwise
  1. G = inv(poses[i]) (tests/se3_ref.py: fp64 from the float32 record, the quaternion as it is); matrices[b] = matrix(G)
  2. count = depth_filter's count of frame i against its six temporal neighbours inside [0, nbuf), poses as stored,
     thresh[b] (oracle.geom.depth_filter)
  3. mean = sum(disps[i]) / (h w) in fp64
  4. keep pixel k iff count[k] >= min_count and disps[i][k] > disp_ratio * mean
  5. point = G (X0 / d), X0 = ((u - cx) / fx, (v - cy) / fy, 1), d = disps[i][k]
  6. colour = float32(images[i, c, 8v+3, 8u+3]) / float32(255) for c = 2, 1, 0
Rows in the order of index, row-major within a frame; src = v w + u; offsets[b] : offsets[b+1] are the rows of b.

Undecided pixels.  A float32 count may differ from the fp64 one only at the (pixel, neighbour) decisions inside the band
of oracle.geom.depth_filter(margins=True); the device's fp64 mean differs from numpy's by the order of the sum.  A pixel
is undecided when the disparity rule holds and its count +- its band decisions straddles min_count, or when
|d - ratio * mean| <= 2^-40 mean.  Everywhere else the keep decision is the reference's."""
import numpy as np

import se3_ref
from oracle import geom


def dense_points(poses, disps, K, frames):
    """G (X0 / d) for every pixel of the frames `frames` (inside the buffer): [len(frames), h, w, 3] float64, and the
    scale S = 8 ((|X0x| + |X0y| + 1) / |d| + |t|_1) of the error bound, t the translation of G."""
    poses = np.asarray(poses, np.float32).astype(np.float64)
    d = np.asarray(disps, np.float32).astype(np.float64)[frames]
    fx, fy, cx, cy = np.asarray(K, np.float32).astype(np.float64)
    h, w = d.shape[1:]
    v, u = np.meshgrid(np.arange(h, dtype=np.float64), np.arange(w, dtype=np.float64), indexing="ij")
    X0 = np.stack([(u - cx) / fx, (v - cy) / fy, np.ones((h, w))], -1)
    G = se3_ref.inv(poses[frames])
    with np.errstate(divide="ignore", invalid="ignore"):
        X = X0[None] / d[..., None]
        pts = se3_ref.rotate(G[:, None, None, 3:], X) + G[:, None, None, :3]
        S = 8.0 * ((np.abs(X0[..., 0]) + np.abs(X0[..., 1]) + 1.0)[None] / np.abs(d) + np.abs(G[:, :3]).sum(-1)[:, None, None])
    return pts, S


def point_cloud(poses, disps, K, index, thresh, images=None, min_count=2, disp_ratio=0.5):
    """The contract above.  Returns a dict: points [P,3] float64, colors [P,3] float32 or None, src [P] int64,
    offsets [n+1] int64, matrices [n,4,4] float64, and per selection (dense, for the tests): valid [n] bool,
    keep / undecided [n,h,w] bool, count [n,h,w], dense [n,h,w,3] (points of every pixel), S [n,h,w]."""
    poses32 = np.asarray(poses, np.float32)
    disps32 = np.asarray(disps, np.float32)
    index = np.asarray(index, np.int64)
    n = len(index)
    nbuf, h, w = disps32.shape
    nbuf = min(nbuf, len(poses32))
    thresh = np.broadcast_to(np.asarray(thresh, np.float32), (n,))
    valid = (index >= 0) & (index < nbuf)
    frames = np.where(valid, index, 0)
    d = disps32.astype(np.float64)
    count, band = geom.depth_filter(poses32, disps32, np.asarray(K, np.float32), index, thresh, margins=True)
    nband = band().sum(axis=1)
    mean = d[frames].sum(axis=(1, 2)) / float(h * w)
    lim = disp_ratio * mean[:, None, None]
    rule = d[frames] > lim
    keep = valid[:, None, None] & (count >= min_count) & rule
    straddle = (count >= min_count) != (np.where(count >= min_count, count - nband, count + nband) >= min_count)
    undecided = valid[:, None, None] & ((rule & straddle) | (np.abs(d[frames] - lim) <= 2.0 ** -40 * np.abs(mean)[:, None, None]))
    dense, S = dense_points(poses32, disps32, K, frames)
    matrices = se3_ref.matrix(se3_ref.inv(poses32[frames])) * valid[:, None, None]
    flat = keep.reshape(n, -1)
    offsets = np.concatenate([[0], np.cumsum(flat.sum(1))]).astype(np.int64)
    sel, src = np.nonzero(flat)
    points = dense.reshape(n, -1, 3)[sel, src]
    colors = None
    if images is not None:
        rgb = np.asarray(images, np.uint8)[:, [2, 1, 0], 3::8, 3::8].transpose(0, 2, 3, 1).astype(np.float32) / np.float32(255.0)
        colors = rgb[frames].reshape(n, -1, 3)[sel, src]
    return dict(points=points, colors=colors, src=src, offsets=offsets, matrices=matrices, valid=valid, keep=keep,
                undecided=undecided, count=count, nband=nband, rule=rule, dense=dense, S=S, mean=mean)
