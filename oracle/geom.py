"""TEST INFRASTRUCTURE ONLY (see oracle/__init__.py): numpy fp64 restatement of the Python-side reprojection and
motion features of the update step, and of the geometry operators of src/droid_kernels.cu together with the
quantity each of their DECISIONS is taken on.  `reproject` is pinned to outputs of the reference's own
projective_transform (tests/test_reference_pin.py, over a stand-in for lietorch, which itself stays unpinned); the
operators of src/droid_kernels.cu only by closed-form cases and by the C restatement (tests/test_oracle_geom.py).

  reproject            droid_slam/depth_video.py:150-158 -> droid_slam/geom/projective_ops.py:96-125
  iproj / actp / proj  droid_slam/geom/projective_ops.py:18-37, :75-93 (X1 = Gij * X0), :39-51
  motion features      droid_slam/factor_graph.py:203-205
  projmap, frame_distance, iproj_points, depth_filter   src/droid_kernels.cu:427-850

Margins.  A float32 evaluation of one of these operators may take a decision (valid flag, clamp branch, 1000 flag,
one count) differently from this file only where the quantity the decision is taken on lies within the float32
rounding of its threshold.  The functions below return that quantity next to the result (`margins=True`):
Z for every depth test, the valid share for frame_distance, | |1/dj - 1/d| - thresh | and the distance of (uj, vj)
from the integer grid for depth_filter, together with `mag`, the magnitude the roundings of the transformed point
scale with (see `z_band`).
"""
import numpy as np

MIN_DEPTH = 0.2            # projective_ops.py:6 (Python side: reproject)
KERNEL_MIN_DEPTH = 0.25    # droid_kernels.cu:26 (projmap valid, frame_distance)
PROJMAP_CLAMP = 0.01       # droid_kernels.cu:497: below it projmap returns the pixel itself
EPS32 = 2.0 ** -24         # unit roundoff of float32

# Roundings on the way to one component of the transformed point Xj = R(q) X0 + d t in float32 (the operation order
# of actSO3, droid_kernels.cu:58-68, and actSE3):
#    4   X0 = (u - cx) / fx, X1 = (v - cy) / fy           a subtraction and a division each
#    9   uv = 2 (qv x X)                                   two products and a difference per component
#    6   X + w uv + (qv x uv)                              w uv, its sum, two products, their difference, the sum
#    2   + d t                                             product and sum
#    9   q (4 components, each entering twice) and t (1) of the relative pose, rounded to float32 once
# = 30 roundings, each of a term no larger than 2 |q|^2 (|X0| + |X1| + 1) or |d| |t| -- the factor 2 is the one in
# uv -- so |dXj| <= 60 * 2^-24 * mag with mag = |X0| + |X1| + 1 + |d| ||t||_1; 64 leaves room for |q| = 1.001.
Z_BAND_C = 64


def z_band(mag, c=Z_BAND_C):
    """Half-width of the band around a depth threshold inside which a float32 evaluation may decide differently."""
    return c * EPS32 * mag


def coord_scale(f, c0, X, Z, mag):
    """What the float32 error of a projected coordinate f * X / Z + c0 scales with: the error of X and of Z
    (`z_band`) through the quotient, plus the roundings of the quotient, the product and the sum.  With it
    |d coord| <= Z_BAND_C * 2^-24 * coord_scale."""
    with np.errstate(divide="ignore", invalid="ignore"):
        r = 1.0 / np.abs(Z)
        return np.abs(f) * mag * r * (1.0 + np.abs(X) * r) + np.abs(f * X * r + c0) + np.abs(c0)


def _quat_rot(q, X):
    """rotate X [...,3] by unit quaternion q = (x, y, z, w) [...,4]"""
    qv, w = q[..., :3], q[..., 3:4]
    uv = 2.0 * np.cross(qv, X)
    return X + w * uv + np.cross(qv, uv)


def _relative(poses, ii, jj, stereo=True):
    """Gij = Gj * Gi^-1 (projective_ops.py:102) as (t, q); stereo edges get the fixed baseline (:105) unless
    `stereo` is False (relSE3 of droid_kernels.cu:96-107, used by projmap / frame_distance / depth_filter)."""
    ti, qi = poses[ii, :3], poses[ii, 3:]
    tj, qj = poses[jj, :3], poses[jj, 3:]
    qi_inv = qi * np.array([-1.0, -1.0, -1.0, 1.0])
    # q = qj * qi^-1 (Hamilton product, (x, y, z, w) layout)
    a, b = qj, qi_inv
    q = np.stack([a[:, 3] * b[:, 0] + a[:, 0] * b[:, 3] + a[:, 1] * b[:, 2] - a[:, 2] * b[:, 1],
                  a[:, 3] * b[:, 1] - a[:, 0] * b[:, 2] + a[:, 1] * b[:, 3] + a[:, 2] * b[:, 0],
                  a[:, 3] * b[:, 2] + a[:, 0] * b[:, 1] - a[:, 1] * b[:, 0] + a[:, 2] * b[:, 3],
                  a[:, 3] * b[:, 3] - a[:, 0] * b[:, 0] - a[:, 1] * b[:, 1] - a[:, 2] * b[:, 2]], axis=-1)
    t = tj - _quat_rot(q, ti)
    if stereo:
        st = ii == jj
        t[st] = np.array([-0.1, 0.0, 0.0])
        q[st] = np.array([0.0, 0.0, 0.0, 1.0])
    return t, q


def _inputs(poses, disps, intrinsics):
    poses = np.asarray(poses, np.float64)
    disps = np.asarray(disps, np.float64)
    K = np.asarray(intrinsics, np.float64)
    if K.ndim == 1:
        K = np.broadcast_to(K, (disps.shape[0], 4))
    return poses, disps, K


def _grid(H, W):
    y, x = np.meshgrid(np.arange(H, dtype=np.float64), np.arange(W, dtype=np.float64), indexing="ij")
    return x, y


def transform(poses, disps, intrinsics, ii, jj, stereo=True):
    """Pixels of frames ii, back-projected with their intrinsics and moved into frames jj: X0 [E,H,W,3] (depth 1),
    X1 = Gij * (X0, disp) [E,H,W,3], the relative translations t [E,3] and mag [E,H,W] (see `z_band`)."""
    poses, disps, K = _inputs(poses, disps, intrinsics)
    ii, jj = np.asarray(ii, np.int64), np.asarray(jj, np.int64)
    H, W = disps.shape[1:]
    x, y = _grid(H, W)
    Ki = K[ii][:, None, None, :]
    X0 = np.stack([(x[None] - Ki[..., 2]) / Ki[..., 0], (y[None] - Ki[..., 3]) / Ki[..., 1],
                   np.ones((len(ii), H, W))], axis=-1)                       # :27-30 (pts[..., :3]; pts[..., 3] = disp)
    d0 = disps[ii]
    t, q = _relative(poses, ii, jj, stereo)
    X1 = _quat_rot(q[:, None, None, :], X0) + t[:, None, None, :] * d0[..., None]   # SE3 acting on a homogeneous point
    mag = np.abs(X0[..., 0]) + np.abs(X0[..., 1]) + 1.0 + np.abs(d0) * np.abs(t).sum(axis=-1)[:, None, None]
    return X0, X1, t, mag


def reproject(poses, disps, intrinsics, ii, jj, margins=False):
    """coords [E,H,W,2], valid [E,H,W,1] (float64).  intrinsics [nbuf,4] or [4].  With `margins` a third value:
    Z (compared with 0.5 * MIN_DEPTH for the depth-1 substitution and with MIN_DEPTH for valid), X1, mag."""
    _, _, K = _inputs(poses, disps, intrinsics)
    jj = np.asarray(jj, np.int64)
    X0, X1, _, mag = transform(poses, disps, intrinsics, ii, jj)
    Kj = K[jj][:, None, None, :]
    Z = X1[..., 2]
    Zc = np.where(Z < 0.5 * MIN_DEPTH, 1.0, Z)                               # :46
    d = 1.0 / Zc
    coords = np.stack([Kj[..., 0] * (X1[..., 0] * d) + Kj[..., 2], Kj[..., 1] * (X1[..., 1] * d) + Kj[..., 3]], axis=-1)
    valid = ((Z > MIN_DEPTH) & (X0[..., 2] > MIN_DEPTH)).astype(np.float64)[..., None]   # :113
    if margins:
        return coords, valid, dict(Z=Z, Zc=Zc, X=X1, mag=mag, Kj=Kj)
    return coords, valid


def motion_features(poses, disps, intrinsics, ii, jj, target):
    """motn [E,4,H,W] = clamp(cat(coords1 - coords0, target - coords1), -64, 64) (factor_graph.py:203-205)."""
    coords, valid = reproject(poses, disps, intrinsics, ii, jj)
    H, W = coords.shape[1:3]
    x, y = _grid(H, W)
    coords0 = np.stack([x, y], axis=-1)
    motn = np.concatenate([coords - coords0[None], np.asarray(target, np.float64) - coords], axis=-1)
    return np.clip(motn.transpose(0, 3, 1, 2), -64.0, 64.0), coords, valid


def projmap(poses, disps, intrinsics, ii, jj, margins=False):
    """projmap_kernel droid_kernels.cu:427-516: coords [E,H,W,3] (third component 0) and valid [E,H,W,1]; no stereo
    rule, one set of intrinsics.  coords is the pixel itself where Z <= 0.01, valid is Z > 0.25.  `margins`: Z, X1, mag."""
    X0, X1, _, mag = transform(poses, disps, np.asarray(intrinsics, np.float64).reshape(4), ii, jj, stereo=False)
    fx, fy, cx, cy = np.asarray(intrinsics, np.float64).reshape(4)
    E, H, W = mag.shape
    x, y = _grid(H, W)
    Z = X1[..., 2]
    far = Z > PROJMAP_CLAMP
    Zs = np.where(far, Z, 1.0)
    coords = np.stack([np.where(far, fx * (X1[..., 0] / Zs) + cx, x[None]),
                       np.where(far, fy * (X1[..., 1] / Zs) + cy, y[None]), np.zeros((E, H, W))], axis=-1)
    valid = (Z > KERNEL_MIN_DEPTH).astype(np.float64)[..., None]
    if margins:
        return coords, valid, dict(Z=Z, X=X1, mag=mag)
    return coords, valid


def frame_distance(poses, disps, intrinsics, ii, jj, beta, margins=False):
    """frame_distance_kernel droid_kernels.cu:518-657: per edge the mean flow magnitude over the pixels with
    Z > 0.25, beta * (full motion) + (1 - beta) * (translation only); 1000 where less than 0.75 of the weight is
    valid.  `margins`: share (compared with 0.75), Z / Zt (full / translation-only depth, compared with 0.25), mag
    and the two flow magnitudes per pixel."""
    X0, X1, t, mag = transform(poses, disps, np.asarray(intrinsics, np.float64).reshape(4), ii, jj, stereo=False)
    fx, fy, cx, cy = np.asarray(intrinsics, np.float64).reshape(4)
    d0 = np.asarray(disps, np.float64)[np.asarray(ii, np.int64)]
    E, H, W = mag.shape
    x, y = _grid(H, W)

    def flow(X):
        with np.errstate(divide="ignore", invalid="ignore"):
            du = fx * (X[..., 0] / X[..., 2]) + cx - x[None]
            dv = fy * (X[..., 1] / X[..., 2]) + cy - y[None]
        return np.sqrt(du * du + dv * dv)

    Xt = X0 + t[:, None, None, :] * d0[..., None]                           # :626-630, rotation left out
    Z, Zt = X1[..., 2], Xt[..., 2]
    f1, f2 = flow(X1), flow(Xt)
    v1, v2 = Z > KERNEL_MIN_DEPTH, Zt > KERNEL_MIN_DEPTH
    parts = dict(a_full=np.where(v1, f1, 0.0).sum(axis=(1, 2)), a_trans=np.where(v2, f2, 0.0).sum(axis=(1, 2)),
                 n_full=v1.sum(axis=(1, 2)).astype(np.float64), n_trans=v2.sum(axis=(1, 2)).astype(np.float64),
                 pixels=H * W)
    dist, share = frame_distance_from_parts(parts, beta)
    if margins:
        parts.update(share=share, Z=Z, Zt=Zt, mag=mag, X=X1, Xt=Xt, flow=f1, flow_t=f2)
        return dist, parts
    return dist


def frame_distance_from_parts(parts, beta):
    """(dist, share) for one beta from the per-edge sums of `frame_distance(..., margins=True)`: the sums over the
    valid pixels do not depend on beta, so one pass over the pixels serves every beta."""
    accum = beta * parts["a_full"] + (1.0 - beta) * parts["a_trans"]
    valid = beta * parts["n_full"] + (1.0 - beta) * parts["n_trans"]
    share = valid / (float(parts["pixels"]) + 1e-8)
    with np.errstate(divide="ignore", invalid="ignore"):
        return np.where(share < 0.75, 1000.0, accum / valid), share         # :655


def iproj(poses, disps, intrinsics, margins=False):
    """iproj_kernel droid_kernels.cu:779-850: points [nm,H,W,3] = (R(q_f) X0 + d t_f) / d with the pose of frame f
    AS STORED (no inversion).  A zero disparity gives inf or nan.  `margins`: mag."""
    poses, disps, _ = _inputs(poses, disps, intrinsics)
    fx, fy, cx, cy = np.asarray(intrinsics, np.float64).reshape(4)
    nm, H, W = disps.shape
    x, y = _grid(H, W)
    X0 = np.broadcast_to(np.stack([(x - cx) / fx, (y - cy) / fy, np.ones((H, W))], axis=-1), (nm, H, W, 3))
    t, q = poses[:nm, :3], poses[:nm, 3:]
    X1 = _quat_rot(q[:, None, None, :], X0) + t[:, None, None, :] * disps[..., None]
    with np.errstate(divide="ignore", invalid="ignore"):
        pts = X1 / disps[..., None]
    if margins:
        mag = np.abs(X0[..., 0]) + np.abs(X0[..., 1]) + 1.0 + np.abs(disps) * np.abs(t).sum(axis=-1)[:, None, None]
        return pts, dict(mag=mag)
    return pts


_DF_SHIFTS = [(dv, du) for dv in (-1, 0, 1) for du in (-1, 0, 1)]


def depth_filter(poses, disps, intrinsics, ix, thresh, margins=False):
    """counter [num,H,W] of droid_kernels.cu:661-775 (depth_filter_kernel): for each selected frame ix and each of
    its six temporal neighbours jx = ix-1, ix-2, ix-3, ix+3, ix+4, ix+5 (:695 -- the kernel's own enumeration),
    every pixel is moved into jx with the relative pose WITHOUT the stereo special case, and the neighbour counts 1
    when the inverse of its transformed disparity is within `thresh` of the inverse disparity of one of the four
    pixels around its projection (:763-767; the comparison is carried out in double precision there, `1.0/dj`).
    Projections whose integer corner is outside [0,W-1) x [0,H-1) do not count (:748).

    `margins`: a second value, `band(c)`, that returns the [num,6,H,W] mask of (pixel, neighbour) decisions a float32
    evaluation may take differently: the smallest | 1/dj - 1/d | of the four corners within the rounding of `thresh`
    (c mag / |di| for Z, three roundings of 1/dj and two of 1/d), or uj / vj within the rounding of an integer
    (c * coord_scale) AND the corner one step over deciding differently or lying in the band of `thresh` itself."""
    poses = np.asarray(poses, np.float64)
    disps = np.asarray(disps, np.float64)
    K = np.asarray(intrinsics, np.float64)
    ix = np.asarray(ix, np.int64)
    thresh = np.asarray(thresh, np.float64)
    nbuf, H, W = disps.shape
    x, y = _grid(H, W)
    out = np.zeros((len(ix), H, W))
    rows = {}
    for b, i in enumerate(ix):
        if i < 0 or i >= nbuf:
            continue
        for nb in range(6):
            j = i - nb - 1 if nb < 3 else i + nb
            if j < 0 or j >= nbuf:
                continue
            X0, X1, t, mag = transform(poses, disps, K, np.array([i]), np.array([j]), stereo=False)
            X1, mag = X1[0], mag[0]
            with np.errstate(divide="ignore", invalid="ignore"):
                uj = K[0] * (X1[..., 0] / X1[..., 2]) + K[2]
                vj = K[1] * (X1[..., 1] / X1[..., 2]) + K[3]
                dj = disps[i] / X1[..., 2]
                idj = 1.0 / dj
            # corners far outside the image are all alike: clip before the integer conversion (inf, nan: outside)
            u0 = np.clip(np.nan_to_num(np.floor(uj), nan=-4.0), -4, W + 4).astype(np.int64)
            v0 = np.clip(np.nan_to_num(np.floor(vj), nan=-4.0), -4, H + 4).astype(np.int64)

            def decide(u0, v0, dnb=disps[j], idj=idj):       # bound now: band() calls it after the loop
                ok = (u0 >= 0) & (v0 >= 0) & (u0 < W - 1) & (v0 < H - 1)
                u0c, v0c = np.clip(u0, 0, max(W - 2, 0)), np.clip(v0, 0, max(H - 2, 0))
                near = np.full((H, W), np.inf)
                big = np.zeros((H, W))
                with np.errstate(divide="ignore", invalid="ignore"):
                    for dv, du in ((0, 0), (0, 1), (1, 0), (1, 1)):
                        inv = 1.0 / dnb[np.minimum(v0c + dv, H - 1), np.minimum(u0c + du, W - 1)]
                        near = np.fmin(near, np.abs(idj - inv))
                        big = np.fmax(big, np.abs(inv))
                return ok, near, big

            ok, near, big = decide(u0, v0)
            out[b] += (near < thresh[b]) & ok
            if margins:
                rows[(b, nb)] = dict(decide=decide, u0=u0, v0=v0, uj=uj, vj=vj, idj=idj, X=X1, mag=mag, di=disps[i],
                                     ok=ok, near=near, big=big, t=thresh[b])
    if not margins:
        return out

    def band(c=Z_BAND_C):
        m = np.zeros((len(ix), 6, H, W), bool)
        for (b, nb), r in rows.items():
            with np.errstate(divide="ignore", invalid="ignore"):
                bt = lambda big: EPS32 * (c * r["mag"] / np.abs(r["di"]) + 3.0 * np.abs(r["idj"]) + 2.0 * big)
                bu = c * EPS32 * coord_scale(K[0], K[2], r["X"][..., 0], r["X"][..., 2], r["mag"])
                bv = c * EPS32 * coord_scale(K[1], K[3], r["X"][..., 1], r["X"][..., 2], r["mag"])
            here = r["ok"] & (r["near"] < r["t"])
            inb = r["ok"] & ~(np.abs(r["near"] - r["t"]) > bt(r["big"]))      # a nan is in the band
            fu, fv = r["uj"] - np.floor(r["uj"]), r["vj"] - np.floor(r["vj"])
            su = {-1: ~(fu > bu), 0: np.ones((H, W), bool), 1: ~(1.0 - fu > bu)}   # which corners rounding can reach
            sv = {-1: ~(fv > bv), 0: np.ones((H, W), bool), 1: ~(1.0 - fv > bv)}
            for dv, du in _DF_SHIFTS:
                if dv == 0 and du == 0:
                    continue
                reach = su[du] & sv[dv]
                if not reach.any():
                    continue
                ok2, near2, big2 = r["decide"](r["u0"] + du, r["v0"] + dv)
                there = ok2 & (near2 < r["t"])
                inb |= reach & ((there != here) | (ok2 & ~(np.abs(near2 - r["t"]) > bt(big2))))
            m[b, nb] = inb
        return m

    return out, band
