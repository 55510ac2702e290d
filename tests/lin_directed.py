"""Directed inputs for the fp64 roundings of the BA linearisation, and a CPU discriminator that proves they are directed.

The FULL body of ba_lin_kernel (csrc/ba_kernels.hip: lin_pixel_pinned and its neighbours) writes out by hand the fused
multiply-adds the compiler chose in the ragged body (se3.hpp::linearize_pixel_d).  A wrong choice in the fp32 part shows
on every input.  A wrong choice in the fp64 part -- the point xd, yd, zd, the two Newton steps of rd, ru / rv -- moves a
result by one fp64 ulp, and everything that reads it reads it rounded to float: on generic inputs the float changes once
in about 2^29 evaluations.  The families below are inputs on which it changes at a few per cent of the pixels, because
the float that is read is the small difference of two large fp64 terms:

  cancel_x       the source frame's disparity is float(-(R0 X0 + R1 X1 + R2) / t0) per pixel, so xd = sum + d t0 is the
                 rounding residue of that float, 2^-24 of the sum: an fp64 ulp of the sum is 2^-29 of xd.  The v weights of
                 the designated edges are 0, so every Hjj entry of rows 2, 3 and every E row entry that carries Ju[2..5]
                 is proportional to x alone.
  cancel_y       the mirror image: yd cancels, the u weights are 0.
  zero_residual  the targets of the designated edges are float32 of the fp64 projection, so ru = tu - (fx rd xd + cx) and
                 rv are rounding residues of the projection: an ulp of xd, yd, zd, rd or of the projection reaches them.
                 The state a converged run approaches.

A disparity map is shared by all edges of its source frame, so a case designates at most one edge per source frame, whole
edges (both pixels of every lane), never a stereo pair (R = I: both fusion orders are exact).  All other edges keep generic
targets and weights.  cancel_x / cancel_y need a scene in which the cancelling disparity is positive and the depth stays
near 1 at every pixel: the principal column (row) of the camera lies outside the image on the side the camera moves
towards (0.05 per frame), and the designated edges look two to four frames ahead.  `redraw` draws that scene -- trajectory,
intrinsics, targets and weights -- for the graph, disparities, eta, lm and ep of a synth.make_ba_problem.  zero_residual needs no
cancelling disparity, but its rarest site, the sum of zd, shows only where R6 X0 + R7 X1 is of the size of R8: a short
lens and a camera that turns (turning_scene).

fp64_sites restates the fp64 part of lin_pixel_pinned with every rounding exact (integer arithmetic, one rounding per
operation) and one switch per rounding site; tests/test_lin_directed.py counts, per case, site and pixel-of-lane, the
designated pixels at which flipping that one switch changes a float the kernel reads, and asks for at least 16.
"""
import copy
import math

import numpy as np

import stage_graphs as sg
from lin_hook import LIN_CP

MIN_DEPTH = 0.25          # include/droid_backends_hip.h: DROID_MIN_DEPTH
SITES = ("x", "y", "z", "newton1", "newton2", "ru", "rv")
AB, CD = 0, 1             # ba_kernels.hip: LIN_FUSE_AB = fma(a, b, c*d), LIN_FUSE_CD = fma(c, d, a*b)


# ---- the fp64 arithmetic, exactly --------------------------------------------------------------------------------------
def _parts(x):
    m, e = math.frexp(x)
    return int(m * 9007199254740992.0), e - 53          # x = m 2^e, m an integer (exact: 53 bits)


def fma(a, b, c):
    """a * b + c rounded once to float64 (ties to even).  Exact integer arithmetic; float(int) rounds correctly.
    For finite arguments whose result is a normal number (all that the linearisation meets)."""
    ma, ea = _parts(a)
    mb, eb = _parts(b)
    mc, ec = _parts(c)
    mp, ep = ma * mb, ea + eb
    if mp == 0:
        return a * b + c
    if mc == 0:
        return math.ldexp(float(mp), ep)
    e = min(ep, ec)
    return math.ldexp(float((mp << (ep - e)) + (mc << (ec - e))), e)


def _sum2(how, a, b, c, d):
    return fma(a, b, c * d) if how == AB else fma(c, d, a * b)


def _f32(x):
    return float(np.float32(x))


def pinned_sites(inst, p):
    """The choice ba_kernels.hip::lin_fuse and lin_pixel_pinned make for pixel-of-lane p of instantiation `inst` =
    (depth, E rows, edge ranges): the baseline the discriminator flips one site of.  (Restated; the GPU tests hold the
    kernel's own table against the ragged body.)"""
    depth, erows, _ = inst
    if erows:
        xy = (AB, CD)
    elif p == 0:
        xy = (AB, AB if depth else CD)
    else:
        xy = (CD, AB)
    return dict(x=xy[0], y=xy[1], z=AB, newton1=1, newton2=1, ru=1, rv=1)


def fp64_sites(K, R, t, X0, X1, disp, tu, tv, sites):
    """The fp64 part of lin_pixel_pinned for one pixel, each operation rounded once.  K: the four float32 intrinsics; R
    (9), t (3): the relative pose in float64; X0, X1: the back-projected pixel (float64); disp, tu, tv: float32 values.
    sites: x, y, z = which product of the sum of two products is fused (AB / CD); newton1, newton2, ru, rv = 1: fused,
    0: multiply, then add.  Returns the float32 values (x, y, d, ru, rv) as Python floats, and zd."""
    fx, fy, cx, cy = (float(k) for k in K)
    dd = float(disp)
    xd = fma(dd, t[0], _sum2(sites["x"], R[0], X0, R[1], X1) + R[2])
    yd = fma(dd, t[1], _sum2(sites["y"], R[3], X0, R[4], X1) + R[5])
    zd = fma(dd, t[2], _sum2(sites["z"], R[6], X0, R[7], X1) + R[8])
    rd = float(np.float32(1.0) / np.float32(zd))
    rd = rd * (fma(-zd, rd, 2.0) if sites["newton1"] else 2.0 - zd * rd)
    rd = rd * (fma(-zd, rd, 2.0) if sites["newton2"] else 2.0 - zd * rd)
    if zd < MIN_DEPTH:
        rd = 0.0
    ru = float(tu) - (fma(fx * rd, xd, cx) if sites["ru"] else fx * rd * xd + cx)
    rv = float(tv) - (fma(fy * rd, yd, cy) if sites["rv"] else fy * rd * yd + cy)
    return (_f32(xd), _f32(yd), _f32(rd), _f32(ru), _f32(rv)), zd


# ---- geometry on the CPU, float64 from the float32 state ----------------------------------------------------------------
def rel_pose_mat(poses, i, j):
    """se3.hpp::rel_pose_mat<double> of a non-stereo pair: R (9, row-major), t (3).  An ulp of disagreement with the
    device (which may contract) is harmless: the families need the cancellation, not its bits."""
    ti, qi = [np.float64(v) for v in poses[i, :3]], [np.float64(v) for v in poses[i, 3:]]
    tj, qj = [np.float64(v) for v in poses[j, :3]], [np.float64(v) for v in poses[j, 3:]]
    x = -qj[3] * qi[0] + qj[0] * qi[3] - qj[1] * qi[2] + qj[2] * qi[1]
    y = -qj[3] * qi[1] + qj[1] * qi[3] - qj[2] * qi[0] + qj[0] * qi[2]
    z = -qj[3] * qi[2] + qj[2] * qi[3] - qj[0] * qi[1] + qj[1] * qi[0]
    w = qj[3] * qi[3] + qj[0] * qi[0] + qj[1] * qi[1] + qj[2] * qi[2]
    R = [1.0 - 2.0 * (y * y + z * z), 2.0 * (x * y - z * w), 2.0 * (x * z + y * w),
         2.0 * (x * y + z * w), 1.0 - 2.0 * (x * x + z * z), 2.0 * (y * z - x * w),
         2.0 * (x * z - y * w), 2.0 * (y * z + x * w), 1.0 - 2.0 * (x * x + y * y)]
    t = [tj[n] - (R[3 * n] * ti[0] + R[3 * n + 1] * ti[1] + R[3 * n + 2] * ti[2]) for n in range(3)]
    return [float(v) for v in R], [float(v) for v in t]


def back_projected(K, H, W):
    """X0, X1 of every pixel as ba_lin_kernel forms them: ((double)(k % W) - cx) / fx, ((double)(k / W) - cy) / fy."""
    fx, fy, cx, cy = (np.float64(k) for k in K)
    k = np.arange(H * W)
    return ((k % W).astype(np.float64) - cx) / fx, ((k // W).astype(np.float64) - cy) / fy


def point(p, e):
    """(xd, yd, zd) of every pixel of edge e at the state of `p`, float64 arrays (numpy: every product and sum rounded
    separately -- for choosing inputs, not for judging roundings)."""
    _, H, W = p.disps.shape
    R, t = rel_pose_mat(p.poses, int(p.ii[e]), int(p.jj[e]))
    X0, X1 = back_projected(p.intrinsics, H, W)
    d = p.disps[int(p.ii[e])].reshape(-1).astype(np.float64)
    return tuple(R[3 * n] * X0 + R[3 * n + 1] * X1 + R[3 * n + 2] + d * t[n] for n in range(3))


# ---- the families -------------------------------------------------------------------------------------------------------
def redraw(p, intr, drift, turn, seed, t_noise=0.01):
    """A scene for the graph of `p`: a camera with intrinsics `intr` that moves by `drift` and turns by `turn` (radians
    about x, y, z) per frame, plus noise (rotation 1 degree as the generator draws it, translation `t_noise`); the state
    = the ground truth perturbed by 0.4 t_noise and 0.5 degrees; targets = reprojection of the ground truth + N(0, 0.25)
    and weights U(0, 1) for every edge, as the generator draws them, except that a target may lie outside the image (a
    point closer than MIN_DEPTH gets weight 0 all the same).  The disparities, eta, lm and ep of `p` stay."""
    from droid_backends import synth
    rng = np.random.default_rng(seed)
    q = copy.deepcopy(p)
    nbuf = p.disps.shape[0]
    intr = np.asarray(intr, np.float64)
    gt = np.zeros((nbuf, 7))
    gt[:, 6] = 1.0
    for k in range(1, nbuf):
        xi = np.concatenate([rng.normal(0, t_noise, 3) + drift, rng.normal(0, np.deg2rad(1.0), 3) + turn])
        dt, dq = synth.se3_exp(xi)
        t, qq = synth.se3_mul(dt, dq, gt[k - 1, :3], gt[k - 1, 3:])
        gt[k, :3], gt[k, 3:] = t, qq / np.linalg.norm(qq)
    gt = gt[track(p)]
    poses = gt.copy()
    for k in range(1, nbuf):
        xi = np.concatenate([rng.normal(0, 0.4 * t_noise, 3), rng.normal(0, np.deg2rad(0.5), 3)])
        dt, dq = synth.se3_exp(xi)
        t, qq = synth.se3_mul(dt, dq, gt[k, :3], gt[k, 3:])
        poses[k, :3], poses[k, 3:] = t, qq / np.linalg.norm(qq)
    coords, Z = synth.reproject(gt, p.gt_disps, intr, p.ii, p.jj)
    q.intrinsics = intr.astype(np.float32)
    q.poses, q.gt_poses, q.gt_coords = poses.astype(np.float32), gt, coords
    q.targets = (coords + rng.normal(0, 0.25, coords.shape)).astype(np.float32)
    q.weights = (rng.uniform(0, 1, coords.shape) * (Z >= MIN_DEPTH)[:, None]).astype(np.float32)
    return q


def track(p):
    """Position of every frame along the trajectory `redraw` draws: the frame index, unless the graph says otherwise
    (p.track: the motion-only graph interleaves its fixed and its new frames)."""
    return np.asarray(getattr(p, "track", np.arange(p.disps.shape[0])))


def _ahead(p, e):
    tr = track(p)
    return int(tr[int(p.jj[e])]) - int(tr[int(p.ii[e])])


def cancel_scene(p, axis, seed):
    """The scene of cancel_x (axis 0) / cancel_y (axis 1): the camera moves 0.05 per frame along `axis`, as the
    generator's does along x (so that the translations, and with them the float32 ulp of the stored state, keep the
    generator's size), behind a long lens whose principal column (row) lies half an image beyond the image's far edge:
    the back-projected coordinate along `axis` is -0.3 .. -0.1 and the disparity that cancels it two to four frames
    ahead is 0.5 .. 3."""
    _, H, W = p.disps.shape
    size = (W, H)[axis]
    intr = np.array([size / 0.2, size / 0.2, W / 2.0, H / 2.0])
    intr[2 + axis] = 1.5 * size
    drift = np.zeros(3)
    drift[axis] = 0.05
    return redraw(p, intr, drift, np.zeros(3), seed, t_noise=0.004)


def _designate(p, count, usable, taken=()):
    """The first `count` edges, in the order of the edge list, that are no stereo pair, leave from distinct source
    frames (none of `taken`) and pass usable(e)."""
    out, src = [], set(taken)
    for e in range(len(p.ii)):
        i, j = int(p.ii[e]), int(p.jj[e])
        if i == j or i in src or not usable(e):
            continue
        out.append(e)
        src.add(i)
        if len(out) == count:
            return out
    raise AssertionError(f"only {len(out)} of {count} designated edges found")


def _cancel(p, axis, count, seed):
    q = cancel_scene(p, axis, seed)
    rng = np.random.default_rng(seed + 1)
    _, H, W = q.disps.shape
    X0, X1 = back_projected(q.intrinsics, H, W)

    def disparity(e):
        R, t = rel_pose_mat(q.poses, int(q.ii[e]), int(q.jj[e]))
        s = R[3 * axis] * X0 + R[3 * axis + 1] * X1 + R[3 * axis + 2]
        d = (-s / t[axis]).astype(np.float32)
        z = R[6] * X0 + R[7] * X1 + R[8] + d.astype(np.float64) * t[2]
        return d, z

    def usable(e):
        if not 2 <= _ahead(q, e) <= 4:       # two to four frames ahead: t[axis] 0.1 .. 0.2
            return False
        d, z = disparity(e)
        return bool(np.all(np.isfinite(d)) and d.min() > 0.25 and d.max() < 4.0 and z.min() > 0.75)

    edges = _designate(q, count, usable)
    for e in edges:
        i = int(q.ii[e])
        d, _ = disparity(e)
        q.disps[i] = d.reshape(H, W)
        q.gt_disps[i] = d.reshape(H, W)
    # the other edges of the rewritten source frames see the new points: their generic targets follow them
    from droid_backends import synth
    hit = np.isin(q.ii, [int(q.ii[e]) for e in edges])
    coords, Z = synth.reproject(q.gt_poses, q.gt_disps, q.intrinsics.astype(np.float64), q.ii[hit], q.jj[hit])
    q.gt_coords[hit] = coords
    q.targets[hit] = (coords + rng.normal(0, 0.25, coords.shape)).astype(np.float32)
    q.weights[hit] = (rng.uniform(0, 1, coords.shape) * (Z >= MIN_DEPTH)[:, None]).astype(np.float32)
    for e in edges:
        # the cancelled coordinate projects onto the principal column (row): targets there, +- the generator's noise
        x, y, z = point(q, e)
        fx, fy, cx, cy = (float(k) for k in q.intrinsics)
        proj = np.stack([fx * x / z + cx, fy * y / z + cy]).reshape(2, H, W)
        q.targets[e] = (proj + rng.normal(0, 0.25, proj.shape)).astype(np.float32)
        q.weights[e, axis] = rng.uniform(0.05, 1, (H, W)).astype(np.float32)
        q.weights[e, 1 - axis] = 0.0
    return q, edges


def cancel_x(p, count, seed=0):
    """`p` redrawn (cancel_scene, axis 0) with `count` designated edges on which xd cancels; returns (problem, edges)."""
    return _cancel(p, 0, count, seed)


def cancel_y(p, count, seed=0):
    """The mirror image of cancel_x: yd cancels, the u weights of the designated edges are 0."""
    return _cancel(p, 1, count, seed)


def turning_scene(p, seed):
    """The scene of zero_residual: the generator's drift (0.05 per frame along x) with a camera that also turns 2, 3 and
    1 degrees per frame about x, y, z, seen through a short lens (fx, fy about W / 6, no round numbers: no product of
    the point is exact).  Two to four frames apart |R6 X0 + R7 X1| reaches 0.25 .. 0.5 over much of the image, where an
    ulp of that sum survives the addition of R8; with the generator's R = I + 0.02 and |X| < 1 the z site shows nowhere."""
    _, H, W = p.disps.shape
    intr = [W / 6.0 * 1.03, W / 6.0 * 0.98, W / 2.0 + 0.37, H / 2.0 - 0.21]
    return redraw(p, intr, np.array([0.05, 0.0, 0.0]), np.deg2rad([2.0, 3.0, 1.0]), seed, t_noise=0.05)


def zero_residual(p, count, seed=0):
    """`p` redrawn (turning_scene) with the targets of `count` designated edges, two to four frames apart, set to float32
    of the fp64 projection of the state, both components, and their weights to U(0.05, 1); the disparities stay generic.
    Returns (problem, edges)."""
    q = turning_scene(p, seed)
    rng = np.random.default_rng(seed + 2)
    _, H, W = q.disps.shape
    fx, fy, cx, cy = (float(k) for k in q.intrinsics)
    edges = _designate(q, count, lambda e: 2 <= abs(_ahead(q, e)) <= 4 and bool(point(q, e)[2].min() > 0.55))
    for e in edges:
        x, y, z = point(q, e)
        rd = 1.0 / z
        q.targets[e] = np.stack([fx * rd * x + cx, fy * rd * y + cy]).reshape(2, H, W).astype(np.float32)
        q.weights[e] = rng.uniform(0.05, 1, (2, H, W)).astype(np.float32)
    return q, edges


# family -> (builder, the sites it is meant to expose, designated edges per case).  One edge gives 7 to 14 pixels per
# half of a 512-pixel chunk at the x, y, ru, rv sites; the z site, the rarest, about 3 on the turning scene.
FAMILIES = {"cancel_x": (cancel_x, ("x",), 4), "cancel_y": (cancel_y, ("y",), 4), "zero_residual": (zero_residual, SITES, 8)}


# ---- the cases: FULL shapes, the smallest that reach each instantiation --------------------------------------------------
def _band(N, reach):
    return sg._edges(sg._band(N, reach))


def _motion(s, H, W):
    """New frames [8, 16) observed from the fixed keyframes 0 .. 7.  Along the trajectory two fixed frames and two new
    ones alternate (p.track), so that every fixed frame has a new one two frames ahead; edges: up to four frames apart."""
    tr = np.array([4 * (k // 2) + k % 2 for k in range(8)] + [4 * (k // 2) + 2 + k % 2 for k in range(8)])
    pairs = {(i, j) for i in range(8) for j in range(8, 16) if abs(int(tr[i]) - int(tr[j])) <= 4}
    p = s.make_ba_problem(N=16, H=H, W=W, seed=7, edges=sg._edges(pairs))
    p.t0, p.t1, p.track = 8, 16, tr
    return p


# graph -> (builder(synth), motion-only, (depth, E rows, edge ranges), family of util.STAGE_BARS, Schur classes)
GRAPHS = {
    "16kf_64e_16x32": (lambda s: s.make_ba_problem(N=16, E=64, H=16, W=32, seed=2), False, (1, 0, 1), "sparse", {0}),
    "24kf_band9_16x32": (lambda s: s.make_ba_problem(N=24, H=16, W=32, seed=21, lm=1e-4, ep=0.1, edges=_band(24, 9)),
                         False, (1, 1, 1), "dense", {0, 1}),
    "260kf_800e_32x48": (lambda s: s.make_ba_problem(N=260, E=800, H=32, W=48, seed=3), False, (1, 0, 0), "sparse", {0}),
    "260kf_band9_32x48": (lambda s: s.make_ba_problem(N=260, H=32, W=48, seed=4, lm=1e-4, ep=0.1, edges=_band(260, 9)),
                          False, (1, 1, 0), "dense", {0, 1}),
    "motion_only_16kf_16x32": (lambda s: _motion(s, 16, 32), True, (0, 0, 0), "motion", {"motion"}),
}
CASES = {f"{fam}-{g}": (fam, g) for fam in FAMILIES for g in GRAPHS}
_built = {}


def build_case(name):
    """(problem, designated edges, motion-only, instantiation, bar family, Schur classes) of case `name`; built once
    per process and shared (callers do not write to it)."""
    if name not in _built:
        from droid_backends import synth
        fam, g = CASES[name]
        make, mo, inst, family, classes = GRAPHS[g]
        p, edges = FAMILIES[fam][0](make(synth), FAMILIES[fam][2])
        _built[name] = (p, edges, mo, inst, family, classes)
    return _built[name]


def designated_pixels(p, edges):
    """Per designated pixel: (edge, pixel, pixel-of-lane, arguments of fp64_sites without `sites`)."""
    _, H, W = p.disps.shape
    X0, X1 = back_projected(p.intrinsics, H, W)
    for e in edges:
        i, j = int(p.ii[e]), int(p.jj[e])
        R, t = rel_pose_mat(p.poses, i, j)
        d, tg = p.disps[i].reshape(-1), p.targets[e].reshape(2, -1)
        for k in range(H * W):
            yield e, k, (k % LIN_CP) // (LIN_CP // 2), (p.intrinsics, R, t, float(X0[k]), float(X1[k]), d[k], tg[0, k], tg[1, k])


def discrimination(p, edges, inst, sites):
    """{site: [count for pixel-of-lane 0, for 1]}: the designated pixels at which flipping that one site of the pinned
    choice changes any of the float32 values x, y, d, ru, rv; and the smallest zd met."""
    counts = {s: [0, 0] for s in sites}
    zmin = math.inf
    for e, k, half, args in designated_pixels(p, edges):
        base = pinned_sites(inst, half)
        ref, zd = fp64_sites(*args, base)
        zmin = min(zmin, zd)
        for s in sites:
            got, _ = fp64_sites(*args, dict(base, **{s: 1 - base[s]}))
            counts[s][half] += int(got != ref)
    return counts, zmin
