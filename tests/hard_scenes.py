"""Bundle-adjustment scenes that synth.make_ba_problem never draws, and the bars they are judged by.  Plain helpers, no
fixtures: tests/test_hard_scenes.py proves on the CPU, from the oracle alone, that every scene does what it claims; the
GPU test (tests/test_gpu_ba_stages.py::test_hard_scene_stages_match_oracle) then runs the same scenes.

What the generator leaves out, and `harden` puts in:
  * intrinsics with fx, fy, cx, cy pairwise different (`aniso_K`): the generator has fx == fy == cx, so a kernel that
    reads one for another passes every other BA test;
  * observations behind MIN_DEPTH = 0.25 that are LIVE: the generator zeroes their weights itself, so the kernels' own
    `Z < MIN_DEPTH` branches (linearisation, Schur stage, back-substitution: each recomputes it) never decide anything.

The band rule is the one of tests/geom_cases.py: an observation whose fp64 depth lies within geom.z_band(mag) of 0.25
gets weight 0 on both rows, so that either decision gives the same system; the mask comes from the reference alone.

Bars (`bars`): nothing in them is measured from the device.
  H, b   max(STAGE_BARS[family], 2 x e32), e32 = util.scaled_system_errors of the oracle's own float32 evaluation
         against its fp64 one on the same scene.  The reference implementation is float32 throughout and the device
         accumulates in fp64, so it has no reason to be further from the truth; 2 for the order of the sums; the floor
         is the family's bar, so that a scene where float32 is lucky cannot fail a correct kernel.
  dx     2^-23 + 10 n 2^-53 cond_2(A), A the oracle's damped matrix: one float32 ulp of the largest component for the
         float32 output, and a backward-stable fp64 factorisation.
  state  max(family bar, 2 x util.relative_state_error of the oracle's float32 finish of the fp64 system against its
         fp64 finish).
"""
import copy

import numpy as np

import geom_cases as gc
import stage_graphs as sg
from droid_backends import synth
from oracle import geom
from util import STAGE_BARS, ba_args, relative_state_error, scaled_system_errors

MIN_DEPTH = geom.KERNEL_MIN_DEPTH
PULL = 0.35                       # geom_cases.matrix_case: wild trajectories pulled together so that views overlap
DISP_SIGMA = 0.8                  # disparities * exp(N(0, 0.8)): more than a decade
PERMUTATIONS = {"fx<->fy": (1, 0, 2, 3), "fx<->cx": (2, 1, 0, 3), "cx<->cy": (0, 1, 3, 2), "fy<->cy": (0, 3, 2, 1)}


aniso_K, aniso_K_frames = gc.aniso_K, gc.aniso_K_frames


def depths(p):
    """fp64 reference of every observation of `p`: Z [E,H,W], mag [E,H,W] (geom.z_band), projection [E,2,H,W]."""
    fx, fy, cx, cy = (float(v) for v in p.intrinsics)
    _, X1, _, mag = geom.transform(p.poses, p.disps, p.intrinsics, p.ii, p.jj, stereo=True)
    Z = X1[..., 2]
    with np.errstate(divide="ignore", invalid="ignore"):
        proj = np.stack([fx * (X1[..., 0] / Z) + cx, fy * (X1[..., 1] / Z) + cy], axis=1)
    return Z, mag, proj


def observe(p, rng, zero_share=0.1):
    """Targets and weights for the state `p` holds: the fp64 reprojection + N(0, 1 px), uniform over and beyond the
    image where the point is behind MIN_DEPTH or projects further than 4 max(H, W) from the principal point; weights
    U(0, 1), `zero_share` of them exactly 0, LIVE behind MIN_DEPTH, 0 on both rows inside the band of MIN_DEPTH."""
    _, H, W = p.disps.shape
    m = max(H, W)
    Z, mag, proj = depths(p)
    cx, cy = float(p.intrinsics[2]), float(p.intrinsics[3])
    near = (np.abs(proj[:, 0] - cx) <= 4 * m) & (np.abs(proj[:, 1] - cy) <= 4 * m)      # a nan is not near
    lost = (Z < MIN_DEPTH) | ~near
    noisy = np.where(lost[:, None], 0.0, proj) + rng.normal(0, 1.0, proj.shape)
    p.targets = np.where(lost[:, None], rng.uniform(-0.5 * m, 1.5 * m, proj.shape), noisy).astype(np.float32)
    w = rng.uniform(0, 1, proj.shape)
    w[rng.uniform(0, 1, proj.shape) < zero_share] = 0.0
    w[np.broadcast_to(gc.in_z_band(Z, mag, (MIN_DEPTH,))[:, None], w.shape)] = 0.0
    p.weights = w.astype(np.float32)
    return p


def harden(p, seed, rot_deg, variant="plain", push_frame=None):
    """`p` (a synth.BAProblem; not modified) with anisotropic intrinsics, wild poses of sigma rot_deg on the window
    [t0, t1) -- one window frame pushed by geom_cases.PUSH along z, translations pulled together by PULL, variant
    "negated": every second quaternion * -1 -- disparities spread over more than a decade, and the targets and weights
    of `observe`.  Frames below t0 keep their poses."""
    assert variant in ("plain", "negated"), variant
    p = copy.deepcopy(p)
    rng = np.random.default_rng(seed)
    _, H, W = p.disps.shape
    p.intrinsics = aniso_K(H, W)
    push_frame = min(p.t0 + 2, p.t1 - 1) if push_frame is None else push_frame
    assert p.t0 <= push_frame < p.t1
    wild = gc.wild_poses(p, rng, rot_deg, gc.PUSH, variant, push_frame)
    wild[:, :3] *= np.float32(PULL)
    p.poses = p.poses.copy()
    p.poses[p.t0:p.t1] = wild[p.t0:p.t1]
    p.disps = (p.disps * np.exp(rng.normal(0, DISP_SIGMA, p.disps.shape))).astype(np.float32)
    return observe(p, rng)


# ---------------------------------------------------------------------------------------------------------------------
# The BA depth ladder (after geom_cases.depth_ladder): identity rotations, frame f at z = -f, the anisotropic K.  Along
# the chain f -> f + 1 the depth is Z = 1 - d, and the disparities of frame f are chosen per pixel so that Z steps
# through LADDER_LEVELS: 5e-3 from MIN_DEPTH, about 1e5 float32 roundings, so no band applies and every weight is live.
# The edges back, f + 1 -> f, see Z = 1 + d: every pixel in front.  Five window frames: a reduced system.
LADDER_LEVELS = np.array([0.245, 0.255, 0.3, 1.0])
LADDER_N = 6


def ladder():
    """(BAProblem, level [E,H,W]: index into LADDER_LEVELS of every observation, -1 on the edges back)."""
    H, W, N = gc.LADDER_H, gc.LADDER_W, LADDER_N
    rng = np.random.default_rng(77)
    poses = np.zeros((N, 7), np.float32)
    poses[:, 6] = 1.0
    poses[:, 2] = -np.arange(N)
    ii = np.concatenate([np.arange(N - 1), np.arange(1, N)]).astype(np.int64)
    jj = np.concatenate([np.arange(1, N), np.arange(N - 1)]).astype(np.int64)
    k = np.arange(H * W)
    lv = np.stack([((k + 3 * f) % 4).reshape(H, W) for f in range(N - 1)])
    disps = np.full((N, H, W), 0.5, np.float32)
    disps[:N - 1] = (1.0 - LADDER_LEVELS[lv]).astype(np.float32)
    level = np.concatenate([lv, np.full((N - 1, H, W), -1)])
    eta = (0.2 * rng.uniform(0, 0.01, (N, H, W)) + 1e-7).astype(np.float32)
    E = len(ii)
    p = synth.BAProblem(poses=poses, disps=disps, intrinsics=aniso_K(H, W), disps_sens=np.zeros((N, H, W), np.float32),
                        targets=np.zeros((E, 2, H, W), np.float32), weights=np.zeros((E, 2, H, W), np.float32), eta=eta,
                        ii=ii, jj=jj, t0=1, t1=N, lm=1e-4, ep=0.1)
    observe(p, rng, zero_share=0.0)
    p.weights = np.maximum(p.weights, np.float32(0.05))          # every weight live
    return p, level


# ---------------------------------------------------------------------------------------------------------------------
class Scene:
    """id, family of the floor bars (util.STAGE_BARS), the Schur classes the device must report -- those of the plain
    form of the graph --, whether the packed build runs too, and problem(): the BAProblem (built once)."""

    def __init__(self, id, make, family, classes, packed=False):
        self.id, self._make, self.family, self.classes, self.packed = id, make, family, classes, packed
        self.motion_only = classes == {"motion"}
        self._p = None
        self._bars = None

    def problem(self):
        if self._p is None:
            self._p = self._make()
        return self._p


def _window(H, W, rot_deg, variant="plain", **kw):
    """the smallest window of the other suites (cfg1's graph: 8 frames, 32 edges) at a shape below one workgroup or
    no multiple of 32 pixels"""
    seed = H * 1009 + W * 31 + int(rot_deg) * 7
    return lambda: harden(synth.make_ba_problem(N=8, E=32, H=H, W=W, seed=seed, **kw), seed + 1, rot_deg, variant)


def _graph(name, seed, rot_deg=20.0, push_frame=None):
    return lambda: harden(sg.GRAPHS[name][0](synth), seed, rot_deg, "plain", push_frame)


def _scenes():
    out = []
    special = {(13, 21, 20.0): ("negated", "sparse", dict()), (8, 32, 20.0): ("stereo", "stereo", dict(stereo=True)),
               (9, 19, 60.0): ("rgbd", "sparse", dict(rgbd=True))}
    for (H, W) in ((9, 19), (13, 21), (8, 32)):
        for rot in (5.0, 20.0, 60.0):
            tag, family, kw = special.get((H, W, rot), ("plain", "sparse", dict()))
            out.append(Scene(f"win{H}x{W}-rot{rot:g}-{tag}", _window(H, W, rot, "negated" if tag == "negated" else "plain", **kw),
                             family, {0}))
    for name, seed, packed, push in (("every_class", 501, True, None), ("dense30_block_pair", 502, False, None),
                                     ("dense36_syrk", 503, False, None), ("variant_stereo_pairs", 504, False, None),
                                     ("variant_window_t0_3", 505, False, None), ("motion_only", 506, True, 7)):
        _, family, classes = sg.GRAPHS[name]
        out.append(Scene(f"hard_{name}", _graph(name, seed, push_frame=push), family, classes, packed))
    out.append(Scene("ladder", lambda: ladder()[0], "sparse", {0}))
    return out


SCENES = {s.id: s for s in _scenes()}


def damped(H, lm, ep):
    """the matrix droid_ba_solve_update factors (util.damped_solve), symmetric, from a lower triangle"""
    lm, ep = float(np.float32(lm)), float(np.float32(ep))
    A = np.tril(H) + np.tril(H, -1).T
    A[np.diag_indices_from(A)] += ep + lm * np.diag(A)
    return A


def build64(oracle, p, motion_only):
    ph = oracle.BAPhases()
    H, b = ph.build(*ba_args(p), 0, p.disps.shape[0], motion_only)
    return ph, H, b


def scene_bars(sc):
    """The bars of the scene `sc` (see the head of this file; any object with id, family, motion_only and problem()),
    from the oracle alone, computed once per scene object.  Next to H, b, dx, state: e32 (H, b, state of the float32
    oracle), cond, n, and `ref`: the fp64 system and its finish."""
    if getattr(sc, "_bars", None) is not None:
        return sc._bars
    import oracle
    p, mo = sc.problem(), sc.motion_only
    ph64, Ho, bo = build64(oracle, p, mo)
    ph32 = oracle.BAPhases("f32")
    H32, b32 = ph32.build(*ba_args(p), 0, p.disps.shape[0], mo)
    e32 = scaled_system_errors(H32, b32, Ho, bo)
    A = damped(Ho, p.lm, p.ep)
    cond, n = float(np.linalg.cond(A)), A.shape[0]
    lm, ep = float(np.float32(p.lm)), float(np.float32(p.ep))
    full = np.tril(Ho) + np.tril(Ho, -1).T
    s64 = ph64.finish(full, bo, lm, ep)
    s32 = ph32.finish(full, bo, lm, ep)
    e32s = relative_state_error(p, s32[:2], s64[:2])
    fam = STAGE_BARS[sc.family]
    sc._bars = dict(H=max(fam["H"], 2 * e32["H"]), b=max(fam["b"], 2 * e32["b"]), dx=2.0 ** -23 + 10 * n * 2.0 ** -53 * cond,
                    state=max(fam["state"], 2 * max(e32s)), e32=dict(H=e32["H"], b=e32["b"], state=e32s, dead=e32["dead"]),
                    cond=cond, n=n, ref=dict(H=Ho, b=bo, A=A, poses=s64[0], disps=s64[1], dx=s64[2]))
    return sc._bars


def bars(scene_id):
    """scene_bars of the scene of SCENES with that id"""
    return scene_bars(SCENES[scene_id])


def scene_bars_line(sc):
    b = scene_bars(sc)
    return (f"[{sc.id}] bars H {b['H']:.2e} b {b['b']:.2e} dx {b['dx']:.2e} state {b['state']:.2e} | float32 oracle H "
            f"{b['e32']['H']:.2e} b {b['e32']['b']:.2e} state {max(b['e32']['state']):.2e} | n {b['n']} cond {b['cond']:.2e}")


def bars_line(scene_id):
    return scene_bars_line(SCENES[scene_id])
