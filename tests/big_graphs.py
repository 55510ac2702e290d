"""Bundle-adjustment graphs that take the code chosen by SIZE alone, and the bars they are judged by.  Plain helpers, no
fixtures: tests/test_big_graphs.py proves on the CPU, from the oracle alone, that every scene reaches what it claims and
that the reached code decides the result; tests/test_gpu_ba_big_graphs.py then runs the scenes on the device.

Two groups (csrc/ba_kernels.hip):
  * hubs: a source frame with more than SLOT_MAXE = 128 edges.  Every BA kernel keeps a slot's per-edge metadata in LDS
    in chunks of 128 edges; such a slot reloads the chunk inside ba_lin_kernel's edge loop, leaves the `resident` path
    of ba_schur_fused_kernel (the only Schur kernel it can get: schur_class sends nedges > 128 to class 3) and takes
    more than one pass of ba_backsub_kernel's chunk loop.
  * prep tables outside LDS: launch_prep builds the tables in dynamic LDS while 4 prep_ints(nbuf, E) <= 150 KB and in
    the workspace's own arrays beyond (ba_prep_kernel<false>).

Why `hover`: with synth.make_ba_problem's drifting trajectory the 129th and later edges of a hub point at frames that
share no view with it, and the generator gives them weight 0 everywhere -- a kernel that dropped its second chunk would
pass (tests/test_big_graphs.py asserts this of the plain hub160, so that the reason stays on record).  A camera that
barely moves is also what produces hubs in practice.

Bars: the recipe of hard_scenes.scene_bars, unchanged; nothing in them is measured from the device.  The family floors
are util.STAGE_BARS["dense"] for the hub scenes and the two 128-frame prep graphs, "sparse" for prep_global_frames.
"""
import copy

import numpy as np

import hard_scenes as hs
import stage_graphs as sg
from droid_backends import synth

SLOT_MAXE = 128                     # csrc/ba_kernels.hip: edges per metadata chunk
LIN_WGS, LIN_CP = 1536, 512         # csrc/ba_internal.hpp: the linearisation's workgroup budget, pixels per chunk
PREP_LDS_INTS = 150 * 1024 // 4     # launch_prep: ba_prep_kernel<true> up to this many ints of dynamic LDS


def hover(p, seed, sig_t=0.05, sig_deg=1.0):
    """`p` (not modified) seen by a camera that barely moves: every pose of the buffer a translation N(0, sig_t) per
    axis and a rotation vector N(0, sig_deg degrees) per axis, as a float32 quaternion; frame 0 the identity; targets
    and weights of hard_scenes.observe for that state.  Intrinsics and disparities stay the generator's."""
    p = copy.deepcopy(p)
    rng = np.random.default_rng(seed)
    nbuf = p.poses.shape[0]
    t = rng.normal(0, sig_t, (nbuf, 3))
    q = synth.so3_exp(rng.normal(0, np.deg2rad(sig_deg), (nbuf, 3)))
    poses = np.concatenate([t, q / np.linalg.norm(q, axis=1, keepdims=True)], 1)
    poses[0] = (0, 0, 0, 0, 0, 0, 1)
    p.poses = poses.astype(np.float32)
    return hs.observe(p, rng)


# ---------------------------------------------------------------------------------------------------------------------
# host restatements (for the CPU proofs, not for judging the device)
def zsplit_of(p):
    """ba_launch_plan: workgroups that share a (slot, pixel chunk) of the linearisation, each with a range of its edges"""
    _, H, W = p.disps.shape
    M = p.eta.shape[0]
    nch = (H * W + LIN_CP - 1) // LIN_CP
    return min(max(LIN_WGS // (M * nch), 1), 8)


def edge_ranges(ne, z):
    """ba_lin_kernel<ZSPLIT>: the ranges [a, b) of a slot's `ne` edges its z workgroups take (empty ones left out)"""
    per = (ne + z - 1) // z
    out = [(min(ne, k * per), min(ne, k * per + per)) for k in range(z)]
    return [(a, b) for a, b in out if b > a]


def prep_ints(nbuf, E):
    """prep_lds_ints (csrc/ba_kernels.hip)"""
    return 9 * (nbuf + 2) + 4 * (E + 1)


def hub_edges(p, f):
    """indices of the edges out of frame f, ascending: the order ba_prep_kernel gives a slot's edges"""
    return np.flatnonzero(p.ii == f)


def chunks(p, f):
    """the metadata chunks of frame f: index arrays of at most SLOT_MAXE edges"""
    e = hub_edges(p, f)
    return [e[c:c + SLOT_MAXE] for c in range(0, len(e), SLOT_MAXE)]


def without(p, edges):
    """`p` with the weights of `edges` zeroed (shallow copy)"""
    q = copy.copy(p)
    q.weights = p.weights.copy()
    q.weights[edges] = 0
    return q


# ---------------------------------------------------------------------------------------------------------------------
def _far(N, f, reach, count):
    """(f, j) for the first `count` frames j with |j - f| > reach"""
    return {(f, j) for j in [j for j in range(N) if abs(j - f) > reach][:count]}


def _all(N, f):
    return {(f, j) for j in range(N) if j != f}


def plain_hub(N, H, W, reach, t0, extra):
    return synth.make_ba_problem(N=N, H=H, W=W, seed=31, lm=1e-4, ep=0.1, t0=t0, edges=sg._edges(sg._band(N, reach) | extra))


def _hub(*a):
    return lambda: hover(plain_hub(*a), 700)


def _prep(N, nbuf, seed, edges=None, E=None):
    kw = dict(edges=sg._edges(edges)) if edges is not None else dict(E=E)
    return lambda: synth.make_ba_problem(N=N, nbuf=nbuf, H=4, W=8, seed=seed, lm=1e-4, ep=0.1, **kw)


_BAND128 = sorted(sg._band(128, 34))


class Scene(hs.Scene):
    """hard_scenes.Scene + what the tables of this file state: edge count, slots per Schur class (0, 1, 2, 3), zsplit,
    hubs {frame: out-degree}, ints of the prep tables."""

    def __init__(self, id, make, family, E, counts, zsplit, hubs=None, ints=None, packed=False):
        super().__init__(id, make, family, {c for c, k in enumerate(counts) if k > 0}, packed)
        self.E, self.counts, self.zsplit, self.hubs, self.ints = E, counts, zsplit, hubs or {}, ints


HUB160 = (160, 8, 16, 2, 30, _all(160, 40) | _far(160, 90, 2, 124) | _far(160, 120, 2, 125))
HUB262 = (262, 4, 8, 2, 1, _all(262, 5) | _far(262, 200, 2, 252))

HUBS = {s.id: s for s in [
    # not wide.  128 stays resident, 129 gives a chunk of one edge, 159 a second chunk of 31; thirty first-chunk targets
    # of hub 40 lie before t0, so the entry base of its second chunk is not 129; edge ranges of 20: [120, 140) crosses
    # the chunk boundary, [140, 159) starts inside the second chunk
    Scene("hub160", _hub(*HUB160), "dense", 1038, (157, 0, 0, 3), 8, {40: 159, 90: 128, 120: 129}, packed=True),
    # wide: the EROWS linearisation with emit == false for the hub, SYRK classes beside it; a stereo edge in a chunked slot
    Scene("hub160_wide", _hub(160, 8, 16, 9, 30, _all(160, 40) | {(40, 40)}), "dense", 2932, (29, 130, 0, 1), 8, {40: 160}),
    # three chunks; 256 = two full chunks exactly; ranges of 53 cross 128 and 256; 32 pixels: less than a tile of any kernel
    Scene("hub262", _hub(*HUB262), "dense", 1551, (260, 0, 0, 2), 5, {5: 261, 200: 256}, packed=True),
    # M * nch = 800 > 768: the linearisation without ZSPLIT, the production shape, reloading inside its loop; five pixel
    # chunks in the back-substitution and the block pairs
    Scene("hub160_z1", _hub(160, 36, 64, 2, 30, _all(160, 40)), "dense", 789, (159, 0, 0, 1), 1, {40: 159}),
]}

PREPS = {s.id: s for s in [
    Scene("prep_lds_limit", _prep(128, 1022, 41, _BAND128[:7295]), "dense", 7295, (6, 11, 111, 0), 8, ints=38400),   # LDS, 150 KB
    Scene("prep_global_edges", _prep(128, 1022, 41, _BAND128[:7296]), "dense", 7296, (6, 11, 111, 0), 8, ints=38404),
    Scene("prep_global_frames", _prep(12, 4400, 42, E=40), "sparse", 40, (12, 0, 0, 0), 8, ints=39782),   # by the frame count alone
]}

SCENES = {**HUBS, **PREPS}


def scene(sid):
    return SCENES.get(sid) or VARIANTS[sid]


def bars(sid):
    return hs.scene_bars(scene(sid))


def bars_line(sid):
    return hs.scene_bars_line(scene(sid))


def appended_frame(p):
    """`p` with one unused frame appended to every per-frame array (identity pose, disparity 1, no sensor depth): the
    same graph and the same system in a buffer of one frame more."""
    q = copy.copy(p)
    q.poses = np.concatenate([p.poses, np.array([[0, 0, 0, 0, 0, 0, 1]], np.float32)])
    one = np.ones((1,) + p.disps.shape[1:], np.float32)
    q.disps = np.concatenate([p.disps, one])
    q.disps_sens = np.concatenate([p.disps_sens, 0 * one])
    return q


# Copies of table scenes that the GPU tests run beside them (not rows of the tables; bars of their own, same recipe):
#   hub160_tail0        hub160 with the weights of hub 40's second chunk zeroed: the device must notice
#   prep_lds_limit+1    prep_lds_limit in a buffer of 1023 frames: 38409 ints, the same graph through the global path
#   hub160_plain        hub160 before `hover` (CPU only: the dead tail)
VARIANTS = {s.id: s for s in [
    Scene("hub160_tail0", lambda: without(HUBS["hub160"].problem(), chunks(HUBS["hub160"].problem(), 40)[1]), "dense",
          1038, (157, 0, 0, 3), 8, {40: 159, 90: 128, 120: 129}),
    Scene("prep_lds_limit+1", lambda: appended_frame(PREPS["prep_lds_limit"].problem()), "dense", 7295, (6, 11, 111, 0), 8,
          ints=38409),
    Scene("hub160_plain", lambda: plain_hub(*HUB160), "dense", 1038, (157, 0, 0, 3), 8, {40: 159, 90: 128, 120: 129}),
]}
GLOBAL_PREP = ["prep_global_edges", "prep_global_frames", "prep_lds_limit+1"]      # scenes whose tables are built outside LDS
