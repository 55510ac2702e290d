"""The graphs of the stage-by-stage BA parity harness (tests/test_gpu_ba_stages.py), with the Schur classes each one must
exercise.  Classes (ba_kernels.hip::schur_class): 0 = the sparse kernel (ba_schur2_kernel + fold), 1 / 2 = the two SYRK
instances of dense graphs, 3 = block pairs (ba_schur_fused_kernel<true>); "motion" = motion-only, no Schur complement."""
import numpy as np


def _band(N, reach):
    return {(i, j) for i in range(N) for d in range(1, reach + 1) for j in (i - d, i + d) if 0 <= j < N}


def _edges(pairs):
    pairs = sorted(pairs)
    return [a for a, _ in pairs], [b for _, b in pairs]


def every_class(synth, seed=11):
    """test_gpu_ba_full.py::test_dense_graph_with_every_schur_class: border frames (sparse), the bulk (SYRK class 1),
    a hub with 68 edges (class 2) and one connected to every other frame (class 3)."""
    N = 100
    pairs = _band(N, 9) | {(10, j) for j in range(0, N, 2) if j != 10} | {(20, j) for j in range(N) if j != 20}
    return synth.make_ba_problem(N=N, H=8, W=16, seed=seed, lm=1e-4, ep=0.1, edges=_edges(pairs))


def variant(synth, name):
    """test_gpu_ba_full.py::test_dense_graph_variants."""
    N = 24
    pairs = _band(N, 9)
    kw = dict(N=N, H=8, W=32, seed=21, lm=1e-4, ep=0.1)
    if name == "window_inside_buffer":
        kw.update(nbuf=30, t0=3)
    elif name == "rgbd":
        kw.update(rgbd=True)
    else:
        pairs |= {(i, i) for i in range(N)}
    return synth.make_ba_problem(edges=_edges(pairs), **kw)


def motion_only(synth):
    """test_gpu_ba.py::test_ba_motion_only: new frames [6,10) observed from fixed keyframes."""
    p = synth.make_ba_problem(N=10, E=36, H=48, W=64, seed=7)
    keep = (p.ii < 6) & (p.jj >= 6)
    p.ii, p.jj = p.ii[keep], p.jj[keep]
    p.targets, p.weights = p.targets[keep], p.weights[keep]
    p.t0, p.t1 = 6, 10
    return p


# name -> (builder(synth), family of the tolerance bars, Schur classes the device must report -- exactly)
GRAPHS = {
    "cfg1": (lambda s: s.make_config("cfg1"), "sparse", {0}),
    "cfg2": (lambda s: s.make_config("cfg2"), "sparse", {0}),
    "cfg3": (lambda s: s.make_config("cfg3"), "sparse", {0}),
    "cfg3_seed12": (lambda s: s.make_config("cfg3", seed=12), "sparse", {0}),
    "cfg3_seed22": (lambda s: s.make_config("cfg3", seed=22), "sparse", {0}),
    "cfg4": (lambda s: s.make_config("cfg4"), "wide", {1, 2}),
    "cfg5": (lambda s: s.make_config("cfg5"), "stereo", {0}),
    "dense36_syrk": (lambda s: s.make_ba_problem(N=36, E=1200, H=16, W=32, seed=77, lm=1e-4, ep=0.1), "dense", {1}),
    "dense30_block_pair": (lambda s: s.make_ba_problem(N=30, E=720, H=15, W=20, seed=78, lm=1e-4, ep=0.1), "dense", {3}),
    "dense20_few_stages": (lambda s: s.make_ba_problem(N=20, E=330, H=8, W=16, seed=5, lm=1e-4, ep=0.1), "dense", {0, 1}),
    "every_class": (lambda s: every_class(s), "dense", {0, 1, 2, 3}),
    "every_class_seed12": (lambda s: every_class(s, 12), "dense", {0, 1, 2, 3}),
    "every_class_seed13": (lambda s: every_class(s, 13), "dense", {0, 1, 2, 3}),
    "variant_window_t0_3": (lambda s: variant(s, "window_inside_buffer"), "dense", {0, 1}),
    "variant_rgbd": (lambda s: variant(s, "rgbd"), "dense", {0, 1}),
    "variant_stereo_pairs": (lambda s: variant(s, "stereo_pairs"), "dense", {0, 1}),
    "motion_only": (lambda s: motion_only(s), "motion", {"motion"}),
}


def predicted_classes(p, S2_MAXE=16, SW_MID=256, SW_BIG=512, SLOT_MAXE=128, own=None):
    """Host restatement of ba_prep_kernel's slot classes (used to write the table above; the tests assert what the
    DEVICE reports, not this).  own: the frame range of a shard whose edges `p` holds (default: the whole buffer)."""
    nbuf, H, W = p.disps.shape
    w0, w1 = (p.t0, p.t1) if own is None else (max(p.t0, own[0]), min(p.t1, own[1]))
    kx = np.unique(np.concatenate([np.arange(w0, max(w0, w1)), p.ii])).astype(np.int64)
    M, E = len(kx), len(p.ii)
    wide = M > 0 and E >= 12 * M and (H * W) % 32 == 0
    out = []
    for f in kx:
        ne = int((p.ii == f).sum())
        nent = int(w0 <= f < w1) + int(((p.ii == f) & (p.jj >= p.t0) & (p.jj < p.t1)).sum())
        rows = 6 * nent + 1
        if nent == 0 or ne <= S2_MAXE:
            out.append(0)
        elif not wide or ne > SLOT_MAXE or rows > SW_BIG:
            out.append(3)
        else:
            out.append(1 if rows <= SW_MID else 2)
    return np.bincount(out, minlength=4)
