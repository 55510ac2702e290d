"""The reduced camera system at the shapes and graphs where the linearisation (ba_lin_kernel) and the assemble step
change path: ragged and full pixel chunks, waves without a pixel, edge ranges (zsplit > 1), a stereo edge, the E-row
instantiation of dense graphs -- with depth slots and motion-only (linearisation + assemble alone).
The bar is the one of test_gpu_ba.py::test_reduced_system_matches_oracle: relative 2e-6 on H and on b."""
import numpy as np
import pytest

from util import ba_args, run_ba_stages

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def synth():
    from droid_backends import synth
    return synth


# H x W: pixels, what it exercises (512 pixels per chunk, 128 per wave, 2 per lane)
SHAPES = {
    "5x7": (5, 7),       # 35: one partial wave, three waves with no pixel
    "16x24": (16, 24),   # 384: the second pixel of half the lanes is missing
    "24x32": (24, 32),   # 768: one full and one half chunk
    "32x48": (32, 48),   # 1536: the full-chunk body
}


def _pairs(pairs):
    pairs = list(pairs)
    return [a for a, _ in pairs], [b for _, b in pairs]


def _star(synth, H, W):
    """18 edges leaving frame 1 of 19: few slots, so every (slot, chunk) is split into edge ranges that start mid-slot"""
    return synth.make_ba_problem(N=19, H=H, W=W, seed=31, edges=_pairs((1, j) for j in range(19) if j != 1))


def _tiny(synth, H, W):
    """3 keyframes / 4 edges: zsplit > 1"""
    return synth.make_ba_problem(N=3, E=4, H=H, W=W, seed=11)


def _stereo(synth, H, W):
    """the 3-keyframe band and one stereo edge (1, 1)"""
    return synth.make_ba_problem(N=3, H=H, W=W, seed=12, edges=_pairs([(0, 1), (1, 0), (1, 2), (2, 1), (1, 1)]))


def _wide(synth, H, W):
    """all pairs of 18 frames: E = 306 >= 12 M = 216 (the E-row instantiation where HW % 32 == 0), 17 edges per slot"""
    return synth.make_ba_problem(N=18, H=H, W=W, seed=33, lm=1e-4, ep=0.1,
                                 edges=_pairs((i, j) for i in range(18) for j in range(18) if i != j))


GRAPHS = {"star18": _star, "3kf4e": _tiny, "stereo_edge": _stereo, "wide18": _wide}


@pytest.mark.parametrize("motion_only", [False, True], ids=["depth", "motion_only"])
@pytest.mark.parametrize("graph", list(GRAPHS))
@pytest.mark.parametrize("shape", list(SHAPES))
def test_reduced_system_at_shape(backends, oracle, synth, shape, graph, motion_only):
    import torch
    H, W = SHAPES[shape]
    p = GRAPHS[graph](synth, H, W)
    ref = oracle.ba(*ba_args(p), 1, p.lm, p.ep, motion_only, debug=True)
    st = run_ba_stages(backends, p, torch, motion_only=motion_only)
    n = 6 * (p.t1 - p.t0)
    sys_ = st["system"]
    Hd, Ho = np.tril(sys_[:n, :n]), np.tril(ref["H"])
    eh = np.abs(Hd - Ho).max() / np.abs(Ho).max()
    eb = np.abs(sys_[n, :n] - ref["b"]).max() / np.abs(ref["b"]).max()
    print(f"{shape} {graph} motion_only={motion_only}: rel err H {eh:.2e}  b {eb:.2e}")
    assert st["status"] & 1 == 0
    assert eh < 2e-6 and eb < 2e-6
