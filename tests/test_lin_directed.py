"""The directed cases of tests/lin_directed.py discriminate: a condition on the inputs, checked on the CPU.

For every case and every rounding site the case is meant to expose, the number of designated pixels at which flipping
that one site of the fp64 arithmetic changes a float the kernel reads (x, y, d, ru, rv) is at least 16, for each of the
two pixels of a lane on its own -- so that a wrong fusion at that site cannot pass tests/test_gpu_lin_directed.py by
luck.  On generic inputs the same count is 0 (test_generic_inputs_do_not_discriminate: the reason these cases exist).
"""
from fractions import Fraction

import numpy as np
import pytest

import lin_directed as ld
from lin_hook import FULL_INSTANTIATIONS, LIN_CP, instantiation

MIN_COUNT = 16


def test_fma_is_exact():
    rng = np.random.default_rng(0)
    for _ in range(2000):
        a, b = (float(v) for v in rng.normal(0, 1, 2) * 2.0 ** rng.integers(-30, 30, 2))
        c = -a * b * (1 + float(rng.integers(-4, 5)) * 2.0 ** -52) if rng.uniform() < 0.5 else float(rng.normal())
        exact = Fraction(a) * Fraction(b) + Fraction(c)
        assert ld.fma(a, b, c) == float(exact), (a, b, c)      # float(Fraction) rounds once, ties to even
    assert ld.fma(3.0, 0.0, 5.0) == 5.0 and ld.fma(3.0, 2.0, 0.0) == 6.0
    # multiply-then-add meets a tie here and rounds down; the exact sum lies 2^-104 above the tie
    a = 1 + 2.0 ** -52
    assert ld.fma(a, a, 2.0 ** -53) == 1 + 2.0 ** -51 + 2.0 ** -52 != a * a + 2.0 ** -53


def test_cases_reach_every_full_instantiation():
    for fam in ld.FAMILIES:
        got = set()
        for name, (f, g) in ld.CASES.items():
            if f != fam:
                continue
            p, edges, mo, inst, _, _ = ld.build_case(name)
            _, H, W = p.disps.shape
            assert (H * W) % LIN_CP == 0, name                  # the product runs the FULL body on it
            assert instantiation(p, mo) == inst, (name, instantiation(p, mo))
            got.add(inst)
        assert got == FULL_INSTANTIATIONS, (fam, got)


@pytest.mark.parametrize("name", list(ld.CASES))
def test_designated_edges_are_sound(name):
    """Whole edges, one per source frame, no stereo pair; every designated pixel in front of the camera by a margin
    (no case leans on the MIN_DEPTH rule), finite positive disparities everywhere, positive weights where the family
    keeps them and zeros where it says so; the other edges keep weights of ordinary size."""
    p, edges, mo, inst, _, _ = ld.build_case(name)
    fam = ld.CASES[name][0]
    assert len(edges) >= 4 and len({int(p.ii[e]) for e in edges}) == len(edges)
    assert all(int(p.ii[e]) != int(p.jj[e]) for e in edges)
    assert np.all(np.isfinite(p.disps)) and p.disps.min() > 0
    for a in (p.poses, p.targets, p.weights, p.intrinsics):
        assert np.all(np.isfinite(a))
    for e in edges:
        x, y, z = ld.point(p, e)
        assert z.min() >= 0.5, (name, e, z.min())
        w = p.weights[e]
        if fam == "cancel_x":
            assert w[0].min() > 0 and not w[1].any()
            assert np.abs(x).max() < 2.0 ** -22 * np.abs(p.disps[int(p.ii[e])]).max()      # xd is a rounding residue
        elif fam == "cancel_y":
            assert w[1].min() > 0 and not w[0].any()
            assert np.abs(y).max() < 2.0 ** -22 * np.abs(p.disps[int(p.ii[e])]).max()
        else:
            assert w.min() > 0
            fx, fy, cx, cy = (float(k) for k in p.intrinsics)
            t = p.targets[e].reshape(2, -1).astype(np.float64)
            assert np.abs(t[0] - (fx * x / z + cx)).max() < 2.0 ** -23 * max(np.abs(t[0]).max(), 1.0)
            assert np.abs(t[1] - (fy * y / z + cy)).max() < 2.0 ** -23 * max(np.abs(t[1]).max(), 1.0)
    others = np.setdiff1d(np.arange(len(p.ii)), edges)
    assert (p.weights[others] > 0).mean() > 0.5, name         # b and H keep their ordinary scale


@pytest.mark.parametrize("name", list(ld.CASES))
def test_cases_discriminate(name):
    p, edges, mo, inst, _, _ = ld.build_case(name)
    fam = ld.CASES[name][0]
    sites = ld.FAMILIES[fam][1]
    counts, zmin = ld.discrimination(p, edges, inst, sites)
    n = len(edges) * p.disps.shape[1] * p.disps.shape[2] // 2
    print(f"[{name}] designated edges {edges}, {n} pixels per pixel-of-lane, min zd {zmin:.3f}; floats changed by one site"
          " (pixel-of-lane 0 / 1): " + "  ".join(f"{s} {c[0]}/{c[1]}" for s, c in counts.items()))
    assert zmin >= 0.5
    for s, c in counts.items():
        assert min(c) >= MIN_COUNT, (name, s, c)


def test_generic_inputs_do_not_discriminate():
    """The same count on the generator's own edges of one graph: why volume is the wrong instrument."""
    from droid_backends import synth
    make, mo, inst, _, _ = ld.GRAPHS["16kf_64e_16x32"]
    p = make(synth)
    edges = ld._designate(p, 4, lambda e: bool(ld.point(p, e)[2].min() > 0.75))
    counts, _ = ld.discrimination(p, edges, inst, ld.SITES)
    print("generic edges: " + "  ".join(f"{s} {c[0]}/{c[1]}" for s, c in counts.items()))
    assert sum(sum(c) for c in counts.values()) <= 2
