"""The two bodies of the BA linearisation (ba_kernels.hip::ba_lin_kernel) leave the same bits.

Where H*W is a multiple of the 512-pixel chunk the product runs the FULL body: no pixel guard, both pixels of a lane in
one basic block, the roundings of the per-pixel arithmetic pinned in source (every fused multiply-add written as fma,
contraction off).  The ragged body is the per-lane guarded one, whose fusions the compiler chooses.  The test hook
droid_test_ba_lin (include/droid_test_hooks_hip.h) runs the linearisation alone on a prepared workspace, with either
body, and copies out what it leaves there: Hpart (per-wave partial Hjj / vj), Q = 1 / C, w and, on dense graphs, the E
rows.  Every case asks for 0 differing 32-bit words between the two bodies, each on a zeroed workspace of its own.

The cases are the smallest shapes at which each path exists; between them they run all five FULL instantiations the
dispatch can choose (depth slots with / without E rows, each with / without edge ranges, and motion-only), which
test_cases_reach_every_full_instantiation holds against a restatement of the host's choice and every GPU case against
the choice the library reports (E rows kept, edge ranges: words 4 and 5 of the hook's size query).
"""
import ctypes
import os
import re

import numpy as np
import pytest

import hard_scenes as hs
import stage_graphs as sg
from lin_hook import LIN_CP, instantiation, run_lin

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _band(N, reach):
    return sg._edges(sg._band(N, reach))


def _motion(synth, H, W):
    p = synth.make_ba_problem(N=10, E=36, H=H, W=W, seed=7)
    keep = (p.ii < 6) & (p.jj >= 6)
    p.ii, p.jj, p.targets, p.weights = p.ii[keep], p.jj[keep], p.targets[keep], p.weights[keep]
    p.t0, p.t1 = 6, 10
    return p


def _hard_window(synth, H, W, rot):
    seed = H * 1009 + W * 31 + int(rot) * 7
    return hs.harden(synth.make_ba_problem(N=8, E=32, H=H, W=W, seed=seed), seed + 1, rot, "plain")


# name -> (builder(synth), motion_only, the instantiation it must reach: (depth, E rows, edge ranges))
CASES = {
    "3kf_4e_16x32": (lambda s: s.make_ba_problem(N=3, E=4, H=16, W=32, seed=11), False, (1, 0, 1)),
    "8kf_32e_16x32": (lambda s: s.make_ba_problem(N=8, E=32, H=16, W=32, seed=2), False, (1, 0, 1)),
    "8kf_32e_32x48": (lambda s: s.make_ba_problem(N=8, E=32, H=32, W=48, seed=2), False, (1, 0, 1)),
    "36kf_1200e_16x32": (lambda s: s.make_ba_problem(N=36, E=1200, H=16, W=32, seed=77, lm=1e-4, ep=0.1), False, (1, 1, 1)),
    "130kf_1600e_16x32": (lambda s: s.make_ba_problem(N=130, E=1600, H=16, W=32, seed=5, lm=1e-4, ep=0.1), False, (1, 1, 1)),
    # more than 768 (slot, chunk) pairs: one workgroup per pair, no edge ranges -- the headline's instantiation ...
    "260kf_800e_32x48": (lambda s: s.make_ba_problem(N=260, E=800, H=32, W=48, seed=3), False, (1, 0, 0)),
    # ... and the same with E rows: 18 edges per slot, every slot served by the SYRK kernels
    "260kf_band9_32x48": (lambda s: s.make_ba_problem(N=260, H=32, W=48, seed=4, lm=1e-4, ep=0.1, edges=_band(260, 9)),
                          False, (1, 1, 0)),
    "motion_only_10kf_36e_32x48": (lambda s: _motion(s, 32, 48), True, (0, 0, 0)),
    "stereo_8kf_32e_16x32": (lambda s: s.make_ba_problem(N=8, E=32, H=16, W=32, seed=6, stereo=True), False, (1, 0, 1)),
    "stereo_pairs_24kf_band9_16x32": (lambda s: s.make_ba_problem(N=24, H=16, W=32, seed=21, lm=1e-4, ep=0.1,
                                                                  edges=sg._edges(sg._band(24, 9) | {(i, i) for i in range(24)})),
                                      False, (1, 1, 1)),
    "rgbd_8kf_32e_16x32": (lambda s: s.make_ba_problem(N=8, E=32, H=16, W=32, seed=8, rgbd=True), False, (1, 0, 1)),
    "rgbd_24kf_band9_16x32": (lambda s: s.make_ba_problem(N=24, H=16, W=32, seed=21, lm=1e-4, ep=0.1, rgbd=True,
                                                          edges=_band(24, 9)), False, (1, 1, 1)),
    # scenes with points behind MIN_DEPTH and targets outside the image (tests/hard_scenes.py)
    "hard_window_16x32_rot20": (lambda s: _hard_window(s, 16, 32, 20.0), False, (1, 0, 1)),
    "hard_window_16x32_rot60": (lambda s: _hard_window(s, 16, 32, 60.0), False, (1, 0, 1)),
    "hard_dense36_syrk": (lambda s: hs.SCENES["hard_dense36_syrk"].problem(), False, (1, 1, 1)),
    "hard_motion_only": (lambda s: hs.SCENES["hard_motion_only"].problem(), True, (0, 0, 0)),
}


@pytest.fixture(scope="module")
def synth():
    from droid_backends import synth
    return synth


def test_cases_reach_every_full_instantiation(synth):
    got = set()
    for name, (build, mo, inst) in CASES.items():
        p = build(synth)
        _, H, W = p.disps.shape
        assert (H * W) % LIN_CP == 0, name          # the product runs the FULL body on it
        assert instantiation(p, mo) == inst, (name, instantiation(p, mo))
        got.add(inst)
    assert got == {(1, 0, 0), (1, 0, 1), (1, 1, 0), (1, 1, 1), (0, 0, 0)}


def test_hook_table_matches_its_header(backends):
    """include/droid_test_hooks_hip.h against _lib.ABI_TEST, class by class, as tests/test_abi.py holds the main header."""
    txt = open(os.path.join(ROOT, "include", "droid_test_hooks_hip.h")).read()
    txt = re.sub(r"//[^\n]*", "", re.sub(r"/\*.*?\*/", "", txt, flags=re.S))

    def cls(decl, is_param):
        if "*" in decl:
            return "pointer"
        words = decl.replace("const", " ").split()
        words = words[:-1] if is_param else words
        assert len(words) == 1 and words[0] in ("int", "int64_t", "size_t", "float", "double"), decl
        return words[0]

    protos = {}
    for res, name, params in re.findall(r"([A-Za-z_][\w \t\*]*?)\b(droid_[a-z0-9_]+)\s*\(([^()]*)\)\s*;", txt):
        assert name not in protos, name
        protos[name] = (cls(res, False), [cls(q.strip(), True) for q in params.split(",")])
    assert sorted(protos) == sorted(backends._lib.ABI_TEST) == ["droid_test_ba_lin"]
    assert hasattr(ctypes.CDLL(backends._lib.LIB_PATH), "droid_test_ba_lin")     # load() binds it but does not require it
    assert not set(protos) & (set(backends._lib.ABI) | set(backends._lib.ABI_UPDATE))
    of_ctype = {ctypes.c_int: "int", ctypes.c_int64: "int64_t", ctypes.c_size_t: "size_t", ctypes.c_float: "float",
                ctypes.c_double: "double", ctypes.c_void_p: "pointer"}
    lib = backends._lib.load()
    for name, (res, params) in protos.items():
        restype, argtypes = backends._lib.signature(name)
        assert of_ctype[restype] == res, name
        assert [of_ctype.get(a) or ("pointer" if issubclass(a, ctypes._Pointer) else None) for a in argtypes] == params, name
        fn = getattr(lib, name)
        assert fn.restype == restype and list(fn.argtypes) == argtypes, name
    rc = lib.droid_test_ba_lin(*([None] * 9), 4, 8, 16, 32, 8, 5, 3, 0, 0, None, 0, None, None, None, None, None, None)
    assert rc == -1 and b"window" in lib.droid_last_error()          # refused on the host, no GPU needed


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(CASES))
def test_full_body_equals_ragged_body(backends, synth, name):
    build, mo, inst = CASES[name]
    p = build(synth)
    full, ragged = run_lin(backends, p, mo, 0), run_lin(backends, p, mo, 1)
    diff = {k: int((full[k] != ragged[k]).sum()) for k in full}
    live = {k: int((ragged[k] != 0).sum()) for k in ragged}
    print(f"[{name}] instantiation {inst}: differing words " + "  ".join(f"{k} {diff[k]} of {full[k].size}" for k in full)
          + f"   (non-zero words: {live})")
    assert live["Hpart"] > 0                       # the launch ran and wrote its sums
    if not mo:
        assert live["Q"] == full["Q"].size and live["w"] > 0
    assert (full["Ebuf"].size > 0) == bool(inst[1])
    if inst[1]:
        assert live["Ebuf"] > 0                    # some slot of the graph has its E rows stored
    assert diff == {k: 0 for k in diff}, diff
