"""The fp64 roundings of the linearisation's FULL body, held against the ragged body on inputs directed at them.

tests/test_gpu_lin_pinned.py compares the two bodies of ba_lin_kernel on 16 generic graphs.  That holds every fp32 fusion
of the pinned arithmetic, and none of the fp64 ones: a wrong fusion in the point, the Newton steps of 1 / z or ru / rv moves
a result by one fp64 ulp, which survives the rounding to float about once in 10^9 generic evaluations.  The cases of
tests/lin_directed.py are inputs on which it survives at 1 to 10 % of the designated pixels -- at least 16 for each site a
case is meant to expose and each pixel of a lane, proved on the CPU by tests/test_lin_directed.py -- on FULL shapes that
between them run all five FULL instantiations.  profiles/lin_directed.txt lists the single-rounding mutants of the pinned
body these tests catch and the older file does not.

Every directed case is an ordinary BA problem as well, so each also goes through the stage checker against the fp64
oracle at the bars of its graph family (util.STAGE_BARS): points on the principal column and row of the target camera,
residuals at rounding level.
"""
import importlib.util
import os

import pytest

import lin_directed as ld
from lin_hook import assert_bodies_equal, run_lin
from util import HDR_M, HDR_NC1, HDR_NC2, STAGE_BARS, assert_system_close, run_ba_stages, slot_classes, stage_errors

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize("name", list(ld.CASES))
def test_full_body_equals_ragged_body_on_directed_case(backends, name):
    """0 differing 32-bit words in Hpart, Q, w and Ebuf between the two bodies, each on a zeroed workspace of its own.

    Found with these cases: the motion-only instantiations contracted their per-lane relative pose
    differently in the two bodies, 4 words of Hpart on zero_residual-motion_only_16kf_16x32; both now round it in source
    (ba_kernels.hip::lin_rel_pose_pinned)."""
    p, edges, mo, inst, _, _ = ld.build_case(name)
    full, ragged = run_lin(backends, p, mo, 0), run_lin(backends, p, mo, 1)
    assert_bodies_equal(full, ragged, mo, inst, name)


# one graph without E rows, one with, one motion-only; the family whose residuals are already at rounding level
ALONG = ["zero_residual-16kf_64e_16x32", "cancel_x-24kf_band9_16x32", "zero_residual-motion_only_16kf_16x32"]


@pytest.mark.parametrize("name", ALONG)
def test_bodies_agree_along_a_run(backends, name):
    """8 iterations through the phase API; before each, the two bodies linearise the current state and must leave the
    same words (tools/lin_bits_along_run.py::compare_along_run, compared on the device).

    What this can show: a smoke test of converging states.  After the first iteration the state is generic again (the
    update moves every disparity, so the cancellation of cancel_x is gone), and a generic state shows an fp64 rounding
    about once in 10^9 evaluations; the three runs make a few million.  Only the residuals of the zero_residual runs stay
    small, and only as far as eight iterations converge.  The directed cases above are the instrument."""
    spec = importlib.util.spec_from_file_location("lin_bits_along_run", os.path.join(ROOT, "tools", "lin_bits_along_run.py"))
    tool = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(tool)
    p, edges, mo, inst, _, _ = ld.build_case(name)
    res = tool.compare_along_run(backends, p, 8, motion_only=mo, twice=False, log=lambda s: print(f"[{name}] {s}"))
    assert len(res) == 8
    for it, r in enumerate(res):
        assert r["live"]["Hpart"] > 0, (name, it)
        assert (r["size"]["Ebuf"] > 0) == bool(inst[1])
        if not mo:
            assert r["live"]["Q"] == r["size"]["Q"] and r["live"]["w"] > 0, (name, it)
        assert r["diff"] == {k: 0 for k in r["diff"]}, (name, it, r["diff"])


@pytest.mark.parametrize("name", list(ld.CASES))
def test_directed_case_stages_match_oracle(backends, oracle, name):
    """droid_ba_build, the solve and the back-substitution of every directed case against the fp64 oracle from identical
    inputs, as test_gpu_ba_stages.check_graph asserts them: the Schur classes of the graph and the bars of its family."""
    import torch
    p, edges, mo, inst, family, classes = ld.build_case(name)
    st = run_ba_stages(backends, p, torch, motion_only=mo)
    got = slot_classes(st, mo)
    err = stage_errors(oracle, p, st, mo)
    hdr, n3 = st["hdr"], st["hint"][1]
    print(f"[{name}] classes {sorted(got, key=str)} (M={hdr[HDR_M]} nc1={hdr[HDR_NC1]} nc2={hdr[HDR_NC2]} n3={n3}) "
          f"H {err['H']:.2e} b {err['b']:.2e} dx {err['dx']:.2e} state {err['state']:.2e} "
          f"(t {err['state_parts'][0]:.1e} q {err['state_parts'][1]:.1e} d {err['state_parts'][2]:.1e}) "
          f"zero blocks {err['zero_blocks']} stray {err['stray']} dead {err['dead']}")
    assert st["status"] & 15 == 0, st["status"]
    assert got == classes, (name, got, classes)
    if not mo:
        assert st["M"] == p.eta.shape[0]
    b = STAGE_BARS[family]
    assert_system_close(err, b, name)
    assert err["dx"] < b["dx"], (name, err["dx"])
    assert err["state"] < b["state"], (name, err["state_parts"])
