"""tests/gru_ref.py's exact module held to the reference's own ConvGRU: tests/golden/reference_gru.npz holds what
droid_slam/modules/gru.py returns in float64 (tests/golden/make_gru_golden.py).  The inputs come from the seeds and are
checked against the fixture's SHA-256; where the reference's checkout exists the fixture is regenerated and compared."""
import importlib.util
import os

import numpy as np
import pytest

import gru_ref
import reference_programs

HERE = os.path.dirname(os.path.abspath(__file__))
FIXTURE = os.path.join(HERE, "golden", "reference_gru.npz")
spec = importlib.util.spec_from_file_location("make_gru_golden", os.path.join(HERE, "golden", "make_gru_golden.py"))
gen = importlib.util.module_from_spec(spec)
spec.loader.exec_module(gen)


@pytest.mark.parametrize("case", gen.CASES, ids=lambda c: c[0])
def test_exact_module_matches_the_references_own_module(case):
    fix = np.load(FIXTURE)
    params, ops = gen.inputs_of(case)
    assert str(fix["sha_" + case[0]]) == gen.digest(params, ops)          # the fixture was made from these inputs
    want = fix["out_" + case[0]]
    got = gru_ref.exact(params, ops[0], ops[1:])["out"]
    assert want.dtype == np.float64 and got.shape == want.shape
    assert np.abs(got - want).max() <= 1e-13


@pytest.mark.skipif(not reference_programs.available(), reason=reference_programs.SKIP_REASON)
def test_the_fixture_is_what_the_reference_computes_today():
    fix, new = np.load(FIXTURE), gen.generate()
    assert sorted(fix.files) == sorted(new)
    for k in new:
        if k.startswith("sha_"):
            assert str(fix[k]) == str(new[k])
        else:
            assert np.abs(fix[k] - new[k]).max() <= 1e-13
