"""The cases of tests/point_cloud_cases.py do what they claim, shown on the CPU with the fp64 reference alone
(oracle.geom.depth_filter with its margins, through tests/point_cloud_ref.py): a useful share of the live pixels is
kept, a useful share is dropped by the disparity rule ALONE (its count would have kept it), every count 0 .. 6 occurs,
every selection inside the buffer keeps something, and the undecided pixels stay within the cap."""
import numpy as np
import pytest

import point_cloud_cases as pcc
import point_cloud_ref

CASES = pcc.all_cases()


@pytest.fixture(scope="module")
def refs():
    return {c.id: point_cloud_ref.point_cloud(c.poses, c.disps, c.K, c.index, c.thresh, c.images, pcc.MIN_COUNT,
                                              pcc.DISP_RATIO) for c in CASES}


def test_table_and_index():
    assert [(c.H, c.W) for c in CASES] == [(8, 8), (9, 19), (17, 24), (31, 41), (48, 64), (48, 64)]
    ix = pcc.INDEX
    inside = (ix >= 0) & (ix < pcc.NBUF)
    assert inside.sum() == pcc.LIVE and (~inside).sum() == 3 and 2 ** 32 + 3 in ix and -1 in ix and pcc.NBUF in ix
    assert (ix == 3).sum() == 2 and 0 in ix and pcc.NBUF - 1 in ix and (np.diff(ix[inside]) < 0).any()
    # one wave of a 4-wave tile; a ragged tile; a ragged last wave; twelve full tiles
    assert 8 * 8 == 64 and (9 * 19) % 256 != 0 and 31 * 41 == 19 * 64 + 55 and 48 * 64 == 12 * 256
    for c in CASES:
        assert c.poses.dtype == np.float32 and c.disps.dtype == np.float32 and c.images.dtype == np.uint8
        assert np.allclose(np.linalg.norm(c.poses[:, 3:], axis=1), 1.0, atol=1e-6) and (c.disps > 0).all()
        assert c.images.shape == (pcc.NBUF, 3, 8 * c.H, 8 * c.W) and c.live_pixels == pcc.LIVE * c.H * c.W


@pytest.mark.parametrize("case", CASES, ids=lambda c: c.id)
def test_case_properties(case, refs):
    r = refs[case.id]
    v = r["valid"]
    live = case.live_pixels
    kept = r["keep"].sum() / live
    by_rule_alone = ((r["count"] >= pcc.MIN_COUNT) & ~r["rule"] & v[:, None, None]).sum() / live
    hist = np.bincount(r["count"][v].astype(int).ravel(), minlength=7)
    undecided = int(r["undecided"].sum())
    print(f"[{case.id}] kept {kept:.3f}, dropped by the disparity rule alone {by_rule_alone:.3f}, counts {hist.tolist()}, "
          f"undecided {undecided} of {live} (cap {pcc.cap(live)})")
    assert 0.52 <= kept <= 0.80
    assert 0.08 <= by_rule_alone <= 0.31
    assert len(hist) == 7 and (hist > 0).all()
    assert undecided <= pcc.cap(live)
    rows = np.diff(r["offsets"])
    assert (rows[v] > 0).all() and (rows[~v] == 0).all() and r["offsets"][-1] == r["keep"].sum()
    assert not r["keep"][~v].any() and not r["undecided"][~v].any()
