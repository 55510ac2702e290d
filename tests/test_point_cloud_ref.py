"""tests/point_cloud_ref.py equals the stock lines of the viewers (visualization.py:100-142) written independently:
points = iproj(SE3(poses).inv(), disps)[mask] with mask = (depth_filter(...) >= 2) & (disps > .5 * mean) by boolean
indexing frame by frame, colours = images[:, [2,1,0], 3::8, 3::8] / 255 under the same mask -- in the order of the
index, duplicates emitted twice, indices outside the buffer contributing nothing."""
import numpy as np
import pytest

import point_cloud_cases as pcc
import point_cloud_ref
import se3_ref
from oracle import geom

CASES = [c for c in pcc.all_cases() if c.H <= 31]


def stock(case, index, thresh):
    """The viewer's loop on the host, for the selections inside the buffer (index_select would raise on the others)."""
    poses, disps = case.poses[index], case.disps[index].astype(np.float64)
    Ps = se3_ref.matrix(se3_ref.inv(poses))
    images = case.images[index][:, [2, 1, 0], 3::8, 3::8].transpose(0, 2, 3, 1).astype(np.float32) / np.float32(255.0)
    points = geom.iproj(se3_ref.inv(poses), disps, case.K)
    count = geom.depth_filter(case.poses, case.disps, case.K, index, thresh)
    masks = (count >= 2) & (disps > .5 * disps.mean(axis=(1, 2), keepdims=True))
    pts, clr = [], []
    for i in range(len(index)):
        pts.append(points[i].reshape(-1, 3)[masks[i].reshape(-1)])
        clr.append(images[i].reshape(-1, 3)[masks[i].reshape(-1)])
    return pts, clr, Ps, masks


@pytest.mark.parametrize("case", CASES, ids=lambda c: c.id)
def test_restatement_equals_the_stock_lines(case):
    r = point_cloud_ref.point_cloud(case.poses, case.disps, case.K, case.index, case.thresh, case.images)
    inside = (case.index >= 0) & (case.index < pcc.NBUF)
    assert np.array_equal(r["valid"], inside)
    pts, clr, Ps, masks = stock(case, case.index[inside], np.full(int(inside.sum()), case.thresh))
    off = r["offsets"]
    assert off[0] == 0 and len(off) == len(case.index) + 1 and off[-1] == len(r["points"]) == len(r["src"]) == len(r["colors"])
    j = 0
    for b, ok in enumerate(inside):
        rows = slice(off[b], off[b + 1])
        if not ok:
            assert off[b + 1] == off[b] and not r["matrices"][b].any()
            continue
        assert np.array_equal(r["keep"][b], masks[j])
        assert np.array_equal(r["src"][rows], np.nonzero(masks[j].reshape(-1))[0])
        assert np.abs(r["points"][rows] - pts[j]).max() <= 1e-12
        assert r["colors"].dtype == np.float32 and np.array_equal(r["colors"][rows], clr[j])
        assert np.abs(r["matrices"][b] - Ps[j]).max() <= 1e-15 * max(1.0, np.abs(Ps[j]).max())
        j += 1
    # the two selections of frame 3 are emitted twice, identically
    b0, b1 = np.nonzero(case.index == 3)[0]
    assert off[b0 + 1] - off[b0] == off[b1 + 1] - off[b1] > 0
    assert np.array_equal(r["points"][off[b0]:off[b0 + 1]], r["points"][off[b1]:off[b1 + 1]])


def test_order_threshold_forms_and_options():
    case = CASES[1]
    base = point_cloud_ref.point_cloud(case.poses, case.disps, case.K, case.index, case.thresh, case.images)
    # a reversed index reverses the blocks, nothing else
    rev = point_cloud_ref.point_cloud(case.poses, case.disps, case.K, case.index[::-1], case.thresh, case.images)
    n = len(case.index)
    for b in range(n):
        a = slice(base["offsets"][b], base["offsets"][b + 1])
        c = slice(rev["offsets"][n - 1 - b], rev["offsets"][n - b])
        assert np.array_equal(base["points"][a], rev["points"][c]) and np.array_equal(base["src"][a], rev["src"][c])
    # a per-selection threshold is the scalar calls selection by selection
    th = np.where(np.arange(n) % 2 == 0, 0.1, 0.03).astype(np.float32)
    mixed = point_cloud_ref.point_cloud(case.poses, case.disps, case.K, case.index, th)
    other = point_cloud_ref.point_cloud(case.poses, case.disps, case.K, case.index, 0.03)
    for b in range(n):
        want = base if b % 2 == 0 else other
        assert np.array_equal(mixed["keep"][b], want["keep"][b])
    assert mixed["colors"] is None and (mixed["keep"] != base["keep"]).any()
    # min_count and disp_ratio are what the rule says
    loose = point_cloud_ref.point_cloud(case.poses, case.disps, case.K, case.index, case.thresh, min_count=0, disp_ratio=0.0)
    assert loose["keep"][loose["valid"]].all() and not loose["keep"][~loose["valid"]].any()
    none = point_cloud_ref.point_cloud(case.poses, case.disps, case.K, case.index, case.thresh, min_count=7)
    assert none["offsets"][-1] == 0 and len(none["points"]) == 0
    outside = point_cloud_ref.point_cloud(case.poses, case.disps, case.K, np.array([-1, 9, 2 ** 32 + 3]), case.thresh)
    assert not outside["offsets"].any() and not outside["matrices"].any()
