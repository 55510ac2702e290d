"""droid_backends.point_cloud / droid_point_cloud on the device against the fp64 restatement tests/point_cloud_ref.py,
over the cases of tests/point_cloud_cases.py (shown on the CPU to do what they claim: tests/test_point_cloud_cases.py).

Structure: offsets start at 0 and never decrease, a selection outside the buffer owns no row and a zero matrix, src is
strictly increasing inside a selection and lies in [0, hw), a frame selected twice is emitted twice.
Membership: every DECIDED pixel is present exactly when the reference keeps it; the undecided ones (the reference's
count +- its band decisions straddles min_count while the disparity rule holds, or |d - ratio mean| <= 2^-40 mean) stay
within the cap max(2, 1e-3 live pixels).
Points: each against the fp64 value at its own src, per component
    |p - ref| <= 2^-23 |ref| + 2^-40 S,   S = 8 ((|X0x| + |X0y| + 1) / |d| + |t|_1).
Derived, not measured: one float32 rounding with a unit of slack for a tie, plus about 30 fp64 roundings on terms up to S,
below 2^-47 S; the 8 covers the quaternion products at |q| <= 1.01.
Matrices: the pose algebra's tested bound 2^-23 |ref| + 2^-36 (1 + largest |translation component|).
Colours: bit for bit the numpy expression float32(byte) / float32(255)."""
import numpy as np
import pytest

import point_cloud_cases as pcc
import point_cloud_ref

pytestmark = pytest.mark.gpu

CASES = pcc.all_cases()
ONCE = next(c for c in CASES if (c.H, c.W) == (31, 41))
SENT_F, SENT_I = -1234.5, -77


def _torch():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    return torch


def _dev(a):
    return _torch().from_numpy(np.ascontiguousarray(a)).cuda()


@pytest.fixture(scope="module")
def refs():
    """One fp64 reference per case, shared by the tests and left unchanged."""
    return {c.id: point_cloud_ref.point_cloud(c.poses, c.disps, c.K, c.index, c.thresh, c.images, pcc.MIN_COUNT,
                                              pcc.DISP_RATIO) for c in CASES}


def run(backends, case, index=None, thresh=None, images=True, poses=None, sync=True):
    """The Python entry point; every tensor of the result on the host."""
    torch = _torch()
    index = case.index if index is None else index
    thresh = case.thresh if thresh is None else thresh
    if isinstance(thresh, np.ndarray):
        thresh = _dev(thresh)
    pc = backends.point_cloud(_dev(case.poses if poses is None else poses), _dev(case.disps), _dev(case.K), _dev(index),
                              thresh, _dev(case.images) if images else None, pcc.MIN_COUNT, pcc.DISP_RATIO, sync=sync)
    torch.cuda.synchronize()
    out = dict(points=pc.points.cpu().numpy(), colors=None if pc.colors is None else pc.colors.cpu().numpy(),
               src=pc.src.cpu().numpy(), offsets=pc.offsets.cpu().numpy(), matrices=pc.matrices.cpu().numpy(),
               offsets_host=pc.offsets_host)
    return out


def run_abi(backends, case, fill=None):
    """The C entry point on sentinel-filled capacity buffers and a workspace of the caller's, pre-filled with `fill`."""
    torch = _torch()
    lib = backends._lib.load()
    n, h, w = len(case.index), case.H, case.W
    cap = n * h * w
    d = [_dev(x) for x in (case.poses, case.disps, case.K, case.index, np.full(n, case.thresh, np.float32), case.images)]
    points = torch.full((cap, 3), SENT_F, dtype=torch.float32, device="cuda")
    colors = torch.full((cap, 3), SENT_F, dtype=torch.float32, device="cuda")
    src = torch.full((cap,), SENT_I, dtype=torch.int32, device="cuda")
    offsets = torch.full((n + 1,), SENT_I, dtype=torch.int32, device="cuda")
    matrices = torch.full((n, 16), SENT_F, dtype=torch.float32, device="cuda")
    nbytes = lib.droid_point_cloud_workspace_bytes(n, h, w)
    assert nbytes == n * ((h * w + 255) // 256) * 36
    ws = torch.empty(nbytes + 64, dtype=torch.uint8, device="cuda")
    if fill is not None:
        ws.fill_(fill)
    rc = lib.droid_point_cloud(*(t.data_ptr() for t in d), n, pcc.NBUF, h, w, pcc.MIN_COUNT, pcc.DISP_RATIO,
                               points.data_ptr(), colors.data_ptr(), src.data_ptr(), offsets.data_ptr(), matrices.data_ptr(),
                               ws.data_ptr(), nbytes, torch.cuda.current_stream().cuda_stream)
    assert rc == 0, lib.droid_last_error()
    torch.cuda.synchronize()
    if fill is not None:
        assert (ws[nbytes:].cpu().numpy() == fill).all(), "written beyond the workspace"
    return dict(points=points.cpu().numpy(), colors=colors.cpu().numpy(), src=src.cpu().numpy(),
                offsets=offsets.cpu().numpy(), matrices=matrices.cpu().numpy().reshape(n, 4, 4))


def same_bits(a, b, upto=None):
    for k in ("points", "colors", "src", "offsets", "matrices"):
        x, y = a[k], b[k]
        if x is None or y is None:
            assert x is None and y is None, k
            continue
        if upto is not None and k in ("points", "colors", "src"):
            x, y = x[:upto], y[:upto]
        assert x.dtype == y.dtype and x.shape == y.shape, (k, x.dtype, y.dtype, x.shape, y.shape)
        assert np.array_equal(x.view(np.uint8), y.view(np.uint8)), k


@pytest.mark.parametrize("case", CASES, ids=lambda c: c.id)
def test_case_against_the_reference(backends, refs, case):
    ref = refs[case.id]
    got = run(backends, case)
    n, hw = len(case.index), case.H * case.W
    off, src = got["offsets"], got["src"]
    P = int(off[-1])
    # ---- structure
    assert off.dtype == np.int32 and off.shape == (n + 1,) and off[0] == 0 and (np.diff(off) >= 0).all()
    assert got["offsets_host"] == off.tolist()
    assert got["points"].shape == (P, 3) and got["colors"].shape == (P, 3) and src.shape == (P,)
    assert got["points"].dtype == np.float32 and got["colors"].dtype == np.float32 and src.dtype == np.int32
    assert got["matrices"].shape == (n, 4, 4) and got["matrices"].dtype == np.float32
    present = np.zeros((n, hw), bool)
    for b in range(n):
        s = src[off[b]:off[b + 1]]
        if not ref["valid"][b]:
            assert len(s) == 0 and not got["matrices"][b].any()
            continue
        assert (np.diff(s) > 0).all() and (len(s) == 0 or (s[0] >= 0 and s[-1] < hw))
        present[b, s] = True
    b0, b1 = np.nonzero(case.index == 3)[0]
    for k in ("points", "colors", "src"):
        assert np.array_equal(got[k][off[b0]:off[b0 + 1]], got[k][off[b1]:off[b1 + 1]]), k
    assert np.array_equal(got["matrices"][b0], got["matrices"][b1])
    # ---- membership
    keep, und = ref["keep"].reshape(n, hw), ref["undecided"].reshape(n, hw)
    wrong = present != keep
    print(f"[{case.id}] P = {P} (reference {int(keep.sum())}), differing pixels {int(wrong.sum())}, "
          f"undecided {int(und.sum())}, cap {pcc.cap(case.live_pixels)}")
    assert und.sum() <= pcc.cap(case.live_pixels)
    assert not (wrong & ~und).any(), np.argwhere(wrong & ~und)[:8]
    # ---- points, each at its own src
    sel = np.repeat(np.arange(n), np.diff(off))
    want = ref["dense"].reshape(n, hw, 3)[sel, src]
    S = ref["S"].reshape(n, hw)[sel, src]
    err = np.abs(got["points"].astype(np.float64) - want)
    bound = 2.0 ** -23 * np.abs(want) + 2.0 ** -40 * S[:, None]
    print(f"[{case.id}] points: worst error / bound = {(err / bound).max():.3f}")
    assert np.isfinite(got["points"]).all() and (err <= bound).all()
    # ---- matrices
    v = ref["valid"]
    mref = ref["matrices"][v]
    St = 1.0 + np.maximum(np.abs(case.poses[case.index[v], :3].astype(np.float64)).max(1), np.abs(mref[:, :3, 3]).max(1))
    merr = np.abs(got["matrices"][v].astype(np.float64) - mref)
    mbound = 2.0 ** -23 * np.abs(mref) + 2.0 ** -36 * St[:, None, None]
    print(f"[{case.id}] matrices: worst error / bound = {(merr / mbound).max():.3f}")
    assert (merr <= mbound).all()
    assert np.array_equal(got["matrices"][v][:, 3], np.tile(np.float32([0, 0, 0, 1]), (int(v.sum()), 1)))
    # ---- colours, bit for bit
    rgb = case.images[:, [2, 1, 0], 3::8, 3::8].transpose(0, 2, 3, 1).astype(np.float32) / np.float32(255.0)
    frames = np.where(v, case.index, 0)
    assert np.array_equal(got["colors"].view(np.uint32), rgb[frames].reshape(n, hw, 3)[sel, src].view(np.uint32))
    # ---- the stock float32 chain (SE3.inv -> iproj), for the record: printed, not asserted
    torch = _torch()
    Ginv = backends.SE3(_dev(case.poses[case.index[v]])).inv().data
    stock = backends.iproj(Ginv, _dev(case.disps[case.index[v]]), _dev(case.K)).cpu().numpy().reshape(-1, hw, 3)
    live = np.cumsum(v) - 1
    torch.cuda.synchronize()
    serr = np.abs(stock[live[sel], src].astype(np.float64) - want)
    print(f"[{case.id}] stock SE3.inv -> iproj: largest distance from the fp64 points {serr.max():.3e} "
          f"({(serr / bound).max():.1f} bounds); this operator {err.max():.3e}")


def test_capacity_rows_beyond_the_count_are_untouched_and_sync_false(backends, refs):
    case = ONCE
    a = run(backends, case)
    P = int(a["offsets"][-1])
    lazy = run(backends, case, sync=False)
    cap = len(case.index) * case.H * case.W
    assert lazy["offsets_host"] is None and lazy["points"].shape == (cap, 3) and lazy["src"].shape == (cap,)
    same_bits(a, {k: (v[:P] if k in ("points", "colors", "src") else v) for k, v in lazy.items()})
    raw = run_abi(backends, case)
    same_bits(a, raw, upto=P)
    assert 0 < P < cap
    assert (raw["points"][P:].view(np.uint32) == np.float32(SENT_F).view(np.uint32)).all()
    assert (raw["colors"][P:].view(np.uint32) == np.float32(SENT_F).view(np.uint32)).all()
    assert (raw["src"][P:] == SENT_I).all()


def test_two_calls_and_a_dirty_workspace_give_the_same_bits(backends):
    case = ONCE
    a = run(backends, case)
    same_bits(a, run(backends, case))
    P = int(a["offsets"][-1])
    same_bits(a, run_abi(backends, case, fill=0xFF), upto=P)
    same_bits(a, run_abi(backends, case, fill=0x00), upto=P)


def test_negated_quaternions_give_the_same_bits(backends):
    case = ONCE
    poses = case.poses.copy()
    poses[1::2, 3:] *= np.float32(-1.0)
    same_bits(run(backends, case), run(backends, case, poses=poses))


def test_per_selection_thresholds_equal_the_scalar_calls(backends):
    case = ONCE
    n = len(case.index)
    th = np.where(np.arange(n) % 2 == 0, np.float32(case.thresh), np.float32(0.01)).astype(np.float32)
    mixed = run(backends, case, thresh=th)
    scalar = {0: run(backends, case), 1: run(backends, case, thresh=0.01)}
    assert not np.array_equal(scalar[0]["offsets"], scalar[1]["offsets"])
    for b in range(n):
        want = scalar[b % 2]
        for k in ("points", "colors", "src"):
            assert np.array_equal(mixed[k][mixed["offsets"][b]:mixed["offsets"][b + 1]],
                                  want[k][want["offsets"][b]:want["offsets"][b + 1]]), (b, k)
    as_tensor = run(backends, case, thresh=np.full(n, case.thresh, np.float32))
    same_bits(scalar[0], as_tensor)


def test_without_images_and_with_nothing_selected(backends):
    case = ONCE
    a = run(backends, case)
    plain = run(backends, case, images=False)
    assert plain["colors"] is None
    a_no_colors = dict(a, colors=None)
    same_bits(a_no_colors, plain)
    outside = np.array([-1, pcc.NBUF, 2 ** 32 + 3, -2 ** 40, 2 ** 62], dtype=np.int64)
    none = run(backends, case, index=outside)
    assert none["offsets"].tolist() == [0] * 6 == none["offsets_host"] and len(none["points"]) == 0 == len(none["src"])
    assert none["colors"].shape == (0, 3) and not none["matrices"].any()
    empty = run(backends, case, index=np.zeros(0, np.int64))
    assert empty["offsets"].tolist() == [0] and empty["points"].shape == (0, 3) and empty["matrices"].shape == (0, 4, 4)


def test_more_selections_than_one_grid_dimension_holds(backends):
    """n = 65 541 selections cycling over the frames of the 8 x 8 case (and two indices outside it): every block of rows
    equals the first occurrence of its frame."""
    case = CASES[0]
    assert (case.H, case.W) == (8, 8)
    n = 65541
    index = (np.arange(n) % (pcc.NBUF + 2) - 1).astype(np.int64)     # -1, 0 .. 8, 9, -1, ...
    got = run(backends, case, index=index)
    off = got["offsets"].astype(np.int64)
    rows = np.diff(off)
    first = {int(f): b for b, f in reversed(list(enumerate(index[:pcc.NBUF + 2])))}
    assert off[0] == 0 and (rows >= 0).all() and off[-1] == len(got["points"])
    per_frame = np.array([rows[first[int(f)]] for f in range(-1, pcc.NBUF + 1)])
    assert np.array_equal(rows, per_frame[index + 1]) and per_frame[0] == 0 == per_frame[-1] and (per_frame[1:-1] > 0).all()
    for f in range(pcc.NBUF):
        blocks = np.nonzero(index == f)[0]
        b0 = first[f]
        want = {k: got[k][off[b0]:off[b0 + 1]] for k in ("points", "colors", "src")}
        idx = (off[blocks][:, None] + np.arange(rows[b0])[None]).reshape(-1)
        for k in ("points", "colors", "src"):
            assert np.array_equal(got[k][idx].reshape((len(blocks),) + want[k].shape), np.broadcast_to(want[k], (len(blocks),) + want[k].shape)), (f, k)
        assert (got["matrices"][blocks] == got["matrices"][b0]).all()
    assert not got["matrices"][(index < 0) | (index >= pcc.NBUF)].any()
