"""Convex upsampling on the device (droid_cvx_upsample through droid_backends.cvx_upsample / upsample_disps) against the
fp64 restatement of its contract (tests/cvx_upsample_ref.py): every output pixel within 32 u nb, one-hot masks bit for
bit, the indexed in-place write between sentinel guards, determinism, independence of the batch, the distance from the
stock torch chain a user sees when switching, and the call DepthVideo.upsample would make."""
import numpy as np
import pytest
import torch

import cvx_upsample_ref as cr

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
TABLE = [(c, s) for c in range(len(cr.CASES)) for s in cr.SIGMAS]
SENTINEL = 0x7FC0DEAD   # a NaN bit pattern no kernel produces


def _dev(a):
    return torch.from_numpy(np.array(a)).to(DEV)   # a copy: the shared references are read-only


def _bits(t):
    return t.contiguous().view(torch.int32)


def _same(a, b):
    return a.shape == b.shape and torch.equal(_bits(a), _bits(b))


def _sentinel(shape):
    return torch.full(shape, SENTINEL, dtype=torch.int32, device=DEV).view(torch.float32)


def _is_sentinel(t):
    return bool((_bits(t) == SENTINEL).all())


def _identity(backends, data, mask):
    """[n, H, W] x [n, 576, H, W] -> [n, 8H, 8W] through the ix = NULL path."""
    return backends.cvx_upsample(data[..., None].contiguous(), mask)[..., 0]


@pytest.mark.parametrize("case,sigma", TABLE)
def test_parity_with_fp64_at_every_pixel(backends, case, sigma):
    """Half and fp32 masks, ix NULL and ix a shuffled subset of a larger buffer: the bar is 32 u nb, no pixel excluded."""
    p = cr.problem(case, sigma)
    n, H, W = cr.CASES[case]
    data = _dev(p["data"])
    rng = np.random.default_rng(case)
    frames = rng.permutation(n + 3)[:n]                      # shuffled, distinct, not sorted
    ix = _dev(frames.astype(np.int64))
    disps = torch.zeros((n + 3, H, W), device=DEV)
    disps[ix] = data
    rest = torch.from_numpy(np.setdiff1d(np.arange(n + 3), frames)).to(DEV)
    for key in ("mask16", "mask32"):
        mask = _dev(p[key])
        got = _identity(backends, data, mask)
        e = cr.err_nb(got.cpu().numpy(), p["ref64"], p["nb"])
        print(f"{cr.CASES[case]} sigma {sigma} {key}: {e / cr.U:.2f} u nb")
        assert e <= cr.BAR, (cr.CASES[case], sigma, key, e / cr.U)
        out = _sentinel((n + 3, 8 * H, 8 * W))
        assert backends.upsample_disps(disps, ix, mask[None], out) is out
        assert _same(out[ix], got), "the indexed path computes other bits than the identity path"
        assert _is_sentinel(out[rest])


@pytest.mark.parametrize("case", range(len(cr.CASES)))
def test_one_hot_masks_bit_for_bit(backends, case):
    """Exactly the selected neighbour, +0.0 where it is padding; (1,1,1) and (2,1,9): all but the centre row is padding."""
    data, mask16, want = cr.onehot(case)
    for mask in (_dev(mask16), _dev(mask16.astype(np.float32))):
        got = _identity(backends, _dev(data), mask).cpu().numpy()
        assert cr.same_bits(got, want), (cr.CASES[case], mask.dtype)


@pytest.mark.parametrize("guard", [1024, 1027])   # 1027 floats: `out` is 4-byte aligned only (the scalar-store path)
def test_indexed_write_touches_only_its_frames(backends, guard):
    nbuf, H, W, s = 12, 5, 7, 4.0
    rng = np.random.default_rng(5)
    frames = [7, 2, 9, -1, 12, 4]
    n = len(frames)
    big_in = _sentinel((2 * guard + nbuf * H * W,))
    disps = big_in[guard:guard + nbuf * H * W].view(nbuf, H, W)
    disps.copy_(_dev(rng.uniform(0.001, 10.0, (nbuf, H, W)).astype(np.float32)))
    mask = _dev(rng.normal(0.0, s, (n, 576, H, W)).astype(np.float16))
    big_out = _sentinel((2 * guard + nbuf * 64 * H * W,))
    out = big_out[guard:guard + nbuf * 64 * H * W].view(nbuf, 8 * H, 8 * W)
    lib = backends._lib.load()
    rc = lib.droid_cvx_upsample(disps.data_ptr(), _dev(np.array(frames, np.int64)).data_ptr(), mask.data_ptr(),
                                out.data_ptr(), n, nbuf, nbuf, H, W, backends._lib.DROID_F16,
                                torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    assert rc == 0
    live = [(e, f) for e, f in enumerate(frames) if 0 <= f < nbuf]
    want = _identity(backends, disps[[f for _, f in live]], mask[[e for e, _ in live]])
    for k, (e, f) in enumerate(live):
        assert _same(out[f], want[k]), (e, f)
    rest = [f for f in range(nbuf) if f not in [f for _, f in live]]
    assert _is_sentinel(out[rest])
    assert _is_sentinel(big_out[:guard]) and _is_sentinel(big_out[-guard:])
    assert _is_sentinel(big_in[:guard]) and _is_sentinel(big_in[-guard:])


def test_frames_outside_the_smaller_buffer_are_skipped(backends):
    """nbuf_in != nbuf_out: the bound is the smaller of the two."""
    H, W = 3, 5
    rng = np.random.default_rng(6)
    disps = _dev(rng.uniform(0.001, 10.0, (4, H, W)).astype(np.float32))
    mask = _dev(rng.normal(0.0, 2.0, (3, 576, H, W)).astype(np.float32))
    out = _sentinel((6, 8 * H, 8 * W))
    backends.upsample_disps(disps, _dev(np.array([4, 1, 5], np.int64)), mask, out)     # 4, 5: not frames of disps
    assert _same(out[1], _identity(backends, disps[1:2], mask[1:2])[0])
    assert _is_sentinel(out[[0, 2, 3, 4, 5]])


def test_deterministic_and_independent_of_the_batch(backends):
    n, H, W = 6, 9, 8
    rng = np.random.default_rng(7)
    data = _dev(rng.uniform(0.001, 10.0, (n, H, W)).astype(np.float32))
    for dtype in (np.float16, np.float32):
        mask = _dev(rng.normal(0.0, 4.0, (n, 576, H, W)).astype(dtype))
        a = _identity(backends, data, mask)
        b = _identity(backends, data, mask)
        assert _same(a, b)
        order = [4, 0, 5, 2, 1, 3]                                  # every frame at another position of a batch of 6
        c = _identity(backends, data[order], mask[order])
        for pos, e in enumerate(order):
            assert _same(c[pos], a[e])
            assert _same(_identity(backends, data[e:e + 1], mask[e:e + 1])[0], a[e])   # alone, n = 1


@pytest.mark.parametrize("case,sigma", TABLE)
def test_distance_from_the_stock_chain(backends, case, sigma):
    """What a user sees when switching.  With half masks the stock chain is the less accurate side (it rounds its
    weights to half: 1.2 .. 1.5 x 2^-12 nb from fp64); the correctness bar is the parity test above."""
    p = cr.problem(case, sigma)
    data = _dev(p["data"])
    for key, bar in (("mask16", cr.STOCK_F16_DEV_BAR), ("mask32", cr.STOCK_F32_BAR)):
        mask = _dev(p[key])
        got = _identity(backends, data, mask).cpu().numpy()
        ref = cr.stock(data, mask).cpu().numpy().astype(np.float64)
        e = cr.err_nb(got, ref, p["nb"])
        print(f"{cr.CASES[case]} sigma {sigma} {key}: {e / cr.U:.1f} u nb = {e * 2 ** 12:.3f} x 2^-12 nb from the stock chain")
        assert e <= bar, (cr.CASES[case], sigma, key, e)


def test_caller_replay_on_a_side_stream(backends):
    """factor_graph.py:247-248: `self.video.upsample(torch.unique(self.ii), upmask)` with the body replaced."""
    nbuf, H, W = 16, 6, 8
    rng = np.random.default_rng(8)
    disps_np = rng.uniform(0.001, 10.0, (nbuf, H, W)).astype(np.float32)
    disps = _dev(disps_np)
    disps_up = _sentinel((nbuf, 8 * H, 8 * W))
    ii = _dev(np.array([3, 3, 5, 9, 9, 9, 12, 5, 3], np.int64))       # sources repeat
    ix = torch.unique(ii)
    n = int(ix.numel())
    mask_np = rng.normal(0.0, 4.0, (1, n, 576, H, W)).astype(np.float16)
    upmask = _dev(mask_np)
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        backends.upsample_disps(disps, ix, upmask, disps_up)
        total = disps_up[ix].double().sum()        # a following op on the same stream sees `out` complete
    side.synchronize()
    frames = ix.cpu().numpy()
    want = cr.ref(disps_np[frames], mask_np[0], np.float64)
    got = disps_up[ix].cpu().numpy()
    assert cr.err_nb(got, want, cr.nb(disps_np[frames])) <= cr.BAR
    assert np.isclose(float(total), got.astype(np.float64).sum(), rtol=1e-10, atol=0.0)
    rest = torch.from_numpy(np.setdiff1d(np.arange(nbuf), frames)).to(DEV)
    assert _is_sentinel(disps_up[rest])
    assert np.array_equal(disps.cpu().numpy(), disps_np)             # the disparity buffer is only read
