"""The wave-level sum of the BA linearisation (ba_kernels.hip::wave_reduce32) through its test hook
droid_test_wave_reduce32: bit for bit the halving butterfly it documents -- partners lane ^ 32, ^ 16, ^ 8, ^ 4, ^ 2, ^ 1,
the half of the lanes with the bit clear keeps the even value of each pair -- and the lane -> value map reduce32_index.
The sums of the reduced camera system depend on that addition tree staying what it is."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

LANES = np.arange(64)


def reduce32_index(lane):
    return ((lane >> 5) & 1) | (((lane >> 4) & 1) << 1) | (((lane >> 3) & 1) << 2) | (((lane >> 2) & 1) << 3) | (((lane >> 1) & 1) << 4)


def tree(x):
    """numpy float32 restatement: x [64 lanes][32 values] -> what every lane returns."""
    v = np.asarray(x, np.float32).copy()
    for bit in (32, 16, 8, 4, 2):
        hi = (LANES & bit) != 0
        nxt = np.empty((64, v.shape[1] // 2), np.float32)
        for i in range(nxt.shape[1]):
            keep = np.where(hi, v[:, 2 * i + 1], v[:, 2 * i])
            send = np.where(hi, v[:, 2 * i], v[:, 2 * i + 1])
            nxt[:, i] = keep + send[LANES ^ bit]
        v = nxt
    return v[:, 0] + v[LANES ^ 1, 0]


def device(backends, x):
    import torch
    lib = backends._lib.load()
    din = torch.from_numpy(np.ascontiguousarray(x, np.float32)).cuda()
    out = torch.full((64,), float("nan"), dtype=torch.float32, device="cuda")
    backends._lib.check(lib.droid_test_wave_reduce32(din.data_ptr(), out.data_ptr(), torch.cuda.current_stream().cuda_stream),
                        "test_wave_reduce32")
    torch.cuda.synchronize()
    return out.cpu().numpy()


def test_tagged_integers_reach_the_right_lane(backends):
    """x[l][k] = 8192 (k + 1) + l^2 + 1: every partial sum is an integer below 2^24, so nothing rounds, and a total
    names its value (multiples of 2^19) and counts every lane once (sum of l^2 + 1 = 85408 < 2^17)."""
    x = (8192.0 * (np.arange(32)[None, :] + 1) + (LANES[:, None] ** 2 + 1)).astype(np.float32)
    got = device(backends, x)
    want = (2.0 ** 19) * (reduce32_index(LANES) + 1) + 85408.0
    print("tagged totals, lanes 0..7:", got[:8], "expected", want[:8])
    assert np.array_equal(got, want.astype(np.float32))
    assert np.array_equal(got.view(np.uint32), tree(x).view(np.uint32))


@pytest.mark.parametrize("seed", [0, 1, 2])
def test_order_dependent_sums_bit_for_bit(backends, seed):
    """Normal draws scaled by 2^[-20, 20): the rounded sum depends on the pairing, so any other tree shows."""
    rng = np.random.default_rng(seed)
    x = (rng.normal(size=(64, 32)) * 2.0 ** rng.integers(-20, 20, size=(64, 32))).astype(np.float32)
    want = tree(x)
    # the inputs do tell trees apart: a plain left-to-right sum over the lanes differs somewhere
    serial = np.zeros(32, np.float32)
    for l in range(64):
        serial = serial + x[l]
    assert not np.array_equal(serial[reduce32_index(LANES)].view(np.uint32), want.view(np.uint32))
    got = device(backends, x)
    bad = np.flatnonzero(got.view(np.uint32) != want.view(np.uint32))
    print(f"seed {seed}: {bad.size} of 64 lanes differ from the restated tree")
    assert bad.size == 0, (bad, got[bad], want[bad])
