"""Pins tests/corr_volume_ref.py against stock PyTorch on the CPU, i.e. against the reference's own call sequence
(`/ 4`, matmul, view, avg_pool2d; droid_slam/modules/corr.py:24-38, 63-71): `pool` equals F.avg_pool2d bit for bit,
and torch's level 0 meets the level-0 criterion of the GPU test against `level0_exact`.  Passes without the operator;
it is what makes the GPU assertions mean something."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import corr_volume_ref as ref

CASES = [(np.float16, torch.float16), (np.float32, torch.float32)]


@pytest.mark.parametrize("npdt,tdt", CASES)
@pytest.mark.parametrize("h,w", [(16, 24), (15, 20)])
def test_pool_is_avg_pool2d_bit_for_bit(npdt, tdt, h, w):
    rng = np.random.default_rng(h * w)
    x = (rng.normal(0, 1, (6, h, w)) * np.exp2(rng.integers(-16, 3, (6, 1, 1)))).astype(npdt)
    lvl = x
    t = torch.from_numpy(x)[:, None]
    for _ in range(3):
        lvl = ref.pool(lvl, npdt)
        t = F.avg_pool2d(t, 2, stride=2)
        assert lvl.shape == tuple(t[:, 0].shape)
        assert np.array_equal(lvl.view(np.uint8), t[:, 0].numpy().view(np.uint8))


@pytest.mark.parametrize("npdt,tdt", CASES)
@pytest.mark.parametrize("h,w", [(16, 24), (15, 20)])
def test_torch_level0_meets_the_level0_criterion(npdt, tdt, h, w):
    rng = np.random.default_rng(7)
    C, nbuf = 128, 3
    fmaps = rng.normal(0, 1, (nbuf, 1, C, h, w)).astype(npdt)
    ii, jj = [0, 2], [1, 0]
    a, b = ref.operands(fmaps, ii, jj, npdt)
    f = torch.from_numpy(fmaps)
    f1 = f[ii, 0].reshape(2, C, h * w) / 4.0
    f2 = f[jj, 0].reshape(2, C, h * w) / 4.0
    assert np.array_equal(f1.numpy(), a) and np.array_equal(f2.numpy(), b)
    vol = torch.matmul(f1.transpose(1, 2), f2).numpy()
    lo, hi, mid = ref.level0_interval(a, b, npdt)
    assert vol.dtype == npdt
    assert np.all(lo <= vol) and np.all(vol <= hi)
    print(f"share of entries != T(x): {np.mean(vol != mid):.2e}")


def test_operands_keep_half_subnormals_and_out_of_range_edges_are_zero():
    rng = np.random.default_rng(3)
    fmaps = (rng.normal(0, 1, (2, 2, 32, 8, 8)) * 2.0 ** -13).astype(np.float16)
    a, b = ref.operands(fmaps, [0, 1, 5], [0, 0, 1], np.float16)
    t = torch.from_numpy(fmaps)
    assert np.array_equal(a[0], (t[0, 0] / 4.0).numpy().reshape(32, 64))
    assert np.array_equal(b[0], (t[0, 1] / 4.0).numpy().reshape(32, 64))   # stereo edge: camera 1
    assert np.array_equal(b[1], (t[0, 0] / 4.0).numpy().reshape(32, 64))
    assert np.any((a[0] != 0) & (np.abs(a[0]) < 2.0 ** -14))               # subnormal operands are present
    assert not a[2].any() and not b[2].any()
