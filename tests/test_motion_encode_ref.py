"""CPU checks of the reference side of the fused motion encoder (tests/motion_encode_ref.py): the restated sum against
torch's own 7 x 7 convolution in float64 on the shapes of the GPU suite, the packed layout against itself, the packer as
a bijection onto [128,4,7,7], the package's packer against the restated layout, and the seed of the product test: both
sides of the ReLU are exercised on every shape."""
import numpy as np
import pytest
import torch

import motion_encode_ref as mr

PRODUCT_SEED = 9      # tests/test_gpu_motion_encode.py uses the same parameters


@pytest.mark.parametrize("H,W,E", mr.SHAPES)
def test_restatement_equals_conv2d_relu_in_float64(H, W, E):
    w, b = mr.params(1)
    m = mr.oracle_motion(H, W, E)[0].astype(np.float32)
    assert np.isfinite(m).all() and np.abs(m).max() <= 64
    # all four planes carry values (a stereo edge alone moves nothing along y: plane 1 of the one-edge case is zero)
    assert all((m[:, c] != 0).any() for c in range(4) if E > 1 or c != 1)
    s, S = mr.sums(m, w, b)
    a = torch.from_numpy(mr.half(m)).double()
    w16 = torch.from_numpy(mr.half(w)).double()
    b16 = torch.from_numpy(mr.half(b)).double()
    want = torch.relu(torch.nn.functional.conv2d(a, w16, b16, padding=3)).numpy()
    assert s.shape == want.shape == (E, mr.N, H, W)
    assert np.abs(mr.relu(s) - want).max() <= 1e-12
    wantS = torch.nn.functional.conv2d(a.abs(), w16.abs(), b16.abs(), padding=3).numpy()
    assert np.abs(S - wantS).max() <= 1e-12
    assert (mr.bound(s, S) >= 2.0 ** -25).all() and (S >= np.abs(s) - 1e-12).all()
    for e in mr.scene(H, W, E)["bad"]:      # m = 0: relu(b16) everywhere
        assert np.array_equal(mr.relu(s)[e], np.broadcast_to(np.maximum(mr.half(b).astype(np.float64), 0)[:, None, None],
                                                             (mr.N, H, W)))


def test_the_window_is_zero_padded_and_ordered_c_ky_kx():
    m = np.arange(1, 1 + 4 * 3 * 5, dtype=np.float32).reshape(1, 4, 3, 5)     # exact in half
    win = mr.windows(m)
    assert win.shape == (1, mr.KTOT, 3, 5)
    for c, ky, kx, v, u in ((0, 3, 3, 1, 2), (2, 0, 0, 0, 0), (3, 6, 6, 2, 4), (1, 2, 5, 1, 0), (3, 4, 1, 2, 3)):
        y, x = v + ky - 3, u + kx - 3
        want = m[0, c, y, x] if 0 <= y < 3 and 0 <= x < 5 else 0.0
        assert win[0, 49 * c + 7 * ky + kx, v, u] == want
    assert win[0, :, 0, 0].reshape(4, 7, 7)[:, :3, :].any() == False and win[0, 24, 1, 2] == m[0, 0, 1, 2]   # noqa: E712
    # the half cast of m is part of the operand: 2049 is not a half
    assert mr.windows(np.full((1, 4, 1, 1), 2049.0, np.float32))[0, 24, 0, 0] == 2048.0


@pytest.mark.parametrize("H,W,E", mr.SHAPES)
def test_the_seed_of_the_product_test_exercises_both_sides_of_the_relu(H, W, E):
    w, b = mr.params(PRODUCT_SEED)
    s, _ = mr.sums(mr.oracle_motion(H, W, E)[0].astype(np.float32), w, b)
    assert (s > 0).mean() > 0.2 and (s < 0).mean() > 0.2, ((s > 0).mean(), (s < 0).mean())


def test_pack_round_trip_is_bit_exact_and_the_padding_is_zero():
    w, b = mr.params(3)
    w[5, 1, 2, 3] = 1e9          # overflows to inf in half: the cast is the contract, not a clamp
    w[6, 3, 6, 6] = 1e-9         # underflows to zero
    p = mr.pack(w, b)
    assert p.dtype == np.float16 and p.shape == (mr.PACKED_HALVES,) and p.nbytes == 4 * 64 * 128 * 2 + 256
    w16, b16 = mr.unpack(p)
    assert np.array_equal(w16.view(np.uint16), mr.half(w).view(np.uint16))
    assert np.array_equal(b16.view(np.uint16), mr.half(b).view(np.uint16))
    assert np.isinf(w16[5, 1, 2, 3]) and w16[6, 3, 6, 6] == 0
    pad = mr.padding_mask()
    assert pad.sum() == mr.CHANNELS * (mr.KP - mr.K) * mr.N
    ones = mr.pack(np.ones((mr.N, 4, 7, 7), np.float32), np.ones(mr.N, np.float32))
    assert not ones.view(np.uint16)[pad].any()            # zero bits, +0
    assert (ones[~pad] == 1).all()                        # and every other entry is a parameter


def test_the_packer_is_a_bijection_onto_the_weight():
    """Every non-padding position of the packed weights names one element of [128,4,7,7], and every element is named
    once: seen through the package's index table and through the restated layout."""
    from droid_backends import corr_encode as ce
    idx = ce.pack_index().numpy()
    body_pad = mr.padding_mask()[:-mr.N]
    assert idx.shape == body_pad.shape
    assert (idx[body_pad] == mr.N * mr.KTOT).all()                       # the padding reads the table's zero entry
    assert np.array_equal(np.sort(idx[~body_pad]), np.arange(mr.N * mr.KTOT))
    # the restated layout puts element (n, c, ky, kx) where the index table says flat index n * 196 + 49 c + 7 ky + kx is
    for n, c, ky, kx in ((0, 0, 0, 0), (127, 3, 6, 6), (17, 2, 4, 5), (64, 1, 0, 6), (99, 3, 3, 3)):
        w = np.zeros((mr.N, 4, 7, 7), np.float32)
        w[n, c, ky, kx] = 1.0
        at = np.flatnonzero(mr.pack(w, np.zeros(mr.N, np.float32)))
        assert at.tolist() == np.flatnonzero(idx == n * mr.KTOT + 49 * c + 7 * ky + kx).tolist() and len(at) == 1


def test_the_packages_packer_is_the_restated_layout():
    from droid_backends import corr_encode as ce, motion_encode as me
    assert (me.CHANNELS, me.KSIZE, me.K, me.N) == (mr.CHANNELS, mr.KS, mr.K, mr.N) and ce.packed_halves() == mr.PACKED_HALVES
    w, b = mr.params(4)
    table = torch.cat([torch.from_numpy(w).to(torch.float16).reshape(-1), torch.zeros(1, dtype=torch.float16)])
    got = torch.cat([table[ce.pack_index()], torch.from_numpy(b).to(torch.float16)]).numpy()
    assert np.array_equal(got.view(np.uint16), mr.pack(w, b).view(np.uint16))
