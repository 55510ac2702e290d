"""CPU checks of the reference side of the fused lookup + encoder (tests/corr_encode_ref.py): the restated sum against
torch's own convolution in float64, the packed layout against itself, its padding, and the package's packer against the
restated layout."""
import numpy as np
import torch

import corr_encode_ref as cr


def _params(seed):
    """nn.Conv2d(196, 128, 1)'s default init: uniform in +-1/sqrt(fan_in) for weight and bias."""
    g = torch.Generator().manual_seed(seed)
    k = 1.0 / np.sqrt(cr.KTOT)
    w = (torch.rand((cr.N, cr.KTOT), generator=g) * 2 - 1) * k
    b = (torch.rand((cr.N,), generator=g) * 2 - 1) * k
    return w.numpy(), b.numpy()


def test_restatement_equals_conv2d_relu_in_float64():
    w, b = _params(1)
    rng = np.random.default_rng(2)
    a = (rng.standard_normal((3, cr.KTOT, 5, 7)) * 4).astype(np.float16)
    a[0, :, 0, 0] = 0
    s, S = cr.sums(a, w, b)
    w16 = torch.from_numpy(cr.half(w)).double()[:, :, None, None]
    b16 = torch.from_numpy(cr.half(b)).double()
    x = torch.from_numpy(a).double()
    want = torch.relu(torch.nn.functional.conv2d(x, w16, b16)).numpy()
    assert s.shape == want.shape == (3, cr.N, 5, 7)
    assert np.abs(cr.relu(s) - want).max() <= 1e-12
    wantS = torch.nn.functional.conv2d(x.abs(), w16.abs(), b16.abs()).numpy()
    assert np.abs(S - wantS).max() <= 1e-12
    assert np.array_equal(cr.relu(s)[0, :, 0, 0], np.maximum(cr.half(b).astype(np.float64), 0))   # a = 0: relu(b16)
    assert (cr.bound(s, S) >= 2.0 ** -25).all() and (S >= np.abs(s) - 1e-12).all()


def test_pack_round_trip_is_bit_exact_and_the_padding_is_zero():
    w, b = _params(3)
    w[5, 7] = 1e9          # overflows to inf in half: the cast is the contract, not a clamp
    w[6, 8] = 1e-9         # underflows to zero
    p = cr.pack(w, b)
    assert p.dtype == np.float16 and p.shape == (cr.PACKED_HALVES,) and p.nbytes == 4 * 64 * 128 * 2 + 256
    w16, b16 = cr.unpack(p)
    assert np.array_equal(w16.view(np.uint16), cr.half(w).view(np.uint16))
    assert np.array_equal(b16.view(np.uint16), cr.half(b).view(np.uint16))
    assert np.isinf(w16[5, 7]) and w16[6, 8] == 0
    pad = cr.padding_mask()
    assert pad.sum() == cr.LEVELS * (cr.KP - cr.K) * cr.N
    ones = cr.pack(np.ones((cr.N, cr.KTOT), np.float32), np.ones(cr.N, np.float32))
    assert not ones.view(np.uint16)[pad].any()            # zero bits, +0
    assert (ones[~pad] == 1).all()                        # and every other entry is a parameter


def test_every_lane_finds_its_fragment_in_one_16_byte_run():
    """Element (l, s, nt, lane, 0..7) is 8 consecutive K of one output channel: the B fragment of the 16x16x32 MFMA."""
    w = np.arange(cr.N * cr.KTOT, dtype=np.float32).reshape(cr.N, cr.KTOT) % 2048     # exact in half
    body = cr.pack(w, np.zeros(cr.N, np.float32))[:-cr.N].reshape(cr.LEVELS, 2, 8, 64, 8)
    for l, s, nt, lane in ((0, 0, 0, 0), (1, 0, 3, 17), (2, 1, 7, 63), (3, 1, 2, 31), (3, 0, 5, 48)):
        n, k0 = 16 * nt + (lane & 15), 32 * s + 8 * (lane >> 4)
        want = [w[n, cr.K * l + k0 + j] if k0 + j < cr.K else 0.0 for j in range(8)]
        assert body[l, s, nt, lane].tolist() == want


def test_the_packages_packer_is_the_restated_layout():
    from droid_backends import corr_encode as ce
    assert (ce.LEVELS, ce.K, ce.KP, ce.N) == (cr.LEVELS, cr.K, cr.KP, cr.N) and ce.packed_halves() == cr.PACKED_HALVES
    w, b = _params(4)
    table = torch.cat([torch.from_numpy(w).to(torch.float16).reshape(-1), torch.zeros(1, dtype=torch.float16)])
    got = torch.cat([table[ce.pack_index()], torch.from_numpy(b).to(torch.float16)]).numpy()
    assert np.array_equal(got.view(np.uint16), cr.pack(w, b).view(np.uint16))
