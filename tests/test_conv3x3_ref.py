"""CPU checks of the numpy restatement of droid_conv3x3's contract (tests/conv3x3_ref.py) that the GPU tests are held
against, of the packed layout, and of the package's packer against the restated one."""
import numpy as np
import pytest
import torch

import conv3x3_ref as ref


@pytest.mark.parametrize("case", ref.cases(), ids=ref.case_id)
def test_the_restatement_is_conv2d_in_float64(case):
    c_in, c_out, k, h, w, B = case
    x, wt, b = ref.operands(3, c_in, k * c_out, h, w, B)
    s, mag = ref.exact(x, wt, b)
    t = lambda a: torch.from_numpy(a.astype(np.float64))
    want = torch.nn.functional.conv2d(t(x), t(wt), t(b), padding=1).numpy()
    scale = np.maximum(mag, 1.0)
    assert np.all(np.abs(s - want) <= 1e-12 * scale)              # two fp64 summation orders
    assert np.all(mag >= np.abs(s - b.astype(np.float64)[None, :, None, None]) - 1e-12 * scale)
    got = ref.conv(x, wt, b, relu=True)
    relu = torch.relu(torch.from_numpy(want)).numpy().astype(np.float16)
    differ = got != relu
    # the two may round a value within 1e-12 of a tie differently; nothing else may differ
    assert differ.sum() <= 2 and np.all(np.abs(got[differ].astype(np.float64) - relu[differ]) <= 2.0 ** -10 * scale[differ])
    assert got.dtype == np.float16 and not np.any(np.signbit(got))   # +0, never -0, below zero


def test_the_window_is_zero_padded_and_ordered_c_ky_kx():
    x = np.arange(1, 2 * 3 * 4 * 5 + 1, dtype=np.float64).reshape(2, 3, 4, 5)
    a = ref.window(x)
    assert a.shape == (2, 4, 5, 27)
    for b in range(2):
        for v in range(4):
            for u in range(5):
                for c in range(3):
                    for ky in range(3):
                        for kx in range(3):
                            r, q = v + ky - 1, u + kx - 1
                            want = x[b, c, r, q] if 0 <= r < 4 and 0 <= q < 5 else 0.0
                            assert a[b, v, u, 9 * c + 3 * ky + kx] == want
    # a row's end sees zeros, not the next row's start or the next image
    assert a[0, 1, 4, 9 * 0 + 3 * 1 + 2] == 0 and a[0, 3, 2, 9 * 1 + 3 * 2 + 1] == 0


def test_relu_keeps_nan_and_gives_plus_zero():
    y = np.array([1.5, -2.0, -0.0, 0.0, np.nan, np.inf, -np.inf], dtype=np.float16)
    r = ref.act(y, True)
    assert r[0] == 1.5 and np.isnan(r[4]) and r[5] == np.inf
    assert np.all(r[[1, 2, 3, 6]].view(np.uint16) == 0)
    assert np.array_equal(ref.act(y, False).view(np.uint16), y.view(np.uint16))


@pytest.mark.parametrize("c_in,c_out", ref.PACK_SIZES)
def test_pack_is_a_bijection_without_padding(c_in, c_out):
    # every weight gets a distinct bit pattern, so a bijection onto the weight shows as a permutation of the values
    n = 9 * c_in * c_out
    w = (np.arange(n, dtype=np.int64) * 7919 % 30011 + 1024).astype(np.uint16)          # normal halves, not distinct yet
    w = w.reshape(c_out, c_in, 3, 3)
    idx = np.arange(n, dtype=np.int64).reshape(c_out, c_in, 3, 3)
    b = (np.arange(c_out) + 15000).astype(np.uint16).view(np.float16)
    packed = ref.pack(w.view(np.float16), b)
    assert packed.size == ref.packed_halves(c_in, c_out) and (packed.size * 2) % 16 == 0 and (n * 2) % 16 == 0
    w2, b2 = ref.unpack(packed, c_in, c_out)
    assert np.array_equal(w2.view(np.uint16), w) and np.array_equal(b2.view(np.uint16), b.view(np.uint16))
    # positions: pack the index planes (as two uint16 planes) and see every index exactly once, where the header says
    lo = ref.pack((idx & 0xffff).astype(np.uint16).view(np.float16), b)[:n].view(np.uint16).astype(np.int64)
    hi = ref.pack((idx >> 16).astype(np.uint16).view(np.float16), b)[:n].view(np.uint16).astype(np.int64)
    where = (hi << 16) | lo
    assert np.array_equal(np.sort(where), np.arange(n))                                   # a bijection: no padding
    el = where.reshape(c_in // 32, 9, c_out // 16, 64, 8)
    for s, t, nt, lane, j in [(0, 0, 0, 0, 0), (0, 5, 1, 17, 3), (c_in // 32 - 1, 8, c_out // 16 - 1, 63, 7), (0, 2, 3, 40, 6)]:
        assert el[s, t, nt, lane, j] == idx[16 * nt + (lane & 15), 32 * s + 8 * (lane >> 4) + j, t // 3, t % 3]


@pytest.mark.parametrize("c_in,c_out", ref.PACK_SIZES)
def test_the_packages_packer_gives_the_restated_layout(c_in, c_out):
    from droid_backends import conv3x3 as mod            # the one test that looks at the package
    rng = np.random.default_rng(c_in + c_out)
    w = rng.normal(0, 1, (c_out, c_in, 3, 3)).astype(np.float32)
    b = rng.normal(0, 1, (c_out,)).astype(np.float32)
    got = mod.pack(torch.from_numpy(w), torch.from_numpy(b)).numpy()
    want = ref.pack(w.astype(np.float16), b.astype(np.float16))                        # rounded once, nearest-even
    assert got.dtype == np.float16 and np.array_equal(got.view(np.uint16), want.view(np.uint16))
    half = mod.pack(torch.from_numpy(w).half(), torch.from_numpy(b).half()).numpy()  # half parameters: the same bits
    assert np.array_equal(half.view(np.uint16), want.view(np.uint16))
    assert mod.supported(c_in, c_out) and not mod.supported(c_in + 16, c_out) and not mod.supported(c_in, c_out + 32)


@pytest.mark.parametrize("chan", ref.CHANNELS + [ref.GRU_CHANNELS], ids=lambda c: "%dto%dx%d" % (c[0], c[2], c[1]))
def test_the_bound_tests_seed_puts_outputs_on_both_sides_of_zero(chan):
    c_in, c_out, k = chan
    x, wt, b = ref.operands(ref.BOUND_SEED, c_in, k * c_out, 11, 13, 3)
    s, _ = ref.exact(x, wt, b)
    assert (s > 0).mean() >= 0.25 and (s < 0).mean() >= 0.25
