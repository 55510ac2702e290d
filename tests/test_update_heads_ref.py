"""CPU checks of tests/update_heads_ref.py, the numpy restatement of droid_update_heads (include/droid_heads_hip.h):
the sums against torch's float64 convolution, the packed layout against itself and against the package's packer, the
bound against what a device may compute (fp32 accumulation in random orders) and against two wrong restatements."""
import numpy as np
import pytest
import torch

import update_heads_ref as uh

KINDS = (uh.IDENTITY, uh.SIGMOID, uh.SOFTPLUS_CENTI)


@pytest.mark.parametrize("H,W,B", uh.SHAPES)
def test_sums_are_the_convolution(H, W, B):
    x = uh.hidden(B, H, W, 1)
    for kind in KINDS:
        w, b = uh.params(kind, 1)
        t, S = uh.sums(x, w, b)
        w64 = torch.from_numpy(uh.half(w).astype(np.float64))
        b64 = torch.from_numpy(uh.half(b).astype(np.float64))
        x64 = torch.from_numpy(x.astype(np.float64))
        want = torch.nn.functional.conv2d(x64, w64, b64, padding=1).permute(0, 2, 3, 1).numpy()
        assert t.shape == want.shape == (B, H, W, uh.N_OUT[kind])
        assert np.abs(t - want).max() <= 1e-12
        wantS = torch.nn.functional.conv2d(x64.abs(), w64.abs(), b64.abs(), padding=1).permute(0, 2, 3, 1).numpy()
        assert np.abs(S - wantS).max() <= 1e-12 and (S >= np.abs(t) - 1e-12).all()


def test_activations():
    t = np.array([-1000.0, -30.0, -1.0, 0.0, 1.0, 19.98, 20.0, 20.02, 1000.0])
    assert np.array_equal(uh.act(uh.IDENTITY, t), t)
    want = torch.sigmoid(torch.from_numpy(t)).numpy()
    assert np.allclose(uh.act(uh.SIGMOID, t), want, rtol=1e-14, atol=0) and uh.act(uh.SIGMOID, -1000.0) == 0.0
    want = .01 * torch.nn.functional.softplus(torch.from_numpy(t)).numpy()
    assert np.allclose(uh.act(uh.SOFTPLUS_CENTI, t), want, rtol=1e-14, atol=0)
    assert np.isfinite(uh.act(uh.SIGMOID, t)).all() and np.isfinite(uh.act(uh.SOFTPLUS_CENTI, t)).all()


@pytest.mark.parametrize("kind", KINDS)
def test_pack_round_trip_and_zero_padding(kind):
    w, b = uh.params(kind, 2)
    n = uh.N_OUT[kind]
    packed = uh.pack(w, b)
    assert packed.dtype == np.float32 and packed.size == uh.packed_floats(n) and packed.size * 4 % 16 == 0
    assert packed.size * 4 == {1: 4624, 2: 9232}[n]
    mask = uh.padding_mask(n)
    assert mask.sum() == {1: 3, 2: 2}[n] and (packed[mask].view(np.uint32) == 0).all()
    w16, b16 = uh.unpack(packed, n)
    assert np.array_equal(w16.view(np.uint16), uh.half(w).view(np.uint16))
    assert np.array_equal(b16.view(np.uint16), uh.half(b).view(np.uint16))
    # every entry is a half widened to fp32, and an entry of its own: distinct weights land in distinct places
    assert np.array_equal(packed, packed.astype(np.float16).astype(np.float32))
    marks = np.arange(n * uh.KTOT, dtype=np.float32).reshape(n, uh.C, 3, 3) % 2048     # exact in half
    back, _ = uh.unpack(uh.pack(marks, np.zeros(n, np.float32)), n)
    assert np.array_equal(back.astype(np.float32), marks)


@pytest.mark.parametrize("kind", KINDS)
def test_the_packages_packer_is_the_restated_layout(backends, kind):
    from droid_backends import update_heads as mod
    n = uh.N_OUT[kind]
    assert backends._lib.load().droid_head_packed_bytes(n) == 4 * uh.packed_floats(n)
    for dtype in (torch.float32, torch.float16):
        w, b = uh.params(kind, 3)
        got = mod.pack(torch.from_numpy(w).to(dtype), torch.from_numpy(b).to(dtype)).numpy()
        assert got.dtype == np.float32
        assert np.array_equal(got.view(np.uint32), uh.pack(w, b).view(np.uint32))


@pytest.mark.parametrize("H,W,B", uh.SHAPES)
def test_fp32_accumulation_in_any_order_meets_the_bound(H, W, B):
    x = uh.hidden(B, H, W, 1)
    for kind in KINDS:
        w, b = uh.params(kind, 1)
        t, S = uh.sums(x, w, b)
        want, bd = uh.act(kind, t), uh.bound(kind, t, S)
        for got in uh.shuffled_fp32(x, w, b, kind, seeds=(11, 12, 13)):
            ratio = np.abs(got - want) / bd
            assert ratio.max() < 1.0, (kind, float(ratio.max()))     # every element, nothing excluded


@pytest.mark.parametrize("H,W,B", [s for s in uh.SHAPES if s[0] >= 3 and s[1] >= 3])
def test_wrong_restatements_miss_the_bound(H, W, B):
    x = uh.hidden(B, H, W, 1)
    for kind in KINDS:
        w, b = uh.params(kind, 1)
        t, S = uh.sums(x, w, b)
        want, bd = uh.act(kind, t), uh.bound(kind, t, S)
        for wrong in (dict(transpose_taps=True), dict(mode="edge")):
            tw, _ = uh.sums(x, w, b, **wrong)
            got = uh.half(uh.act(kind, tw)).astype(np.float64)
            assert (np.abs(got - want) / bd).max() > 1.0, (kind, wrong)


def test_inputs_are_shared_and_what_they_claim():
    x = uh.hidden(5, 48, 64, 1)
    assert x is uh.hidden(5, 48, 64, 1) and not x.flags.writeable and x.dtype == np.float16
    zeros = float((x == 0).mean())
    assert 0.45 < zeros < 0.55 and (x >= 0).all()
    for kind in KINDS:
        w, b = uh.params(kind, 1)
        assert w.shape == (uh.N_OUT[kind], 128, 3, 3) and np.abs(w).max() <= 1 / np.sqrt(1152)
