"""droid_motion_encode on the device (include/droid_motion_encode_hip.h): reproject + motion features fused with
flow_encoder[0:2].

1. The operand, bit for bit: selection weights make the sum one exact term, so y[:, n] must be the bits of
   relu(+-half(m)[c, shifted by (ky - 3, kx - 3), zero-filled]) with m from motion_features (which the rest of the suite
   pins to the oracle) -- through the geometry loader and through enc.conv(m).
2. coords1 and mask are reproject's bits; the edge outside the buffer gives zeros and y = relu(b16).
3. The product: random parameters at nn.Conv2d's init scale, every element within tests/motion_encode_ref.bound of
   relu(s), s in float64 from the device's own m.
4. Both loaders agree.   5. Determinism and history.   6. The stock chain's distance (printed).
"""
import functools

import numpy as np
import pytest
import torch

import motion_encode_ref as mr
from test_gpu_pyramid_slots import _coords as _mix_coords, _poison_free_memory, _random_pyramid
from test_motion_encode_ref import PRODUCT_SEED

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
GEOMETRY = ("poses", "disps", "intrinsics", "ii", "jj", "target")
# weight[n, first + n] = +-1: k = 0 .. 127 and 68 .. 195, each with both sign patterns -- all 196 (c, ky, kx), every one
# with both signs (behind the ReLU one sign shows only the positive values of m at a tap, the other only the negative)
SELECTIONS = ((0, 0), (0, 1), (68, 0), (68, 1))


def _bits(x):
    return x.contiguous().view(torch.int16)


def _relu(x):
    """max(., 0) of the contract: +0 for everything that is not above zero."""
    return torch.where(x > 0, x, torch.zeros_like(x))


@functools.lru_cache(maxsize=None)
def _inputs(H, W, E):
    sc = mr.scene(H, W, E)
    return tuple(torch.from_numpy(np.array(sc[k])).to(DEV) for k in GEOMETRY)     # scene's arrays are read-only


@functools.lru_cache(maxsize=None)
def _unfused(H, W, E):
    """(m [E,4,H,W], coords1 [1,E,H,W,2], mask [1,E,H,W,1]) of the unfused operator on the case's inputs."""
    import droid_backends as db
    m, coords1, mask = db.motion_features(*_inputs(H, W, E))
    torch.cuda.synchronize()
    return m[0].contiguous(), coords1, mask


def _params(seed):
    w, b = mr.params(seed)
    return torch.from_numpy(w).to(DEV), torch.from_numpy(b).to(DEV)


def _selection(first, flip):
    w = torch.zeros((mr.N, mr.KTOT))
    n = torch.arange(mr.N)
    sign = torch.where((n + flip) % 2 == 0, 1.0, -1.0)
    w[n, first + n] = sign
    return w.reshape(mr.N, mr.CHANNELS, mr.KS, mr.KS).to(DEV), sign.to(DEV)


def _windows(m):
    """[E,196,H,W] half: channel 49 c + 7 ky + kx is half(m)[:, c] shifted by (ky - 3, kx - 3), zero-filled."""
    E, _, H, W = m.shape
    return torch.nn.functional.unfold(m.half().float(), mr.KS, padding=3).reshape(E, mr.KTOT, H, W).half()


# ------------------------------------------------------------------------------------------- 1. the operand, bit for bit
@pytest.mark.parametrize("loader", ["geometry", "conv"])
@pytest.mark.parametrize("H,W,E", mr.SHAPES)
def test_selection_weights_return_the_operand_bits(backends, H, W, E, loader):
    m = _unfused(H, W, E)[0]
    win = _windows(m)
    zero_bias = torch.zeros(mr.N, device=DEV)
    nonzero = False
    for first, flip in SELECTIONS:
        wsel, sign = _selection(first, flip)
        enc = backends.FlowEncoder(wsel, zero_bias)
        _poison_free_memory((E, mr.N, H, W), torch.float16)
        got = enc(*_inputs(H, W, E))[0] if loader == "geometry" else enc.conv(m)
        torch.cuda.synchronize()
        want = _relu(win[:, first:first + mr.N] * sign.half()[None, :, None, None])
        assert bool(torch.isfinite(want).all())
        nonzero = nonzero or bool((want != 0).any())
        assert got.shape == (E, mr.N, H, W) and got.dtype == torch.float16
        bad = _bits(got) != _bits(want)
        assert not bool(bad.any()), (first, int(bad.sum()), torch.nonzero(bad)[:4].tolist())
    assert nonzero      # over the four sets (at 1 x 1 one set alone can be all zero: four taps, a sign each)


# ------------------------------------------------------------------------------------------- 2. the geometry's outputs
@pytest.mark.parametrize("H,W,E", mr.SHAPES)
def test_coords_and_mask_are_reprojects_bits(backends, H, W, E):
    inp = _inputs(H, W, E)
    c_ref, v_ref = backends.reproject(*inp[:5])
    m_ref, c_mf, v_mf = _unfused(H, W, E)
    w, b = _params(5)
    enc = backends.FlowEncoder(w, b)
    _poison_free_memory((E, mr.N, H, W), torch.float16)
    _poison_free_memory((1, E, H, W, 2), torch.float32)
    y, coords1, mask = enc(*inp)
    torch.cuda.synchronize()
    assert coords1.shape == (1, E, H, W, 2) and mask.shape == (1, E, H, W, 1) and y.shape == (E, mr.N, H, W)
    assert coords1.dtype == mask.dtype == torch.float32 and y.dtype == torch.float16
    for ref_c, ref_v in ((c_ref, v_ref), (c_mf, v_mf)):
        assert torch.equal(coords1.view(torch.int32), ref_c.view(torch.int32))
        assert torch.equal(mask.view(torch.int32), ref_v.view(torch.int32))
    bad = mr.scene(H, W, E)["bad"]
    assert len(bad) == (1 if E >= 3 else 0)
    for e in bad:
        assert not bool(coords1[0, e].view(torch.int32).any()) and not bool(mask[0, e].view(torch.int32).any())
        assert not bool(m_ref[e].view(torch.int32).any())
        want = _relu(b.half())[:, None, None].expand(mr.N, H, W)
        assert torch.equal(_bits(y[e]), _bits(want)) and bool((want > 0).any())
    # the batched state, one set of intrinsics and a target without the batch dimension are the same call
    one_k = inp[2][0].contiguous()
    y1, c1, v1 = enc(inp[0][None], inp[1][None], one_k, inp[3], inp[4], inp[5])
    c2, v2, m2 = backends.reproject(inp[0], inp[1], one_k, inp[3], inp[4], inp[5])
    torch.cuda.synchronize()
    assert torch.equal(c1.view(torch.int32), c2.view(torch.int32)) and torch.equal(v1.view(torch.int32), v2.view(torch.int32))
    assert torch.equal(_bits(y1), _bits(enc.conv(m2)))


# ------------------------------------------------------------------------------------------- 3. the product
@functools.lru_cache(maxsize=None)
def _reference(H, W, E):
    """(s, S) of case (H, W, E) with the parameters mr.params(PRODUCT_SEED): m is the device's own."""
    w, b = mr.params(PRODUCT_SEED)
    return mr.sums(_unfused(H, W, E)[0].cpu().numpy(), w, b)


def _worst_ratio(got, s, S):
    """worst |err| / bound, and the number of elements left out of it (non-finite reference sums: there must be none)."""
    ok = np.isfinite(s) & np.isfinite(S)
    err = np.abs(got.astype(np.float64) - mr.relu(s))
    with np.errstate(invalid="ignore"):
        ratio = np.where(ok, err / mr.bound(s, S), 0.0)
    return float(ratio.max()), int((~ok).sum())


@pytest.mark.parametrize("loader", ["geometry", "conv"])
@pytest.mark.parametrize("H,W,E", mr.SHAPES)
def test_product_is_within_the_fp32_accumulation_bound(backends, H, W, E, loader):
    s, S = _reference(H, W, E)
    enc = backends.FlowEncoder(*_params(PRODUCT_SEED))
    got = enc(*_inputs(H, W, E))[0] if loader == "geometry" else enc.conv(_unfused(H, W, E)[0])
    torch.cuda.synchronize()
    got = got.cpu().numpy()
    worst, excluded = _worst_ratio(got, s, S)
    print(f"motion_encode {H}x{W} E={E} {loader}: worst |err| / bound = {worst:.4f}, excluded {excluded}")
    assert excluded == 0
    assert np.isfinite(got).all()
    assert worst <= 1.0
    assert (mr.relu(s) > 0).mean() > 0.2 and (s < 0).mean() > 0.2      # the ReLU is exercised on both sides


# ------------------------------------------------------------------------------------------- 4. both loaders agree
@pytest.mark.parametrize("H,W,E", mr.SHAPES)
def test_both_loaders_give_the_same_bits(backends, H, W, E):
    enc = backends.FlowEncoder(*_params(PRODUCT_SEED))
    inp = _inputs(H, W, E)
    fused = enc(*inp)[0]
    given = enc.conv(backends.motion_features(*inp)[0])        # [1,E,4,H,W] as motion_features returns it
    torch.cuda.synchronize()
    assert torch.equal(_bits(fused), _bits(given))


# ------------------------------------------------------------------------------------------- 5. determinism, history
def test_bits_do_not_depend_on_the_run_the_batch_or_what_ran_before(backends):
    H, W, E = 48, 64, 5
    inp = _inputs(H, W, E)
    enc = backends.FlowEncoder(*_params(PRODUCT_SEED))
    first, c_first, v_first = enc(*inp)
    again = enc(*inp)[0]
    torch.cuda.synchronize()
    assert torch.equal(_bits(first), _bits(again))
    for e in (0, 1, 3):       # alone in a batch of one: an ordinary edge, the stereo edge, one further down the batch
        alone, c_alone, _ = enc(inp[0], inp[1], inp[2], inp[3][e:e + 1].contiguous(), inp[4][e:e + 1].contiguous(),
                                inp[5][e:e + 1].contiguous())
        torch.cuda.synchronize()
        assert torch.equal(_bits(alone[0]), _bits(first[e]))
        assert torch.equal(c_alone[0, 0].view(torch.int32), c_first[0, e].view(torch.int32))
    # an unrelated kernel leaves NaN bits in the LDS (the lookup's small-plane and cooperative kernels stage their planes
    # there), and the allocator's next blocks for the outputs hold NaN bits
    nan_pyr = [torch.full_like(p, float("nan")) for p in _random_pyramid(3, 1, H, W, torch.float16)]
    junk, = backends.corr_pyramid_forward(nan_pyr, _mix_coords(7, 1, H, W), 3)
    assert bool(torch.isnan(junk).any())
    del junk, nan_pyr
    _poison_free_memory((E, mr.N, H, W), torch.float16)
    after, c_after, v_after = enc(*inp)
    _poison_free_memory((E, mr.N, H, W), torch.float16)
    after_conv = enc.conv(_unfused(H, W, E)[0])
    torch.cuda.synchronize()
    assert torch.equal(_bits(after), _bits(first)) and torch.equal(_bits(after_conv), _bits(first))
    assert torch.equal(c_after.view(torch.int32), c_first.view(torch.int32))
    assert torch.equal(v_after.view(torch.int32), v_first.view(torch.int32))


# ------------------------------------------------------------------------------------------- 6. the stock chain
def test_distance_to_the_stock_chain_is_reported(backends):
    """Reported, not asserted: the vendor library's accumulation is not ours to bound."""
    H, W, E = 48, 64, 5
    s, S = _reference(H, W, E)
    w, b = _params(PRODUCT_SEED)
    m = _unfused(H, W, E)[0]
    try:
        with torch.autocast("cuda", dtype=torch.float16):
            stock = torch.relu_(torch.nn.functional.conv2d(m, w, b, padding=3))
        torch.cuda.synchronize()
        form = "conv2d under autocast"
    except RuntimeError as err:      # the convolution library cannot run here: the same halves as unfold + matmul
        x = _windows(m).reshape(E, mr.KTOT, H * W)
        stock = torch.relu_(torch.matmul(w.half().reshape(mr.N, mr.KTOT), x) + b.half()[None, :, None]).reshape(E, mr.N, H, W)
        torch.cuda.synchronize()
        form = f"unfold + matmul ({type(err).__name__} from conv2d)"
    got = backends.FlowEncoder(w, b).conv(m)
    torch.cuda.synchronize()
    ours, _ = _worst_ratio(got.cpu().numpy(), s, S)
    theirs, _ = _worst_ratio(stock.float().cpu().numpy(), s, S)
    differ = int((_bits(got) != _bits(stock.half())).sum())
    print(f"stock chain = {form}: worst |err| / bound fused {ours:.4f}, stock {theirs:.4f}; "
          f"{differ} of {got.numel()} elements differ in bits")
    assert stock.shape == got.shape
