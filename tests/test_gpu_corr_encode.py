"""droid_corr_encode on the device (include/droid_update_hip.h): the lookup fused with corr_encoder[0:2].

1. `a` and the channel order, bit for bit: selection weights make the sum one exact term, so the output must be the bits
   of relu(+-corr[:, sel[n]]) of corr_pyramid_forward (which the rest of the suite pins to the oracle) -- half and fp32
   pyramids, both coordinate layouts, contiguous and through a shuffled slot list with a dead slot and a repeated one.
2. The product: random parameters at nn.Conv2d's init scale, every element within tests/corr_encode_ref.bound of
   relu(s), s in float64 from the device's own lookup bits.
3. Determinism and history.   4. The shapes of CASES.   5. PyramidStore.encode.   6. The stock chain's distance (printed).
"""
import functools

import numpy as np
import pytest
import torch

import corr_encode_ref as cr
from corr_cases import NONFINITE
from test_gpu_pyramid_slots import _coords as _mix_coords, _poison_free_memory, _random_pyramid

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
# (h, w, E): 8x8 one wave, level 3 is 1x1 | 11x13 ragged, odd row starts, element-wise stores | 16x24 several
# workgroups | 30x40 and 48x64: the real plane sizes (30x40: a tail workgroup, 48x64: all 16-byte stores)
CASES = [(8, 8, 1), (11, 13, 3), (16, 24, 5), (30, 40, 3), (48, 64, 5)]
DTYPES = [torch.float16, torch.float32]
SLOTS = {3: [2, 7, 2], 5: [4, 0, -1, 3, 3]}   # cap = E: one dead slot, one slot named twice, both ends of the buffer


def _bits(x):
    return x.contiguous().view(torch.int16)


def _idx(v):
    return torch.tensor(v, dtype=torch.int64, device=DEV)


def _relu(x):
    """max(., 0) of the contract: +0 for everything that is not above zero."""
    return torch.where(x > 0, x, torch.zeros_like(x))


@functools.lru_cache(maxsize=None)
def _pyramid(h, w, E, dtype):
    """E edges' pyramids: corr_volume_pyramid on random half feature maps with C = 128 where its shape limits allow
    (fp32: the same maps widened), else random pyramids."""
    import droid_backends as db
    if h >= 8 and w >= 8 and w % 8 == 0 and (h * w) % 16 == 0:
        g = torch.Generator().manual_seed(1000 + h)
        fmaps = torch.randn((3, 1, 128, h, w), generator=g).to(torch.float16).to(dtype).to(DEV)
        rng = np.random.default_rng(h * w + E)
        return tuple(db.corr_volume_pyramid(fmaps, _idx(rng.integers(0, 3, E)), _idx(rng.integers(0, 3, E)), 4))
    return tuple(_random_pyramid(h * w, E, h, w, dtype))


@functools.lru_cache(maxsize=None)
def _coords(h, w, E):
    """[E,2,h,w]: the near / wide / far mix with the two whole-tensor-guard corners, plus integer and half-pixel
    coordinates and the non-finite pairs, on pixels 1 .. of every entry."""
    c = _mix_coords(7 * h + w, E, h, w).cpu().numpy()
    flat = c.reshape(E, 2, h * w)
    special = [(3.0, 2.0), (float(w - 1), float(h - 1)), (0.0, 0.0), (2.5, 4.5), (w - 1.5, 0.5)] + list(NONFINITE)
    for i, (x, y) in enumerate(special):
        flat[:, 0, 1 + i], flat[:, 1, 1 + i] = x, y
    return torch.from_numpy(c).to(DEV)


def _params(seed, device=DEV):
    g = torch.Generator().manual_seed(seed)
    k = 1.0 / np.sqrt(cr.KTOT)
    w = ((torch.rand((cr.N, cr.KTOT, 1, 1), generator=g) * 2 - 1) * k).to(device)
    b = ((torch.rand((cr.N,), generator=g) * 2 - 1) * k).to(device)
    return w, b


def _selection(first, flip):
    """weight[n, first + n] = +-1, everything else 0."""
    w = torch.zeros((cr.N, cr.KTOT))
    n = torch.arange(cr.N)
    sign = torch.where((n + flip) % 2 == 0, 1.0, -1.0)
    w[n, first + n] = sign
    return w.to(DEV), sign.to(DEV)


def _run(db, enc, pyr, coords, slots, layout):
    c = coords if layout == "2hw" else coords.permute(0, 2, 3, 1).contiguous()
    return enc(list(pyr), c, slots=slots, layout=layout)


def _lookup_half(db, pyr, coords, slots):
    corr, = db.corr_pyramid_forward(list(pyr), coords, 3, slots=slots)
    return corr.half()     # half pyramids: the bits themselves; fp32: autocast's cast


# ------------------------------------------------------------------------------------------- 1. a, bit for bit
@pytest.mark.parametrize("layout", ["2hw", "hw2"])
@pytest.mark.parametrize("dtype", DTYPES, ids=["f16", "f32"])
@pytest.mark.parametrize("h,w,E,mode", [c + (m,) for c in CASES for m in ("contiguous", "slots")
                                        if m == "contiguous" or c[2] in SLOTS])   # a dead and a repeated slot: E >= 3
def test_selection_weights_return_the_lookup_bits(backends, h, w, E, mode, dtype, layout):
    slots = _idx(SLOTS[E]) if mode == "slots" else None
    pyr, coords = _pyramid(h, w, E, dtype), _coords(h, w, E)
    corr = _lookup_half(backends, pyr, coords, slots)
    assert bool(torch.isfinite(corr).all()) and bool((corr != 0).any())
    zero_bias = torch.zeros(cr.N, device=DEV)
    for first, flip in ((0, 0), (68, 1)):            # k = 0 .. 127 and 68 .. 195, both signs at every k of the overlap
        wsel, sign = _selection(first, flip)
        enc = backends.CorrEncoder(wsel, zero_bias)
        _poison_free_memory((E, cr.N, h, w), torch.float16)
        got = _run(backends, enc, pyr, coords, slots, layout)
        torch.cuda.synchronize()
        want = _relu(corr[:, first:first + cr.N] * sign.half()[None, :, None, None])
        assert got.shape == (E, cr.N, h, w) and got.dtype == torch.float16
        bad = _bits(got) != _bits(want)
        assert not bool(bad.any()), (first, int(bad.sum()), torch.nonzero(bad)[:4].tolist())
    if slots is not None:
        # the dead entry with a non-zero bias, on a block of NaN bits: relu(b16) everywhere
        bias = _params(5)[1]
        enc = backends.CorrEncoder(wsel, bias)
        _poison_free_memory((E, cr.N, h, w), torch.float16)
        got = _run(backends, enc, pyr, coords, slots, layout)
        torch.cuda.synchronize()
        dead = [e for e, s in enumerate(SLOTS[E]) if not 0 <= s < E]
        assert len(dead) == 1
        want = _relu(bias.half())[:, None, None].expand(cr.N, h, w)
        assert torch.equal(_bits(got[dead[0]]), _bits(want)) and bool((want > 0).any())
        twice = [e for e, s in enumerate(SLOTS[E]) if SLOTS[E].count(s) == 2]
        assert not torch.equal(_bits(got[twice[0]]), _bits(got[twice[1]]))   # one slot, two coordinate sets


# ------------------------------------------------------------------------------------------- 2. the product
@functools.lru_cache(maxsize=None)
def _reference(h, w, E, dtype):
    """(a, s, S) of case (h, w, E) with the parameters _params(9): a from the device's own lookup."""
    import droid_backends as db
    a = _lookup_half(db, _pyramid(h, w, E, dtype), _coords(h, w, E), None).cpu().numpy()
    wt, b = _params(9, "cpu")
    s, S = cr.sums(a, wt.numpy().reshape(cr.N, cr.KTOT), b.numpy())
    return a, s, S


def _worst_ratio(got, a, s, S):
    ok = np.broadcast_to(cr.finite_mask(a), s.shape)
    err = np.abs(got.astype(np.float64) - cr.relu(s))
    ratio = np.where(ok, err / cr.bound(s, S), 0.0)
    return float(ratio.max()), int((~ok).sum())


@pytest.mark.parametrize("layout", ["2hw", "hw2"])
@pytest.mark.parametrize("dtype", DTYPES, ids=["f16", "f32"])
@pytest.mark.parametrize("h,w,E", CASES)
def test_product_is_within_the_fp32_accumulation_bound(backends, h, w, E, dtype, layout):
    a, s, S = _reference(h, w, E, dtype)
    enc = backends.CorrEncoder(*_params(9))
    got = _run(backends, enc, _pyramid(h, w, E, dtype), _coords(h, w, E), None, layout)
    torch.cuda.synchronize()
    worst, excluded = _worst_ratio(got.cpu().numpy(), a, s, S)
    print(f"corr_encode {h}x{w} E={E} {dtype} {layout}: worst |err| / bound = {worst:.4f}, excluded {excluded}")
    assert excluded == 0
    assert np.isfinite(got.cpu().numpy()).all()
    assert worst <= 1.0
    assert (cr.relu(s) > 0).mean() > 0.2 and (s < 0).mean() > 0.2      # the ReLU is exercised on both sides


# ------------------------------------------------------------------------------------------- 3. determinism, history
@pytest.mark.parametrize("dtype", DTYPES, ids=["f16", "f32"])
def test_bits_do_not_depend_on_the_run_the_batch_or_what_ran_before(backends, dtype):
    h, w, E = 48, 64, 5
    pyr, coords = _pyramid(h, w, E, dtype), _coords(h, w, E)
    enc = backends.CorrEncoder(*_params(9))
    first = _run(backends, enc, pyr, coords, None, "2hw")
    again = _run(backends, enc, pyr, coords, None, "2hw")
    torch.cuda.synchronize()
    assert torch.equal(_bits(first), _bits(again))
    for e in (0, 3):       # E = 1: alone in a batch of one, and as the one slot of a slot list
        alone = _run(backends, enc, [p[e:e + 1].contiguous() for p in pyr], coords[e:e + 1].contiguous(), None, "hw2")
        by_slot = _run(backends, enc, pyr, coords[e:e + 1].contiguous(), _idx([e]), "2hw")
        torch.cuda.synchronize()
        assert torch.equal(_bits(alone[0]), _bits(first[e])) and torch.equal(_bits(by_slot[0]), _bits(first[e]))
    # an unrelated kernel leaves NaN bits in the LDS (the lookup's small-plane and cooperative kernels stage their
    # planes there), and the allocator's next block for the output holds NaN bits
    nan_pyr = [torch.full_like(p, float("nan")) for p in _pyramid(48, 64, 1, torch.float16)]
    junk, = backends.corr_pyramid_forward(nan_pyr, coords[:1].contiguous(), 3)
    assert bool(torch.isnan(junk).any())
    del junk, nan_pyr
    _poison_free_memory((E, cr.N, h, w), torch.float16)
    after = _run(backends, enc, pyr, coords, None, "2hw")
    torch.cuda.synchronize()
    assert torch.equal(_bits(after), _bits(first))


# ------------------------------------------------------------------------------------------- 5. PyramidStore.encode
def test_store_encode_after_add_keep_add(backends):
    from droid_backends.pyramid_store import PyramidStore
    h, w = 30, 40
    g = torch.Generator().manual_seed(77)
    fmaps = torch.randn((6, 1, 128, h, w), generator=g).to(torch.float16).to(DEV)
    store = PyramidStore(fmaps, cap=8)
    store.add(_idx([0, 1, 2, 3, 4]), _idx([1, 2, 3, 4, 5]))
    store.keep([True, False, True, False, True])
    store.add(_idx([5, 0, 2]), _idx([0, 4, 2]))
    E = len(store)
    assert E == 6 and store.table.slots == [0, 2, 4, 1, 3, 5]
    enc = backends.CorrEncoder(*_params(9))
    coords1 = _coords(h, w, E).permute(0, 2, 3, 1)[None].contiguous()        # [1,E,h,w,2]
    got = store.encode(coords1, enc)
    direct = enc(store.pyramid, coords1[0], slots=store._slots_dev, layout="hw2")
    planes = enc(store.pyramid, _coords(h, w, E), slots=store._slots_dev, layout="2hw")
    corr = store(coords1)[0]                                                  # [E,196,h,w]
    torch.cuda.synchronize()
    assert got.shape == (E, cr.N, h, w) and got.dtype == torch.float16
    assert torch.equal(_bits(got), _bits(direct)) and torch.equal(_bits(got), _bits(planes))
    a = corr.cpu().numpy()
    wt, b = _params(9, "cpu")
    s, S = cr.sums(a, wt.numpy().reshape(cr.N, cr.KTOT), b.numpy())
    worst, excluded = _worst_ratio(got.cpu().numpy(), a, s, S)
    print(f"PyramidStore.encode {h}x{w} E={E}: worst |err| / bound = {worst:.4f}")
    assert excluded == 0 and worst <= 1.0


# ------------------------------------------------------------------------------------------- 6. the stock chain
@pytest.mark.parametrize("dtype", DTYPES, ids=["f16", "f32"])
def test_distance_to_the_stock_chain_is_reported(backends, dtype):
    """Reported, not asserted: the vendor library's accumulation is not ours to bound."""
    h, w, E = 48, 64, 5
    a, s, S = _reference(h, w, E, dtype)
    wt, b = _params(9)
    corr, = backends.corr_pyramid_forward(list(_pyramid(h, w, E, dtype)), _coords(h, w, E), 3)
    try:
        with torch.autocast("cuda", dtype=torch.float16):
            stock = torch.relu_(torch.nn.functional.conv2d(corr, wt, b))
        torch.cuda.synchronize()
        form = "conv2d under autocast"
    except RuntimeError as err:      # the convolution library cannot run here: the same arithmetic as a matmul
        x = corr.half().reshape(E, cr.KTOT, h * w)
        stock = torch.relu_(torch.matmul(wt.half().reshape(cr.N, cr.KTOT), x) + b.half()[None, :, None]).reshape(E, cr.N, h, w)
        torch.cuda.synchronize()
        form = f"matmul ({type(err).__name__} from conv2d)"
    got = _run(backends, backends.CorrEncoder(wt, b), _pyramid(h, w, E, dtype), _coords(h, w, E), None, "2hw")
    torch.cuda.synchronize()
    ours, _ = _worst_ratio(got.cpu().numpy(), a, s, S)
    theirs, _ = _worst_ratio(stock.float().cpu().numpy(), a, s, S)
    differ = int((_bits(got) != _bits(stock.half())).sum())
    print(f"stock chain = {form}, {dtype}: worst |err| / bound fused {ours:.4f}, stock {theirs:.4f}; "
          f"{differ} of {got.numel()} elements differ in bits")
    assert stock.shape == got.shape
