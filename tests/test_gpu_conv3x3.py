"""droid_conv3x3 on the device (include/droid_conv3x3_hip.h), against tests/conv3x3_ref.py.

The maps are the smallest at which the kernel can go wrong: 1 x 1, 1 x 2 and 3 x 3 (all halo), 8 x 8 with B = 5 (several
images inside one 64-pixel run), 2 x 64 (a full tile row), 5 x 9 and 11 x 13 (odd, no multiple of anything), 9 x 70 (a row
wider than a tile, H W no multiple of 8), 30 x 40 and 48 x 64 (the frontend's maps: several tiles, every tile shape).

1. Selection weights return the operand's bits (every tap, both signs, both activations, both store paths).
2. Impulses return every weight's bits.          3. The accumulation bound, on every case (the fractions are printed).
4. Strides: channel slices in and out.           5. The pair, and the hand-over from and to the fused neighbours.
6. Determinism and history.                      7. NaN locality.       8. The stock chain's distance (printed).
"""
import functools

import numpy as np
import pytest
import torch

import conv3x3_ref as ref
from test_gpu_pyramid_slots import _poison_free_memory

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
SPECIAL_C = lambda c_in: sorted({0, 7, 8, 31, 32 % c_in, c_in - 1})
FRACTIONS = {}      # channel configuration -> largest measured fraction of the bound (ours, stock)


def _bits(x):
    return x.contiguous().view(torch.int16)


def _same_bits(got, want):
    bad = _bits(got) != _bits(want)
    return not bool(bad.any()), (int(bad.sum()), torch.nonzero(bad)[:4].tolist())


def _act(x, relu):
    return torch.where((x > 0) | torch.isnan(x), x, torch.zeros_like(x)) if relu else x


def _t(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


@functools.lru_cache(maxsize=None)
def _distinct(B, C, h, w):
    """[B,C,h,w] half of normal, nonzero halves: all 61440 of them in a fixed shuffle, repeated with that period, so any
    two elements fewer than 61440 apart -- a pixel's neighbours in its row, column, channel and image -- differ."""
    pos = np.arange(0x0400, 0x7C00, dtype=np.uint16)
    pat = np.concatenate([pos, pos | 0x8000])
    pat = pat[np.random.default_rng(7).permutation(pat.size)]
    n = B * C * h * w
    return _t(pat[np.arange(n) % pat.size].view(np.float16).reshape(B, C, h, w))


def _misaligned(t):
    """A copy of t that begins 2 bytes past a 16-byte boundary: the element paths of the loader and of the store."""
    flat = torch.empty(t.numel() + 8, dtype=t.dtype, device=t.device)
    v = flat[1:1 + t.numel()].view(t.shape)
    v.copy_(t)
    assert v.data_ptr() % 16 == 2
    return v


def _make(backends, wt, b, k, relu):
    """Conv3x3 of k stacked layers from numpy / torch parameters [k * C_out, C_in, 3, 3]."""
    wt, b = (_t(a) if isinstance(a, np.ndarray) else a for a in (wt, b))
    if k == 1:
        return backends.Conv3x3(wt, b, relu=relu)
    return backends.Conv3x3(list(zip(wt.chunk(k), b.chunk(k))), relu=relu)


def _run(conv, x, k):
    y = conv(x)
    return torch.cat(y, dim=-3) if k > 1 else y


# ------------------------------------------------------------------------------------- 1. the operand, bit for bit
@pytest.mark.parametrize("case", ref.cases(), ids=ref.case_id)
def test_selection_weights_return_the_operand_bits(backends, case):
    c_in, c_out, k, h, w, B = case
    N = k * c_out
    x = _distinct(B, c_in, h, w)
    xm = _misaligned(x)
    win = torch.nn.functional.unfold(x.float(), 3, padding=1).reshape(B, 9 * c_in, h, w).half()   # k = 9 c + 3 ky + kx
    special = SPECIAL_C(c_in)
    n = torch.arange(N)
    seen = set()
    for r in range(9):
        for flip in range(2):
            tap = (n + r) % 9
            # the special input channels in turn, the others in between
            c = torch.where(n % 2 == 0, torch.tensor(special)[(n // 2 + r) % len(special)], (5 * n + 3 * r + 1) % c_in)
            sign = torch.where((n + flip) % 2 == 0, 1.0, -1.0)
            wt = torch.zeros((N, c_in, 9))
            wt[n, c, tap] = sign
            wt = wt.reshape(N, c_in, 3, 3).to(DEV)
            seen.update((int(a), int(b_), int(t_)) for a, b_, t_ in zip(n.tolist(), c.tolist(), tap.tolist())
                        if a in (0, 15, 16, 63, 64, N - 1))
            sel = win[:, (9 * c + tap).to(DEV)]
            want_id = sel * sign.half().to(DEV)[None, :, None, None]
            want_id[sel == 0] = 0               # a sum of zeros of either sign that starts at +0 is +0
            for relu in (False, True):
                conv = _make(backends, wt, torch.zeros(N, device=DEV), k, relu)
                want = _act(want_id, relu)
                _poison_free_memory((B, N, h, w), torch.float16)
                got = _run(conv, x, k)                                  # 16-byte path where w allows it
                ok, info = _same_bits(got, want)
                assert ok, ("aligned", r, flip, relu, info)
                if k == 1:
                    out = _misaligned(torch.full((B, N, h, w), float("nan"), dtype=torch.float16, device=DEV))
                    assert conv(xm, out=out) is out                     # element loads, element stores
                    ok, info = _same_bits(out, want)
                    assert ok, ("misaligned", r, flip, relu, info)
                else:
                    ok, info = _same_bits(_run(conv, xm, k), want)      # element loads
                    assert ok, ("misaligned x", r, flip, relu, info)
    for a in (0, 15, 16, 63, N - 1):
        assert {t_ for a_, _, t_ in seen if a_ == a} == set(range(9))      # every tap at the tile-edge channels
    assert {c_ for _, c_, _ in seen} >= set(special)


# ------------------------------------------------------------------------------------- 2. every weight, bit for bit
@pytest.mark.parametrize("h,w", [(3, 3), (5, 9)])
@pytest.mark.parametrize("chan", ref.CHANNELS + [ref.GRU_CHANNELS], ids=lambda c: "%dto%dx%d" % (c[0], c[2], c[1]))
def test_impulses_return_every_weights_bits(backends, chan, h, w):
    c_in, c_out, k = chan
    N = k * c_out
    _, wt, b = ref.operands(11, c_in, N, 1, 1, 1)
    wt, b = _t(np.where(wt == 0, np.float16(0), wt)), _t(b)       # a weight that rounded to -0 comes back as +0: make it +0
    cv, cu = h // 2, w // 2
    x = torch.zeros((c_in, c_in, h, w), dtype=torch.float16, device=DEV)
    i = torch.arange(c_in, device=DEV)
    x[i, i, cv, cu] = 1.0
    # y[b, n, v, u] = w16[n, b, cv - v + 1, cu - u + 1] inside the 3 x 3 around the centre, the bare bias elsewhere
    resp = torch.zeros((c_in, N, h, w), dtype=torch.float16, device=DEV)
    resp[:, :, cv - 1:cv + 2, cu - 1:cu + 2] = wt.flip(2, 3).permute(1, 0, 2, 3)
    got = _run(_make(backends, wt, torch.zeros_like(b), k, False), x, k)
    ok, info = _same_bits(got, resp)
    assert ok, info
    assert int((got != 0).sum()) == int((wt != 0).sum())
    got = _run(_make(backends, wt, b, k, True), x, k)
    want = _act((resp.float() + b.float()[None, :, None, None]).half(), True)       # the fp32 sum, ONE rounding
    ok, info = _same_bits(got, want)
    assert ok, info


# ------------------------------------------------------------------------------------- 3. the accumulation bound
@functools.lru_cache(maxsize=None)
def _bound_case(case):
    c_in, c_out, k, h, w, B = case
    x, wt, b = ref.operands(ref.BOUND_SEED, c_in, k * c_out, h, w, B)
    s, mag = ref.exact(x, wt, b)
    return x, wt, b, s, ref.bound(c_in, s, mag)


def _fraction(y, s, bnd, relu=True):
    want = np.maximum(s, 0.0) if relu else s            # relu moves no value by more than its argument moved
    return np.abs(y.astype(np.float64) - want) / bnd


@pytest.mark.parametrize("case", ref.cases(), ids=ref.case_id)
def test_every_element_is_within_the_accumulation_bound(backends, case):
    c_in, c_out, k, h, w, B = case
    x, wt, b, s, bnd = _bound_case(case)
    got = _run(_make(backends, wt, b, k, True), _t(x), k)
    assert got.shape == (B, k * c_out, h, w) and got.dtype == torch.float16 and got.is_contiguous()
    frac = _fraction(got.cpu().numpy(), s, bnd)
    key = "%d->%dx%d" % (c_in, k, c_out)
    FRACTIONS[key] = max(FRACTIONS.get(key, 0.0), float(frac.max()))
    print("conv3x3 %s %dx%d B=%d: largest fraction of the bound %.3f (so far for %s: %.3f)"
          % (key, h, w, B, frac.max(), key, FRACTIONS[key]))
    assert np.all(np.isfinite(frac)) and frac.max() <= 1.0, (float(frac.max()), np.argwhere(frac > 1.0)[:4].tolist())
    # without the activation the same bits where the value is above zero, and the rounded sum itself below
    lin = _run(_make(backends, wt, b, k, False), _t(x), k)
    frac = _fraction(lin.cpu().numpy(), s, bnd, relu=False)
    assert frac.max() <= 1.0, float(frac.max())
    ok, info = _same_bits(_act(lin, True), got)
    assert ok, info


# ------------------------------------------------------------------------------------- 4. strides
@pytest.mark.parametrize("h,w,B", [(5, 9, 2), (8, 8, 5), (2, 64, 2), (11, 13, 3), (30, 40, 2)])
@pytest.mark.parametrize("c_in,c_out", [(128, 128), (128, 64), (64, 128)])
def test_channel_slices_in_and_out_give_the_contiguous_bits(backends, c_in, c_out, h, w, B):
    x, wt, b = ref.operands(5, c_in, c_out, h, w, B)
    x = _t(x)
    conv = _make(backends, wt, b, 1, True)
    base = conv(x)
    wide = torch.full((B, 448, h, w), float("nan"), dtype=torch.float16, device=DEV)
    lo = 448 - c_in - 32
    wide[:, lo:lo + c_in] = x
    ok, info = _same_bits(conv(wide[:, lo:lo + c_in]), base)
    assert ok, info
    SENT = 0x7e2a       # a NaN pattern no computation gives
    buf = torch.full((B, 448, h, w), SENT, dtype=torch.int16, device=DEV).view(torch.float16)
    for first in (256, 0, 448 - c_out):
        buf.view(torch.int16).fill_(SENT)
        sl = buf[:, first:first + c_out]
        assert conv(wide[:, lo:lo + c_in], out=sl) is sl
        ok, info = _same_bits(sl, base)
        assert ok, (first, info)
        rest = torch.ones(448, dtype=torch.bool, device=DEV)
        rest[first:first + c_out] = False
        assert bool((buf.view(torch.int16)[:, rest] == SENT).all())
    # the batched form, into a batched slice
    buf.view(torch.int16).fill_(SENT)
    got = conv(x[None], out=buf[None][:, :, 64:64 + c_out])
    assert got.shape == (1, B, c_out, h, w)
    ok, info = _same_bits(got[0], base)
    assert ok, info
    assert conv(x[None]).shape == (1, B, c_out, h, w)
    with pytest.raises(RuntimeError, match="conv3x3: out must not overlap x"):
        conv(wide[:, lo:lo + c_in], out=wide[:, lo - 32:lo - 32 + c_out])
    sl = wide[:, :c_out]          # two slices of one buffer that do not touch
    conv(wide[:, lo:lo + c_in], out=sl)
    ok, info = _same_bits(sl, base)
    assert ok, info


# ------------------------------------------------------------------------------------- 5. the pair and the hand-over
@pytest.mark.parametrize("h,w,E", [(5, 9, 2), (8, 8, 5), (30, 40, 2), (48, 64, 1)])
def test_the_pair_is_its_two_layers_and_feeds_update_heads(backends, h, w, E):
    net, wt, b = ref.operands(21, 128, 256, h, w, E)
    net, wt, b = _t(net), _t(wt), _t(b)
    pair = backends.Conv3x3([(wt[:128], b[:128]), (wt[128:], b[128:])], relu=True)
    hd, hw = pair(net)
    assert hd.shape == hw.shape == (E, 128, h, w) and hd.is_contiguous() and hw.is_contiguous()
    for got, sl in ((hd, slice(0, 128)), (hw, slice(128, 256))):
        ok, info = _same_bits(got, backends.Conv3x3(wt[sl].float(), b[sl].float(), relu=True)(net))
        assert ok, info
    hd5, hw5 = pair(net[None])
    assert hd5.shape == (1, E, 128, h, w) and torch.equal(_bits(hd5[0]), _bits(hd)) and torch.equal(_bits(hw5[0]), _bits(hw))
    rng = np.random.default_rng(2)
    p = lambda n: (_t(rng.normal(0, 0.03, (n, 128, 3, 3)).astype(np.float32)), _t(rng.normal(0, 0.1, (n,)).astype(np.float32)))
    heads = backends.UpdateHeads(*p(2), *p(2), *p(1))
    d0, w0 = heads(hd, hw)
    d1, w1 = heads(hd.clone(), hw.clone())
    assert torch.equal(_bits(d0), _bits(d1)) and torch.equal(_bits(w0), _bits(w1))
    eta0 = heads.eta(hd)
    assert torch.equal(_bits(eta0), _bits(heads.eta(hd.clone())))


def test_the_encoders_outputs_enter_unchanged(backends):
    """What FlowEncoder.conv returns ([E,128,h,w] half, contiguous) is what Conv3x3 takes."""
    import motion_encode_ref as mr
    h, w, E = 11, 13, 3
    wt7, b7 = mr.params(5)
    enc = backends.FlowEncoder(_t(wt7), _t(b7))
    motn = _t(np.random.default_rng(1).normal(0, 2, (E, 4, h, w)).astype(np.float32))
    flow = enc.conv(motn)
    _, wt, b = ref.operands(8, 128, 64, h, w, E)
    conv = _make(backends, wt, b, 1, True)
    got = conv(flow)
    assert got.shape == (E, 64, h, w)
    s, mag = ref.exact(flow.cpu().numpy(), wt, b)
    assert _fraction(got.cpu().numpy(), s, ref.bound(128, s, mag)).max() <= 1.0
    ok, info = _same_bits(conv(flow.clone()), got)
    assert ok, info


# ------------------------------------------------------------------------------------- 6. determinism and history
@pytest.mark.parametrize("c_in,c_out,k", [(128, 128, 1), (128, 128, 2), (128, 64, 1)])
@pytest.mark.parametrize("h,w", [(8, 8), (5, 9), (30, 40)])
def test_bits_do_not_depend_on_run_batch_position_or_history(backends, c_in, c_out, k, h, w):
    B = 5
    x, wt, b = ref.operands(31, c_in, k * c_out, h, w, B)
    x = _t(x)
    conv = _make(backends, wt, b, k, True)
    first = _run(conv, x, k).clone()
    assert torch.equal(_bits(_run(conv, x, k)), _bits(first))
    for i in range(B):                                            # alone
        assert torch.equal(_bits(_run(conv, x[i:i + 1], k)), _bits(first[i:i + 1])), i
    perm = torch.tensor([3, 0, 4, 2, 1], device=DEV)              # another position, another B
    assert torch.equal(_bits(_run(conv, x[perm], k)), _bits(first[perm]))
    assert torch.equal(_bits(_run(conv, x[perm][:3].contiguous(), k)), _bits(first[perm][:3]))
    # after another shape, another layer, and into memory that held NaNs
    other = _make(backends, *ref.operands(32, 64, 128, 9, 70, 1)[1:], 1, False)
    other(_t(ref.operands(32, 64, 128, 9, 70, 1)[0]))
    _poison_free_memory((k, B, c_out, h, w), torch.float16)
    assert torch.equal(_bits(_run(conv, x, k)), _bits(first))
    assert _run(conv, x[:0], k).shape == (0, k * c_out, h, w)    # B = 0 launches nothing


# ------------------------------------------------------------------------------------- 7. NaN locality
@pytest.mark.parametrize("h,w,v,u", [(5, 9, 0, 8), (8, 8, 7, 0), (11, 13, 5, 6), (9, 70, 4, 63), (30, 40, 15, 31), (1, 2, 0, 1)])
@pytest.mark.parametrize("c_in,c_out,k", [(128, 128, 2), (64, 128, 1)])
def test_a_nan_reaches_its_windows_and_nothing_else(backends, c_in, c_out, k, h, w, v, u):
    B, bi, ci = 3, 1, c_in - 3
    x, wt, b = ref.operands(41, c_in, k * c_out, h, w, B)
    wt[wt == 0] = np.float16(0.01)            # every weight takes part
    x = _t(x)
    conv = _make(backends, wt, b, k, False)
    clean = _run(conv, x, k)
    assert not bool(torch.isnan(clean).any())
    x2 = x.clone()
    x2[bi, ci, v, u] = float("nan")
    got = _run(conv, x2, k)
    hit = torch.zeros((B, k * c_out, h, w), dtype=torch.bool, device=DEV)
    hit[bi, :, max(v - 1, 0):v + 2, max(u - 1, 0):u + 2] = True
    assert torch.equal(torch.isnan(got), hit)
    assert torch.equal(_bits(got)[~hit], _bits(clean)[~hit])
    relu = _run(_make(backends, wt, b, k, True), x2, k)          # the ReLU keeps them
    assert torch.equal(torch.isnan(relu), hit)


# ------------------------------------------------------------------------------------- 8. the stock chain's distance
@pytest.mark.parametrize("case", [(128, 128, 1, 48, 64, 1), (128, 64, 1, 30, 40, 1), (128, 128, 2, 11, 13, 3),
                                  (448, 128, 1, 11, 13, 3)], ids=ref.case_id)
def test_report_the_stock_chains_distance(backends, case):
    """Reported, not asserted: autocast runs F.conv2d on half tensors, then relu_."""
    c_in, c_out, k, h, w, B = case
    x, wt, b, s, bnd = _bound_case(case)
    ours = _fraction(_run(_make(backends, wt, b, k, True), _t(x), k).cpu().numpy(), s, bnd).max()
    stock = torch.nn.functional.conv2d(_t(x), _t(wt), _t(b), padding=1).relu_()
    theirs = _fraction(stock.cpu().numpy(), s, bnd).max()
    print("conv3x3 %s: largest fraction of the bound, ours %.3f, stock conv2d + relu_ %.3f" % (ref.case_id(case), ours, theirs))
    assert ours <= 1.0
