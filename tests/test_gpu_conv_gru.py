"""The ConvGRU on the device (include/droid_gru_hip.h), against tests/gru_ref.py.

Maps (h, w, B): 1 x 1 x 1 and 3 x 3 x 3 are all halo; 8 x 8 x 5 several images; 2 x 64 x 2 a full tile row; 5 x 9 x 2 and
11 x 13 x 3 odd sizes; 9 x 70 x 1 three tiles, so the context mean crosses tiles with a masked tail, on the element path;
30 x 40 x 1 and 48 x 64 x 1 carry the whole step and the gate bound only.  Inputs: 128 + 128 + 128 + 64 channels, and a
single 320-channel input.

1. Directed bits: constant gates, the blend's ends, selection weights at every tap and at the segment edges.
2. The stage bounds, every element, each stage from its actual inputs (the largest fractions are printed).
3. Bit equalities: phases, one concatenated input, slices, batch position, history, in place, nothing else written.
4. NaN locality.        5. The hand-over from and to the fused neighbours.        6. End to end against the stock half chain.
"""
import functools

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import conv3x3_ref as c3
import gru_ref as ref
from test_gpu_conv3x3 import _bits, _distinct, _misaligned, _same_bits, _t
from test_gpu_pyramid_slots import _poison_free_memory

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
U = ref.U
SPLIT3, SPLIT1 = ref.SPLITS
MAP_SPLITS = [(m, s) for s in ref.SPLITS for m in ref.MAPS]
FRACTIONS = {}


def _id(v):
    return "x".join(str(a) for a in v) if isinstance(v, tuple) else None


def _mk(backends, params):
    return backends.ConvGRU(**{k: (_t(w), _t(b)) for k, (w, b) in params.items()})


@functools.lru_cache(maxsize=None)
def _random_module(backends, seed=11, inputs=320):
    p = ref.random_params(seed, 128, inputs)
    return p, ref.halves(p), _mk(backends, p)


def _zero_params(inputs=320):
    return {k: (np.zeros_like(w), np.zeros_like(b)) for k, (w, b) in ref.random_params(0, 128, inputs).items()}


@functools.lru_cache(maxsize=None)
def _zero_module(backends):
    return _mk(backends, _zero_params())


def _ops(seed, splits, h, w, B):
    return [_t(a) for a in ref.operands(seed, splits, h, w, B)]


def _np(t):
    return t.detach().cpu().numpy()


def _record(stage, frac):
    worst = float(np.max(frac))
    FRACTIONS[stage] = max(FRACTIONS.get(stage, 0.0), worst)
    print("conv_gru %s: largest fraction of the bound %.3f (so far %.3f)" % (stage, worst, FRACTIONS[stage]))
    return worst


# --------------------------------------------------------------------------------------------------- 1. directed bits
@pytest.mark.parametrize("hwb,splits", MAP_SPLITS, ids=_id)
def test_zero_weights_give_half_gates_and_the_blends_ends(backends, hwb, splits):
    h, w, B = hwb
    zero = _zero_module(backends)
    net = _distinct(B, 128, h, w)
    inputs = _ops(3, splits, h, w, B)[1:]
    g0 = torch.zeros((B, 3, 128), device=DEV)
    z, rnet = zero.gates(g0, net, *inputs)
    assert z.shape == rnet.shape == (B, 128, h, w) and z.is_contiguous() and rnet.is_contiguous()
    ok, info = _same_bits(z, torch.full_like(z, 0.5))
    assert ok, info
    ok, info = _same_bits(rnet, (0.5 * net.float()).half())          # fp32 product, ONE rounding
    assert ok, info
    # z = 0 keeps net's bits, whatever the candidate is; also in place
    _, _, gru = _random_module(backends)
    g = torch.randn((B, 3, 128), device=DEV)
    z0 = torch.zeros_like(net)
    ok, info = _same_bits(gru.update(g, z0, rnet, net, *inputs), net)
    assert ok, info
    work = net.clone()
    assert gru.update(g, z0, rnet, work, *inputs, out=work) is work
    ok, info = _same_bits(work, net)
    assert ok, info
    # z = 1 with zero weights is half(tanh(g)): exactly +-1 for large |g|, never NaN
    g[:, 2, :8] = torch.tensor([20.0, -20.0, 100.0, -100.0, 9.0, -9.0, 3e38, -3e38], device=DEV)
    got = zero.update(g, torch.ones_like(net), rnet, _ops(4, (), h, w, B)[0], *inputs)
    want = np.tanh(_np(g)[:, 2].astype(np.float64))[:, :, None, None]
    err = np.abs(_np(got).astype(np.float64) - want)
    assert err.max() <= 8 * U + 2.0 ** -11, float(err.max())
    assert bool((got[:, :4].float().abs() == 1.0).all()) and bool((got[:, 6:8].float().abs() == 1.0).all())


def _selection(splits, rot, flip):
    """Selection weights [128,C,3,3]: output channel n takes (tap, channel) pair number (n + 37 rot) of the list of all
    9 taps x the special channels -- {0, 7, 31, 32} and the first and last channel of every segment -- with sign +-1."""
    edges = np.cumsum((0, 128) + tuple(splits))
    special = sorted({0, 7, 31, 32} | {int(e) for e in edges[:-1]} | {int(e) - 1 for e in edges[1:]})
    pairs = [(tap, c) for c in special for tap in range(9)]
    assert len(pairs) <= 128
    n = np.arange(128)
    pick = (n + 37 * rot) % len(pairs)
    tap, c = np.array([pairs[i][0] for i in pick]), np.array([pairs[i][1] for i in pick])
    sign = np.where((n + flip) % 2 == 0, 1.0, -1.0)
    wt = np.zeros((128, int(edges[-1]), 9), dtype=np.float32)
    wt[n, c, tap] = sign
    assert {(int(a), int(b)) for a, b in zip(tap, c)} == set(pairs)       # every tap at every special channel
    return wt.reshape(128, -1, 3, 3), tap, c, sign


@pytest.mark.parametrize("aligned", [True, False], ids=["wide", "element"])
@pytest.mark.parametrize("hwb", [(3, 3, 3), (2, 64, 2), (5, 9, 2), (11, 13, 3), (8, 8, 5)], ids=_id)
@pytest.mark.parametrize("splits", ref.SPLITS, ids=_id)
def test_selection_weights_return_the_selected_operand(backends, splits, hwb, aligned):
    h, w, B = hwb
    ops = ref.operands(21, splits, h, w, B)
    dev = [_t(a) if aligned else _misaligned(_t(a)) for a in ops]
    g = np.zeros((B, 3, 128), dtype=np.float32)
    gd = _t(g)
    for rot, flip in ((0, 0), (1, 1)):
        wt, tap, c, sign = _selection(splits, rot, flip)
        p = _zero_params(sum(splits))
        for k in ("convz", "convr", "convq"):
            p[k] = (wt, p[k][1])
        p16 = ref.halves(p)
        gru = _mk(backends, p)
        z, rnet = gru.gates(gd, *dev)
        # the selected, zero-padded operand, taken directly: window column 9 c + tap
        win = c3.window(np.concatenate(ops, axis=1).astype(np.float64)).transpose(0, 3, 1, 2)
        sel = win[:, 9 * c + tap] * sign[None, :, None, None]
        zx, bz, rx, br = ref.stage_gates(p16, g, ops[0], ops[1:])
        assert np.array_equal(zx, ref.sigmoid(sel)) and np.array_equal(rx, ref.sigmoid(sel) * ops[0].astype(np.float64))
        fz = np.abs(_np(z).astype(np.float64) - zx) / bz
        fr = np.abs(_np(rnet).astype(np.float64) - rx) / br
        assert fz.max() <= 1.0 and fr.max() <= 1.0, (rot, float(fz.max()), float(fr.max()))
        # the candidate: z = 1 returns half(tanh(+-selected operand of cat(rnet, inp...)))
        ones = torch.ones((B, 128, h, w), dtype=torch.float16, device=DEV)
        out = torch.full((B, 128, h, w), float("nan"), dtype=torch.float16, device=DEV)
        out = out if aligned else _misaligned(out)
        assert gru.update(gd, ones, rnet, dev[0], *dev[1:], out=out) is out
        rn = _np(rnet)
        winq = c3.window(np.concatenate([rn] + ops[1:], axis=1).astype(np.float64)).transpose(0, 3, 1, 2)
        selq = winq[:, 9 * c + tap] * sign[None, :, None, None]
        ox, bo = ref.stage_update(p16, g, _np(ones), rn, ops[0], ops[1:])
        assert np.abs(ox - np.tanh(selq)).max() <= 1e-15
        fo = np.abs(_np(out).astype(np.float64) - ox) / bo
        assert fo.max() <= 1.0, (rot, float(fo.max()))


# ------------------------------------------------------------------------------------------------ 2. the stage bounds
@pytest.mark.parametrize("hwb,splits", MAP_SPLITS + [(m, SPLIT3) for m in ref.BIG_MAPS], ids=_id)
def test_every_stage_is_within_its_bound_from_its_actual_inputs(backends, hwb, splits):
    h, w, B = hwb
    _, p16, gru = _random_module(backends)
    ops = ref.operands(31 + h, splits, h, w, B)
    dev = [_t(a) for a in ops]
    g = gru.context(dev[0])
    assert g.shape == (B, 3, 128) and g.dtype == torch.float32
    gx, bg = ref.stage_context(p16, ops[0])
    fg = np.abs(_np(g).astype(np.float64) - gx) / bg
    z, rnet = gru.gates(g, *dev)
    zx, bz, rx, br = ref.stage_gates(p16, _np(g), ops[0], ops[1:])
    fz = np.abs(_np(z).astype(np.float64) - zx) / bz
    fr = np.abs(_np(rnet).astype(np.float64) - rx) / br
    worst = [_record("context g", fg), _record("gate z", fz), _record("gate r * net", fr)]
    if hwb not in ref.BIG_MAPS:
        out = gru.update(g, z, rnet, *dev)
        ox, bo = ref.stage_update(p16, _np(g), _np(z), _np(rnet), ops[0], ops[1:])
        worst.append(_record("update", np.abs(_np(out).astype(np.float64) - ox) / bo))
    assert all(np.isfinite(v) for v in worst) and max(worst) <= 1.0, worst


# ------------------------------------------------------------------------------------------------- 3. bit equalities
@pytest.mark.parametrize("hwb,splits", MAP_SPLITS + [(m, SPLIT3) for m in ref.BIG_MAPS], ids=_id)
def test_fused_call_is_the_phases_and_the_concatenated_input(backends, hwb, splits):
    h, w, B = hwb
    _, _, gru = _random_module(backends)
    dev = _ops(41, splits, h, w, B)
    _poison_free_memory((B, 128, h, w), torch.float16)
    first = gru(*dev)
    assert first.shape == (B, 128, h, w) and first.dtype == torch.float16 and first.is_contiguous()
    assert not bool(torch.isnan(first).any())
    g = gru.context(dev[0])
    z, rnet = gru.gates(g, *dev)
    ok, info = _same_bits(gru.update(g, z, rnet, *dev), first)
    assert ok, info
    cat = torch.cat(dev, dim=1)
    ok, info = _same_bits(gru(cat[:, :128], cat[:, 128:]), first)                   # two slices of one [B,448,h,w]
    assert ok, info
    again = gru(*[t[None] for t in dev])                                              # the batched form, a second run
    assert again.shape == (1, B, 128, h, w)
    ok, info = _same_bits(again[0], first)
    assert ok, info
    # in place, and into a slice of a sentinel-filled buffer: nothing else is written
    work = dev[0].clone()
    assert gru(work, *dev[1:], out=work) is work
    ok, info = _same_bits(work, first)
    assert ok, info
    SENT = 0x7e2a
    buf = torch.full((B, 448, h, w), SENT, dtype=torch.int16, device=DEV).view(torch.float16)
    sl = buf[:, 192:320]
    assert gru(*dev, out=sl) is sl
    ok, info = _same_bits(sl, first)
    assert ok, info
    rest = torch.ones(448, dtype=torch.bool, device=DEV)
    rest[192:320] = False
    assert bool((buf.view(torch.int16)[:, rest] == SENT).all())
    with pytest.raises(RuntimeError, match=r"conv_gru: out must not overlap inputs\[0\]"):
        gru(cat[:, :128], cat[:, 128:], out=cat[:, 192:320])


@pytest.mark.parametrize("hwb", [(8, 8, 5), (5, 9, 5), (9, 70, 3)], ids=_id)
def test_bits_do_not_depend_on_slices_batch_position_or_history(backends, hwb):
    h, w, B = hwb
    _, _, gru = _random_module(backends)
    dev = _ops(51, SPLIT3, h, w, B)
    first = gru(*dev).clone()
    # channel slices of wider NaN-filled buffers, one per input, at odd places
    wide = [torch.full((B, t.shape[1] + 160, h, w), float("nan"), dtype=torch.float16, device=DEV) for t in dev]
    sl = [wb[:, 32 * (k + 1):32 * (k + 1) + t.shape[1]] for k, (wb, t) in enumerate(zip(wide, dev))]
    for s, t in zip(sl, dev):
        s.copy_(t)
    ok, info = _same_bits(gru(*sl), first)
    assert ok, info
    for i in (0, B - 1):                                               # alone
        ok, info = _same_bits(gru(*[t[i:i + 1] for t in dev]), first[i:i + 1])
        assert ok, (i, info)
    perm = torch.arange(B - 1, -1, -1, device=DEV)                     # another position
    ok, info = _same_bits(gru(*[t[perm] for t in dev]), first[perm])
    assert ok, info
    ok, info = _same_bits(gru(*[t[perm][:2].contiguous() for t in dev]), first[perm][:2])      # another B
    assert ok, info
    gru(*_ops(52, SPLIT3, 11, 13, 2))                                  # after another shape, into poisoned memory
    _poison_free_memory((B, 128, h, w), torch.float16)
    ok, info = _same_bits(gru(*dev), first)
    assert ok, info
    assert gru(*[t[:0] for t in dev]).shape == (0, 128, h, w)          # B = 0 launches nothing


# --------------------------------------------------------------------------------------------------- 4. NaN locality
@pytest.mark.parametrize("h,w,v,u", [(5, 9, 0, 8), (8, 8, 7, 0), (11, 13, 5, 6), (9, 70, 4, 63)])
def test_nans_stay_where_the_module_carries_them(backends, h, w, v, u):
    B, bi = 3, 1
    p = ref.random_params(61, 128, 320)
    for k in ("convz", "convr", "convq"):
        p[k][0][np.abs(p[k][0]) < 1e-4] = 0.01           # every weight takes part, as a half too
    gru = _mk(backends, p)
    dev = _ops(62, SPLIT3, h, w, B)
    clean = gru(*dev)
    assert not bool(torch.isnan(clean).any())
    inp2 = dev[2].clone()
    inp2[bi, 77, v, u] = float("nan")
    got = gru(dev[0], dev[1], inp2, dev[3])
    hit = torch.zeros((B, 128, h, w), dtype=torch.bool, device=DEV)
    hit[bi, :, max(v - 2, 0):v + 3, max(u - 2, 0):u + 3] = True       # 3 x 3 through the gates, 5 x 5 through r * net
    assert torch.equal(torch.isnan(got), hit)
    assert torch.equal(_bits(got)[~hit], _bits(clean)[~hit])
    net2 = dev[0].clone()
    net2[bi, 5, v, u] = float("nan")                                    # through the context: the whole image, no other
    got = gru(net2, *dev[1:])
    hit[:] = False
    hit[bi] = True
    assert torch.equal(torch.isnan(got), hit)
    assert torch.equal(_bits(got)[~hit], _bits(clean)[~hit])


# ----------------------------------------------------------------------------------------------------- 5. hand-over
def test_the_neighbours_outputs_enter_and_the_result_leaves_unchanged(backends):
    import motion_encode_ref as mr
    h, w, E = 8, 8, 3
    rng = np.random.default_rng(71)
    small = lambda n, c: (_t(rng.normal(0, 1 / np.sqrt(9 * c), (n, c, 3, 3)).astype(np.float32)), _t(rng.normal(0, 0.1, (n,)).astype(np.float32)))
    cenc = backends.CorrEncoder(_t(rng.normal(0, 0.07, (128, 196)).astype(np.float32)), _t(rng.normal(0, 0.1, (128,)).astype(np.float32)))
    pyramid = [_t(rng.normal(0, 1, (E, h, w, h >> l, w >> l)).astype(np.float16)) for l in range(4)]
    coords = _t(rng.uniform(0, 7, (E, 2, h, w)).astype(np.float32))
    corr = backends.Conv3x3(*small(128, 128), relu=True)(cenc(pyramid, coords))
    wt7, b7 = mr.params(5)
    fenc = backends.FlowEncoder(_t(wt7), _t(b7))
    flow = backends.Conv3x3(*small(64, 128), relu=True)(fenc.conv(_t(rng.normal(0, 2, (E, 4, h, w)).astype(np.float32))))
    assert corr.shape == (E, 128, h, w) and flow.shape == (E, 64, h, w)
    _, p16, gru = _random_module(backends)
    net, inp = _ops(72, (128,), h, w, E)
    out = gru(net, inp, corr, flow)
    ok, info = _same_bits(gru(net.clone(), inp.clone(), corr.clone(), flow.clone()), out)
    assert ok, info
    g = gru.context(net)
    z, rnet = gru.gates(g, net, inp, corr, flow)
    ox, bo = ref.stage_update(p16, _np(g), _np(z), _np(rnet), _np(net), [_np(inp), _np(corr), _np(flow)])
    assert (np.abs(_np(out).astype(np.float64) - ox) / bo).max() <= 1.0
    pair = backends.Conv3x3([small(128, 128), small(128, 128)], relu=True)
    hd, hw = pair(out)
    hd2, hw2 = pair(out.clone())
    assert torch.equal(_bits(hd), _bits(hd2)) and torch.equal(_bits(hw), _bits(hw2))
    p = lambda n: (_t(rng.normal(0, 0.03, (n, 128, 3, 3)).astype(np.float32)), _t(rng.normal(0, 0.1, (n,)).astype(np.float32)))
    heads = backends.UpdateHeads(*p(2), *p(2), *p(1))
    assert torch.equal(_bits(heads.eta(out)), _bits(heads.eta(out.clone())))
    d0, w0 = heads(hd, hw)
    d1, w1 = heads(hd.clone(), hw.clone())
    assert torch.equal(_bits(d0), _bits(d1)) and torch.equal(_bits(w0), _bits(w1))


# ----------------------------------------------------------------------------------------------------- 6. end to end
def _stock_half_chain(p16, net, inputs):
    """The module's lines as autocast runs them: F.conv2d on half tensors, every intermediate a half tensor."""
    cv = lambda k, x, pad: F.conv2d(x, _t(p16[k][0]), _t(p16[k][1]), padding=pad)
    inp = torch.cat(inputs, dim=1)
    net_inp = torch.cat([net, inp], dim=1)
    b, c, h, w = net.shape
    glo = torch.sigmoid(cv("w", net, 0)) * net
    glo = glo.view(b, c, h * w).mean(-1).view(b, c, 1, 1)
    z = torch.sigmoid(cv("convz", net_inp, 1) + cv("convz_glo", glo, 0))
    r = torch.sigmoid(cv("convr", net_inp, 1) + cv("convr_glo", glo, 0))
    q = torch.tanh(cv("convq", torch.cat([r * net, inp], dim=1), 1) + cv("convq_glo", glo, 0))
    return (1 - z) * net + z * q


@pytest.mark.parametrize("hwb", [(11, 13, 3), (48, 64, 1)], ids=_id)
def test_distance_from_the_exact_module_against_the_stock_half_chain(backends, hwb):
    h, w, B = hwb
    _, p16, gru = _random_module(backends)
    ops = ref.operands(81, SPLIT3, h, w, B)
    dev = [_t(a) for a in ops]
    exact = ref.exact(p16, ops[0], ops[1:])["out"]
    ours = np.abs(_np(gru(*dev)).astype(np.float64) - exact).max()
    stock = _stock_half_chain(p16, dev[0], dev[1:])
    assert stock.dtype == torch.float16
    theirs = np.abs(_np(stock).astype(np.float64) - exact).max()
    print("conv_gru %dx%dx%d: largest distance from the exact fp64 module, ours %.3e, stock half chain %.3e, ratio %.3f"
          % (h, w, B, ours, theirs, ours / theirs))
    assert ours <= 2 * theirs, (float(ours), float(theirs))
