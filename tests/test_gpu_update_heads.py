"""droid_update_heads on the device (include/droid_heads_hip.h) against tests/update_heads_ref.py: every tap and the
operand bit for bit, the activations on exact sums, the product within the bound of the restatement, independence of the
batch, the other head and the memory's history, and the hand-over of the results to `ba_inputs`."""
import numpy as np
import pytest
import torch

import update_heads_ref as uh
from test_gpu_pyramid_slots import _poison_free_memory

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
KINDS = (uh.IDENTITY, uh.SIGMOID, uh.SOFTPLUS_CENTI)


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _bits(t):
    return t.contiguous().view(torch.int16).cpu().numpy().view(np.uint16)


def _run(backends, heads):
    """heads = [(x [B,128,H,W] float16 numpy or device tensor, weight, bias, kind)], one or two: the raw launch of the
    class, with any activation in any slot.  Returns the outputs as device tensors [B,H,W,n]."""
    from droid_backends import update_heads as mod
    xs = [h[0] if isinstance(h[0], torch.Tensor) else _dev(h[0]) for h in heads]
    packed = [mod.pack(_dev(np.asarray(h[1], np.float32)), _dev(np.asarray(h[2], np.float32))) for h in heads]
    n_out = [int(np.asarray(h[1]).shape[0]) for h in heads]
    return backends.UpdateHeads._run("update_heads", xs, packed, n_out, [h[3] for h in heads])


def _same(a, b):
    return a.shape == b.shape and np.array_equal(a, b)


# ------------------------------------------------------------------------------------------- 1. every tap, bit for bit
def _impulses(iv, iu):
    x = np.zeros((128, 128, 5, 5), np.float16)
    x[np.arange(128), np.arange(128), iv, iu] = 1.0
    return x


def _taps_expected(w16, iv, iu):
    """out[b, iv + 1 - ky, iu + 1 - kx, n] = w16[n, b, ky, kx] where that pixel exists, +0 everywhere else."""
    n = w16.shape[0]
    want = np.zeros((128, 5, 5, n), np.float16)
    hits = 0
    for ky in range(3):
        for kx in range(3):
            v, u = iv + 1 - ky, iu + 1 - kx
            if 0 <= v < 5 and 0 <= u < 5:
                want[:, v, u, :] = w16[:, :, ky, kx].T
                hits += 1
    return want, hits


@pytest.mark.parametrize("iv,iu", [(2, 2), (0, 0), (0, 4), (4, 0), (4, 4)])
def test_every_tap_bit_for_bit(backends, iv, iu):
    rng = np.random.default_rng(100 + 5 * iv + iu)
    x = _impulses(iv, iu)
    other = uh.hidden(128, 5, 5, 3)
    zero2, zero1 = np.zeros(2, np.float32), np.zeros(1, np.float32)
    w2 = uh.half(rng.uniform(-1, 1, (2, 128, 3, 3)))
    w1 = uh.half(rng.uniform(-1, 1, (1, 128, 3, 3)))
    wo, bo = uh.params(uh.SIGMOID, 4)
    assert (w2 != 0).all() and (w1 != 0).all()
    want2, hits = _taps_expected(w2, iv, iu)
    want1, _ = _taps_expected(w1, iv, iu)
    assert hits == (9 if (iv, iu) == (2, 2) else 4)      # at a corner the taps falling outside are simply absent
    first, _ = _run(backends, [(x, w2, zero2, uh.IDENTITY), (other, wo, bo, uh.SIGMOID)])
    _, second = _run(backends, [(other, wo, bo, uh.SIGMOID), (x, w2, zero2, uh.IDENTITY)])
    alone, = _run(backends, [(x, w2, zero2, uh.IDENTITY)])
    one, = _run(backends, [(x, w1, zero1, uh.IDENTITY)])
    one_second = _run(backends, [(other, wo, bo, uh.SIGMOID), (x, w1, zero1, uh.IDENTITY)])[1]
    for got in (first, second, alone):
        assert _same(_bits(got), want2.view(np.uint16))
    for got in (one, one_second):
        assert _same(_bits(got), want1.view(np.uint16))


# ------------------------------------------------------------------------------------------- 2. the operand, bit for bit
def _shifted(x, c, ky, kx):
    """x[:, c] shifted by (ky - 1, kx - 1), zero-filled: [B,H,W] float16."""
    B, _, H, W = x.shape
    p = np.zeros((B, H + 2, W + 2), np.float16)
    p[:, 1:-1, 1:-1] = x[:, c]
    return p[:, ky:ky + H, kx:kx + W]


@pytest.mark.parametrize("H,W,B", uh.SHAPES)
def test_the_operand_bit_for_bit(backends, H, W, B):
    x = uh.hidden(B, H, W, 2)
    xd = _dev(x)
    zero2, zero1 = np.zeros(2, np.float32), np.zeros(1, np.float32)
    nonzero = 0
    for c in (0, 31, 32, 127):
        for ky in range(3):
            for kx in range(3):
                w2 = np.zeros((2, 128, 3, 3), np.float32)
                w2[0, c, ky, kx], w2[1, c, 2 - ky, 2 - kx] = 1.0, -1.0
                w1 = np.zeros((1, 128, 3, 3), np.float32)
                w1[0, c, ky, kx] = -1.0
                plus = _shifted(x, c, ky, kx)
                minus = np.float16(0) - _shifted(x, c, 2 - ky, 2 - kx)      # +0 where x is zero: 0 * -1 added to +0
                got2, got1 = _run(backends, [(xd, w2, zero2, uh.IDENTITY), (xd, w1, zero1, uh.IDENTITY)])
                g2 = _bits(got2)
                assert _same(g2[..., 0], plus.view(np.uint16)), (c, ky, kx)
                assert _same(g2[..., 1], minus.view(np.uint16)), (c, ky, kx)
                assert _same(_bits(got1)[..., 0], (np.float16(0) - plus).view(np.uint16)), (c, ky, kx)
                nonzero += int(plus.any())
    assert nonzero > 0
    if H * W > 1:
        assert nonzero == 36


# ------------------------------------------------------------------------------------------- 3. activations on exact sums
SIGMOID_T = [0.0] + [s * v for v in (2.0 ** -14, 1.0, 8.0, 17.0, 30.0, 89.0, 104.0, 65504.0) for s in (1.0, -1.0)]
SOFTPLUS_T = [-104.0, -89.0, -20.0, -1.0, 0.0, 1.0, 19.98, 20.0, 20.02, 30.0, 88.8, 1000.0]


def _activation_case(backends, kind, values):
    """x = 0, so t = float(b16) at every pixel, borders included."""
    H, W, B = 3, 5, 2
    x = np.zeros((B, 128, H, W), np.float16)
    w, _ = uh.params(kind, 5)
    b = np.asarray(values, np.float32)
    got, = _run(backends, [(x, w, b, kind)])
    got = got.float().cpu().numpy().astype(np.float64)
    t, S = uh.sums(x, w, b)
    assert np.array_equal(t[0, 0, 0], uh.half(b).astype(np.float64)) and np.array_equal(S, np.abs(t))
    want, bd = uh.act(kind, t), uh.bound(kind, t, S)
    assert np.isfinite(got).all(), (values, got[0, 0, 0])
    ratio = np.abs(got - want) / bd
    print(f"update_heads activation {kind} t = {list(t[0, 0, 0])}: got {list(got[0, 0, 0])}, want {list(want[0, 0, 0])}, "
          f"worst ratio {ratio.max():.3f}")
    assert ratio.max() < 1.0, (values, got[0, 0, 0], want[0, 0, 0])
    exact = np.isin(uh.half(want).astype(np.float64), (0.0, 1.0))
    assert np.array_equal(got[exact], uh.half(want).astype(np.float64)[exact]), (values, got[0, 0, 0])
    return exact.any()


def test_sigmoid_on_exact_sums(backends):
    vals = SIGMOID_T + [0.0]
    assert len(vals) % 2 == 0
    exact = [_activation_case(backends, uh.SIGMOID, vals[i:i + 2]) for i in range(0, len(vals), 2)]
    assert any(exact)      # the saturated ends were reached


def test_softplus_centi_on_exact_sums(backends):
    for v in SOFTPLUS_T:     # 88.8: a missing threshold or an overflowing exp gives inf here
        _activation_case(backends, uh.SOFTPLUS_CENTI, [v])


# ------------------------------------------------------------------------------------------- 4. the product
def _stock(x, w, b, kind):
    """The stock half chain on the device, as information: conv2d under autocast, the activation, `.01 *`."""
    with torch.autocast("cuda", dtype=torch.float16):
        y = torch.nn.functional.conv2d(x, _dev(w), _dev(b), padding=1)
        if kind == uh.SIGMOID:
            y = torch.sigmoid(y)
        elif kind == uh.SOFTPLUS_CENTI:
            y = .01 * torch.nn.functional.softplus(y)
    return y.permute(0, 2, 3, 1).float().cpu().numpy().astype(np.float64)


@pytest.mark.parametrize("H,W,B", uh.SHAPES)
def test_the_product_within_the_bound(backends, H, W, B):
    xs = {kind: uh.hidden(B, H, W, 10 + kind) for kind in KINDS}
    par = {kind: uh.params(kind, 6) for kind in KINDS}
    heads = backends.UpdateHeads(*[_dev(a) for kind in KINDS for a in par[kind]])
    delta, weight = heads(_dev(xs[uh.IDENTITY]), _dev(xs[uh.SIGMOID])[None])
    eta = heads.eta(_dev(xs[uh.SOFTPLUS_CENTI]))
    assert delta.shape == weight.shape == (1, B, H, W, 2) and eta.shape == (1, B, H, W)
    assert delta.dtype == weight.dtype == eta.dtype == torch.float16
    assert delta.is_contiguous() and weight.is_contiguous() and eta.is_contiguous()
    got = {uh.IDENTITY: delta[0], uh.SIGMOID: weight[0], uh.SOFTPLUS_CENTI: eta[0][..., None]}
    for kind in KINDS:
        w, b = par[kind]
        t, S = uh.sums(xs[kind], w, b)
        want, bd = uh.act(kind, t), uh.bound(kind, t, S)
        g = got[kind].float().cpu().numpy().astype(np.float64)
        ratio = np.abs(g - want) / bd
        stock = np.abs(_stock(_dev(xs[kind]), w, b, kind) - want) / bd
        print(f"update_heads {H}x{W} B={B} act {kind}: worst |device - exact| / bound {ratio.max():.3f}; "
              f"the stock half chain: {stock.max():.2f} bounds")
        assert ratio.max() < 1.0, (kind, float(ratio.max()))      # every element, nothing excluded


# ------------------------------------------------------------------------------------------- 5. independence
@pytest.mark.parametrize("H,W,B", [(11, 13, 3), (48, 64, 5)])
def test_batch_position_the_other_head_and_history_do_not_matter(backends, H, W, B):
    x, y = uh.hidden(B, H, W, 20), uh.hidden(B, H, W, 21)
    (wi, bi), (ws, bs), (we, be) = (uh.params(kind, 7) for kind in KINDS)
    xd, yd = _dev(x), _dev(y)
    a0, b0 = (_bits(t) for t in _run(backends, [(xd, wi, bi, uh.IDENTITY), (yd, ws, bs, uh.SIGMOID)]))
    a1, b1 = (_bits(t) for t in _run(backends, [(xd, wi, bi, uh.IDENTITY), (yd, ws, bs, uh.SIGMOID)]))
    assert _same(a0, a1) and _same(b0, b1)                                   # two runs
    _poison_free_memory((B, H, W, 2), torch.float16)
    _poison_free_memory((B, H, W, 2), torch.float16)
    a2, b2 = (_bits(t) for t in _run(backends, [(xd, wi, bi, uh.IDENTITY), (yd, ws, bs, uh.SIGMOID)]))
    assert _same(a0, a2) and _same(b0, b2)                                   # after poisoning free memory
    b3, a3 = (_bits(t) for t in _run(backends, [(yd, ws, bs, uh.SIGMOID), (xd, wi, bi, uh.IDENTITY)]))
    assert _same(a0, a3) and _same(b0, b3)                                   # the other slot
    a4, e4 = (_bits(t) for t in _run(backends, [(xd, wi, bi, uh.IDENTITY), (xd, we, be, uh.SOFTPLUS_CENTI)]))
    assert _same(a0, a4)                                                     # the other head changed (n_out too)
    assert _same(e4, _bits(_run(backends, [(xd, we, be, uh.SOFTPLUS_CENTI)])[0]))
    for e in range(B):                                                       # alone, B = 1, in either slot
        xe, ye = xd[e:e + 1].contiguous(), yd[B - 1 - e:B - e].contiguous()
        alone, = _run(backends, [(xe, wi, bi, uh.IDENTITY)])
        assert _same(_bits(alone)[0], a0[e]), e
        _, second = _run(backends, [(ye, ws, bs, uh.SIGMOID), (xe, wi, bi, uh.IDENTITY)])
        assert _same(_bits(second)[0], a0[e]), e


@pytest.mark.parametrize("H,W,B", [(11, 13, 3), (9, 70, 2), (48, 64, 5)])
def test_a_nan_and_an_inf_reach_exactly_their_windows(backends, H, W, B):
    x, y = uh.hidden(B, H, W, 22).copy(), uh.hidden(B, H, W, 23)
    (wi, bi), (ws, bs) = uh.params(uh.IDENTITY, 8), uh.params(uh.SIGMOID, 8)
    clean = [_bits(t) for t in _run(backends, [(x, wi, bi, uh.IDENTITY), (y, ws, bs, uh.SIGMOID)])]
    spots = [(0, 5, H - 1, W - 1, np.nan), (B - 1, 127, H // 2, min(W - 1, 64), np.inf)]
    hit = np.zeros((B, H, W), bool)
    for b, c, v, u, value in spots:
        x[b, c, v, u] = value
        hit[b, max(v - 1, 0):v + 2, max(u - 1, 0):u + 2] = True
    got = _run(backends, [(x, wi, bi, uh.IDENTITY), (y, ws, bs, uh.SIGMOID)])
    g0 = got[0].float().cpu().numpy()
    assert not np.isfinite(g0[hit]).any()                 # w16 has no zeros, so every output of a window is reached
    assert (uh.half(wi) != 0).all()
    assert _same(_bits(got[0])[~hit], clean[0][~hit])     # every other output keeps its bits
    assert _same(_bits(got[1]), clean[1])                 # and the other head all of them


# ------------------------------------------------------------------------------------------- 6. hand-over to ba_inputs
def test_results_go_to_ba_inputs_unchanged(backends):
    H, W, E, G, nbuf = 11, 13, 5, 3, 6
    par = {kind: uh.params(kind, 9) for kind in KINDS}
    heads = backends.UpdateHeads(*[_dev(a) for kind in KINDS for a in par[kind]])
    delta, weight = heads(_dev(uh.hidden(E, H, W, 30)), _dev(uh.hidden(E, H, W, 31)))
    eta = heads.eta(_dev(uh.hidden(G, H, W, 32))[None])
    ii = torch.tensor([1, 1, 2, 4, 4], dtype=torch.int64, device=DEV)
    jj = torch.tensor([2, 3, 1, 3, 5], dtype=torch.int64, device=DEV)
    g = torch.Generator(device=DEV).manual_seed(5)
    coords1 = 20 * torch.rand((1, E, H, W, 2), generator=g, device=DEV)

    def run(d, w, e):
        buf = torch.zeros((nbuf, H, W), device=DEV)
        r = backends.ba_inputs(coords1, d, w, e, buf, ii, jj)
        return [r.target_state, r.weight_state, r.target, r.weight, r.eta, buf, r.ii, r.jj, r.frames]

    got = run(delta, weight, eta)
    want = run(delta.clone().contiguous(), weight.clone().contiguous(), eta.clone().contiguous())
    for a, b in zip(got, want):
        assert a.shape == b.shape and a.dtype == b.dtype and torch.equal(a.view(torch.int32) if a.dtype == torch.float32 else a,
                                                                         b.view(torch.int32) if b.dtype == torch.float32 else b)
    # and what went in is what the update operator would have handed over: target = coords1 + delta, eta from damping
    assert torch.equal(got[0], coords1 + delta.float()) and torch.equal(got[1], weight.float())
    assert float(got[4].min()) > 0
