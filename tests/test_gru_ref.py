"""tests/gru_ref.py checked on the CPU: the packed layout holds every weight exactly once and unpacks to what went in;
the exact module is the stock lines of the ConvGRU written independently in torch float64; the staged contract differs
from the exact module by its three roundings only; and the package's own `pack` is the same layout."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import gru_ref as ref


def _stock(p, net, inputs):
    """droid_slam/modules/gru.py's forward, line by line, on float64 tensors."""
    t = lambda a: torch.from_numpy(np.asarray(a, dtype=np.float64))
    cv = lambda k, x, pad: F.conv2d(x, t(p[k][0]), t(p[k][1]), padding=pad)
    net = t(net)
    inp = torch.cat([t(x) for x in inputs], dim=1)
    net_inp = torch.cat([net, inp], dim=1)
    b, c, h, w = net.shape
    glo = torch.sigmoid(cv("w", net, 0)) * net
    glo = glo.view(b, c, h * w).mean(-1).view(b, c, 1, 1)
    z = torch.sigmoid(cv("convz", net_inp, 1) + cv("convz_glo", glo, 0))
    r = torch.sigmoid(cv("convr", net_inp, 1) + cv("convr_glo", glo, 0))
    q = torch.tanh(cv("convq", torch.cat([r * net, inp], dim=1), 1) + cv("convq_glo", glo, 0))
    return ((1 - z) * net + z * q).numpy(), z.numpy(), r.numpy(), q.numpy()


@pytest.mark.parametrize("hidden,splits,h,w,B", [(32, (64,), 5, 9, 2), (32, (32, 32), 3, 3, 3), (128, (128, 128, 64), 1, 1, 1),
                                                 (128, (320,), 4, 6, 1)])
def test_exact_module_is_the_stock_lines_in_float64(hidden, splits, h, w, B):
    p = ref.random_params(3, hidden, sum(splits))
    ops = ref.operands(4, splits, h, w, B, hidden)
    got = ref.exact(p, ops[0], ops[1:])
    out, z, r, q = _stock(p, ops[0], ops[1:])
    for a, b_ in ((got["out"], out), (got["z"], z), (got["r"], r), (got["q"], q)):
        assert np.abs(a - b_).max() <= 1e-13


@pytest.mark.parametrize("hidden,c_in", [(32, 96), (128, 160), (128, 448)])
def test_pack_round_trip_holds_every_weight_once(hidden, c_in):
    p16 = ref.halves(ref.random_params(5, hidden, c_in - hidden))
    # all-distinct tags instead of values: element i of the flattened parameters is the half with bit pattern i
    tags, at = {}, 0
    for k in ref.LAYERS:
        for part in (0, 1):
            n = p16[k][part].size
            tags[(k, part)] = (at + np.arange(n)).astype(np.uint32)
            at += n
    assert at == ref.packed_halves(hidden, c_in)
    back = ref.unpack(ref.pack(p16), hidden, c_in)
    for k in ref.LAYERS:
        for part in (0, 1):
            assert back[k][part].shape == p16[k][part].shape
            assert np.array_equal(back[k][part].view(np.uint16), p16[k][part].view(np.uint16)), (k, part)
    # positions: pack two 16-bit tag planes and see every index exactly once
    lo = {k: tuple((tags[(k, i)] & 0xffff).astype(np.uint16).view(np.float16).reshape(p16[k][i].shape) for i in (0, 1)) for k in ref.LAYERS}
    hi = {k: tuple((tags[(k, i)] >> 16).astype(np.uint16).view(np.float16).reshape(p16[k][i].shape) for i in (0, 1)) for k in ref.LAYERS}
    seen = ref.pack(lo).view(np.uint16).astype(np.uint32) | (ref.pack(hi).view(np.uint16).astype(np.uint32) << 16)
    assert seen.size == at and np.array_equal(np.sort(seen), np.arange(at, dtype=np.uint32))


def test_the_packages_pack_is_the_same_layout():
    from droid_backends import conv_gru
    p = ref.random_params(6, 128, 320)
    mine = conv_gru.pack({k: (torch.from_numpy(w), torch.from_numpy(b)) for k, (w, b) in p.items()})
    want = ref.pack(ref.halves(p))
    assert mine.dtype == torch.float16 and mine.numel() == want.size == ref.packed_halves(128, 448)
    assert np.array_equal(mine.numpy().view(np.uint16), want.view(np.uint16))


def test_staged_contract_is_the_exact_module_up_to_its_roundings():
    p = ref.random_params(7, 32, 64)
    ops = ref.operands(8, (64,), 5, 9, 2, 32)
    p16 = ref.halves(p)
    g, z16, rnet16, out16 = ref.staged(p, ops[0], ops[1:])
    ex = ref.exact(p16, ops[0], ops[1:])
    assert np.abs(g - ex["g"]).max() <= 1e-13
    assert np.abs(z16.astype(np.float64) - ex["z"]).max() <= 2.0 ** -11            # one rounding of a value below one
    net = ops[0].astype(np.float64)
    assert np.all(np.abs(rnet16.astype(np.float64) - ex["r"] * net) <= 2.0 ** -11 * np.abs(ex["r"] * net) + 2.0 ** -25)
    assert np.abs(out16.astype(np.float64) - ex["out"]).max() <= 0.02              # three roundings through two layers
    # the stage bounds are positive and small against values of order one
    _, bg = ref.stage_context(p16, ops[0])
    _, bz, _, br = ref.stage_gates(p16, g, ops[0], ops[1:])
    _, bo = ref.stage_update(p16, g, z16, rnet16, ops[0], ops[1:])
    for b_ in (bg, bz, br, bo):
        assert np.all(b_ > 0) and b_.max() < 0.01
