"""The ConvGRU of the update operator on the device (droid_slam/modules/gru.py, h_planes = 128; droid_net.py:127).

Under autocast the stock module runs about 25 launches -- three torch.cat, the 1 x 1 convolution, sigmoid, product and mean
of the global context, three 1 x 1 convolutions on [E,128,1,1], three 3 x 3 convolutions over 448 channels, and the
pointwise tail -- and rounds every intermediate to half.  `ConvGRU` computes it in four launches that read the inputs
where they lie, without a cat (droid_conv_gru, include/droid_gru_hip.h, which states the arithmetic).

    gru = ConvGRU.from_module(update.gru)      # or ConvGRU(convz=(w, b), convr=..., convq=..., w=..., convz_glo=..., ...)
    net = gru(net, inp, corr, flow)            # 1..4 inputs after net; [E,C,h,w] or [1,E,C,h,w] half; channel slices allowed
    gru(net, inp, corr, flow, out=net)         # in place
    g = gru.context(net); z, rnet = gru.gates(g, net, inp, corr, flow); net2 = gru.update(g, z, rnet, net, inp, corr, flow)
"""
from __future__ import annotations

import ctypes

import torch

from . import _lib
from ._args import ScratchCache, _stream, _ws_key, check_tensors
from .conv3x3 import _no_grad, _overlap, _planes
from .conv3x3 import pack as _pack_conv

HIDDEN, SLAB = 128, 32
F16, F32, F16_OR_F32 = torch.float16, torch.float32, (torch.float16, torch.float32)
LAYERS = ("convz", "convr", "convq", "w", "convz_glo", "convr_glo", "convq_glo")
_ws = ScratchCache()   # _ws_key(device) -> grow-only uint8 scratch of the ConvGRU calls


def supported(c_in):
    """The input widths of the contract: the channels of cat(net, inp...), a multiple of 32 in [160, 512]."""
    return 160 <= c_in <= 512 and c_in % SLAB == 0


def pack(params):
    """The packed parameters (include/droid_gru_hip.h) from {layer: (weight, bias)}: halves, [Wz; Wr] and Wq in
    droid_conv3x3's fragment layout without a bias, w as [4][8][64][8], the three context matrices row-major, then
    bw, bz, br, bq, bzg, brg, bqg."""
    h = lambda t: t.detach().to(F16)
    wz, wr, wq = (h(params[k][0]) for k in ("convz", "convr", "convq"))
    none = torch.zeros(0, dtype=F16, device=wz.device)
    w1 = h(params["w"][0]).reshape(HIDDEN // 16, 16, HIDDEN // SLAB, 4, 8)           # (nt, c16, s, g, j)
    parts = [_pack_conv(torch.cat([wz, wr]), none), _pack_conv(wq, none), w1.permute(2, 0, 3, 1, 4).reshape(-1)]
    parts += [h(params[k][0]).reshape(-1) for k in ("convz_glo", "convr_glo", "convq_glo")]
    parts += [h(params[k][1]).reshape(-1) for k in ("w", "convz", "convr", "convq", "convz_glo", "convr_glo", "convq_glo")]
    return torch.cat(parts).contiguous()


class ConvGRU:
    """The module's seven layers as (weight, bias) pairs, fp32 or half, on the device: convz, convr, convq
    [128,C,3,3] / [128] with C = 128 + the channels of the inputs; w, convz_glo, convr_glo, convq_glo [128,128,1,1] (or
    [128,128]) / [128].  They are rounded to half (autocast's cast) and packed once; rebuild the object after the weights
    change.  Inference only."""

    def __init__(self, convz, convr, convq, w, convz_glo, convr_glo, convq_glo):
        what = "ConvGRU"
        given = dict(zip(LAYERS, (convz, convr, convq, w, convz_glo, convr_glo, convq_glo)))
        for name, pair in given.items():
            if not isinstance(pair, (list, tuple)) or len(pair) != 2:
                raise RuntimeError(f"{what}: {name} must be a (weight, bias) pair")
        tensors = [(t, f"{name}.{part}", F16_OR_F32) for name, pair in given.items() for t, part in zip(pair, ("weight", "bias"))]
        check_tensors(what, tensors, placement=False)
        c_in = int(convz[0].shape[1]) if convz[0].dim() == 4 else -1
        for name in LAYERS[:3]:
            wt = given[name][0]
            if wt.dim() != 4 or tuple(wt.shape[2:]) != (3, 3) or int(wt.shape[0]) != HIDDEN or not supported(int(wt.shape[1])):
                raise RuntimeError(f"{what}: {name}.weight must be [{HIDDEN},C,3,3] with C a multiple of 32 in 160 .. 512, "
                                   f"got {list(wt.shape)}")
            if int(wt.shape[1]) != c_in:
                raise RuntimeError(f"{what}: {name}.weight must have the {c_in} input channels of convz.weight, got "
                                   f"{list(wt.shape)}")
        for name in LAYERS[3:]:
            wt = given[name][0]
            if tuple(wt.shape) not in ((HIDDEN, HIDDEN, 1, 1), (HIDDEN, HIDDEN)):
                raise RuntimeError(f"{what}: {name}.weight must be [{HIDDEN},{HIDDEN},1,1], got {list(wt.shape)}")
        for name in LAYERS:
            if tuple(given[name][1].shape) != (HIDDEN,):
                raise RuntimeError(f"{what}: {name}.bias must be [{HIDDEN}], got {list(given[name][1].shape)}")
        check_tensors(what, tensors, types=False, contiguous=False, on=(convz[0], "convz.weight"))
        self.c_in = c_in
        lib = _lib.load()
        self.packed = pack(given)
        assert self.packed.numel() * 2 == lib.droid_gru_packed_bytes(self.c_in)

    @classmethod
    def from_module(cls, m):
        """From any object with the attributes convz, convr, convq, w, convz_glo, convr_glo and convq_glo, each with a
        weight and a bias: the reference's ConvGRU as it is."""
        for name in LAYERS:
            layer = getattr(m, name, None)
            if layer is None or not hasattr(layer, "weight") or getattr(layer, "bias", None) is None:
                raise RuntimeError(f"ConvGRU: the module has no layer {name} with a weight and a bias")
        return cls(*[(getattr(m, name).weight, getattr(m, name).bias) for name in LAYERS])

    # ------------------------------------------------------------------------------------------------ argument checks
    def _inputs(self, what, net, inputs, extra=()):
        """The first half of a call's checks -- types and shapes, a caller's mistake named before the device is looked
        at; `_placed` is the second.  extra = [(tensor, name, dtype)] come after the inputs.  Returns (rows of net, rows
        of the inputs, batched, every tensor)."""
        if not 1 <= len(inputs) <= 4:
            raise RuntimeError(f"{what}: takes 1 to 4 inputs after net, got {len(inputs)}")
        tensors = [(net, "net", F16)] + [(x, f"inputs[{k}]", F16) for k, x in enumerate(inputs)] + list(extra)
        check_tensors(what, tensors, placement=False)
        rows, batched = _planes(what, net, "net", HIDDEN)
        B, _, h, w = (int(v) for v in rows.shape)
        xs, total = [], HIDDEN
        for k, x in enumerate(inputs):
            name = f"inputs[{k}]"
            lead = x.dim() == 5 and x.shape[0] == 1
            ch = int(x.shape[2 if lead else 1]) if x.dim() in (4, 5) else -1
            if x.dim() not in (4, 5) or ch < SLAB or ch % SLAB != 0:
                raise RuntimeError(f"{what}: {name} must be [B,C,h,w] or [1,B,C,h,w] with C a positive multiple of {SLAB}, "
                                   f"got {list(x.shape)}")
            r, bt = _planes(what, x, name, ch)
            if bt != batched or (int(r.shape[0]), int(r.shape[2]), int(r.shape[3])) != (B, h, w):
                want = [B, ch, h, w]
                raise RuntimeError(f"{what}: {name} must be {[1] + want if batched else want} like net, got {list(x.shape)}")
            xs.append(r)
            total += ch
        if total != self.c_in:
            raise RuntimeError(f"{what}: net and the inputs have {total} channels in all, the module was built for "
                               f"{self.c_in}")
        return rows, xs, batched, tensors

    def _placed(self, what, tensors):
        _no_grad(what, tensors)
        check_tensors(what, tensors, types=False, contiguous=False, on=(self.packed, "the packed weights"))

    @staticmethod
    def _table(segs):
        k = len(segs)
        return ((ctypes.c_void_p * k)(*[t.data_ptr() for t in segs]), (ctypes.c_int64 * k)(*[int(t.stride(0)) for t in segs]),
                (ctypes.c_int * k)(*[int(t.shape[1]) for t in segs]), k)

    def _out(self, what, out, rows, batched, inputs):
        """rows of `out` (checked; it may be net itself, any other overlap with an input is refused)."""
        B, _, h, w = (int(v) for v in rows.shape)
        orows, obatched = _planes(what, out, "out", HIDDEN)
        if tuple(orows.shape) != (B, HIDDEN, h, w) or obatched != batched:
            want = [B, HIDDEN, h, w]
            raise RuntimeError(f"{what}: out must be {[1] + want if batched else want}, got {list(out.shape)}")
        same = orows.data_ptr() == rows.data_ptr() and (B <= 1 or orows.stride(0) == rows.stride(0))
        if not same and _overlap(rows, orows):
            raise RuntimeError(f"{what}: out must be net itself or must not overlap net in memory")
        for k, x in enumerate(inputs):
            if _overlap(x, orows):
                raise RuntimeError(f"{what}: out must not overlap inputs[{k}] in memory")
        return orows

    # ----------------------------------------------------------------------------------------------------- the calls
    def __call__(self, net, *inputs, out=None):
        """net [B,128,h,w] or [1,B,128,h,w] half and 1 to 4 inputs of the same form (contiguous or channel slices of
        contiguous tensors) whose channels add up to the module's.  Returns the new hidden state, contiguous, of net's
        form -- or `out`, which may be net itself (in place) or a half tensor of net's shape that shares no memory with
        any input."""
        what = "conv_gru"
        rows, xs, batched, tensors = self._inputs(what, net, inputs, [(out, "out", F16)] if out is not None else [])
        B, _, h, w = (int(v) for v in rows.shape)
        orows = self._out(what, out, rows, batched, xs) if out is not None else None
        self._placed(what, tensors)
        lib = _lib.load()
        if orows is None:
            res = torch.empty((B, HIDDEN, h, w), dtype=F16, device=net.device)
            orows = res
        if B > 0:
            ws = _ws.get_bytes(_ws_key(net.device), lib.droid_gru_workspace_bytes(B, h, w), net.device)
            _lib.check(lib.droid_conv_gru(*self._table([rows] + xs), self.packed.data_ptr(), orows.data_ptr(),
                                          int(orows.stride(0)), B, h, w, ws.data_ptr(), ws.numel(), _stream()), what)
        if out is not None:
            return out
        return res[None] if batched else res

    def context(self, net):
        """g [B,3,128] fp32: per image and gate (z, r, q) the context term plus both biases of the gate."""
        what = "conv_gru.context"
        check_tensors(what, [(net, "net", F16)], placement=False)
        rows, _ = _planes(what, net, "net", HIDDEN)
        _no_grad(what, [(net, "net", F16)])
        check_tensors(what, [(net, "net", F16)], types=False, contiguous=False, on=(self.packed, "the packed weights"))
        B, _, h, w = (int(v) for v in rows.shape)
        lib = _lib.load()
        g = torch.empty((B, 3, HIDDEN), dtype=F32, device=net.device)
        if B > 0:
            ws = _ws.get_bytes(_ws_key(net.device), lib.droid_gru_workspace_bytes(B, h, w), net.device)
            _lib.check(lib.droid_gru_context(rows.data_ptr(), int(rows.stride(0)), self.packed.data_ptr(), self.c_in, B, h, w,
                                             g.data_ptr(), ws.data_ptr(), ws.numel(), _stream()), what)
        return g

    @staticmethod
    def _g(what, g, B):
        if tuple(g.shape) != (B, 3, HIDDEN) or not g.is_contiguous():
            raise RuntimeError(f"{what}: g must be a contiguous [{B}, 3, {HIDDEN}], got {list(g.shape)}")

    def gates(self, g, net, *inputs):
        """(z16, rnet16), two contiguous half [B,128,h,w] (or [1,B,128,h,w]), from g = context(net)."""
        what = "conv_gru.gates"
        rows, xs, batched, tensors = self._inputs(what, net, inputs, [(g, "g", F32)])
        B, _, h, w = (int(v) for v in rows.shape)
        self._g(what, g, B)
        self._placed(what, tensors)
        lib = _lib.load()
        z, rnet = (torch.empty((B, HIDDEN, h, w), dtype=F16, device=net.device) for _ in range(2))
        if B > 0:
            _lib.check(lib.droid_gru_gates(*self._table([rows] + xs), self.packed.data_ptr(), g.data_ptr(), z.data_ptr(),
                                           rnet.data_ptr(), B, h, w, _stream()), what)
        return (z[None], rnet[None]) if batched else (z, rnet)

    def update(self, g, z, rnet, net, *inputs, out=None):
        """The new hidden state from g, z16 and rnet16 (contiguous, as `gates` returns them); out as in a call."""
        what = "conv_gru.update"
        extra = [(g, "g", F32), (z, "z", F16), (rnet, "rnet", F16)] + ([(out, "out", F16)] if out is not None else [])
        rows, xs, batched, tensors = self._inputs(what, net, inputs, extra)
        B, _, h, w = (int(v) for v in rows.shape)
        self._g(what, g, B)
        zr = []
        for t, name in ((z, "z"), (rnet, "rnet")):
            r, bt = _planes(what, t, name, HIDDEN)
            if tuple(r.shape) != (B, HIDDEN, h, w) or bt != batched or not r.is_contiguous():
                raise RuntimeError(f"{what}: {name} must be contiguous and of net's shape, got {list(t.shape)}")
            zr.append(r)
        orows = self._out(what, out, rows, batched, xs + zr) if out is not None else None
        self._placed(what, tensors)
        lib = _lib.load()
        if orows is None:
            res = torch.empty((B, HIDDEN, h, w), dtype=F16, device=net.device)
            orows = res
        if B > 0:
            _lib.check(lib.droid_gru_update(*self._table([zr[1]] + xs), self.packed.data_ptr(), g.data_ptr(), zr[0].data_ptr(),
                                            rows.data_ptr(), int(rows.stride(0)), orows.data_ptr(), int(orows.stride(0)),
                                            B, h, w, _stream()), what)
        if out is not None:
            return out
        return res[None] if batched else res
