"""The output heads of the update operator on the device: the last layer of `delta`, of `weight` and of `GraphAgg.eta`.

`UpdateModule.forward` ends with `delta = self.delta(net)`, `weight = self.weight(net)` and their
`.view(...).permute(0,1,3,4,2)[..., :2].contiguous()` (droid_slam/droid_net.py:95-106, :130-134); `GraphAgg.forward` ends
with `eta = self.eta(net)` and `.01 *` (:51-54, :72-75).  The last layer of each is a Conv2d(128, 2 or 1, 3, padding=1)
followed by the gradient clip (the identity in forward) and, for `weight`, a Sigmoid, for `eta`, a Softplus.
`UpdateHeads` computes these layers (droid_update_heads, include/droid_heads_hip.h): one launch for delta + weight, one
for eta, the activation on the fp32 sum, one rounding to half, and the result in the layout `ba_inputs` reads.  A caller
keeps `delta[0:2]`, `weight[0:2]` and `agg.conv2` + ReLU and hands their results over.

    heads = UpdateHeads(update.delta[2].weight, update.delta[2].bias, update.weight[2].weight, update.weight[2].bias,
                        update.agg.eta[0].weight, update.agg.eta[0].bias)      # once per network
    delta, weight = heads(hd, hw)       # hd, hw [E,128,h,w] (or [1,E,128,h,w]) half -> two [1,E,h,w,2] half
    eta = heads.eta(net)                # net [G,128,h,w] (or [1,G,128,h,w]) half -> [1,G,h,w] half
"""
from __future__ import annotations

import ctypes

import torch

from . import _lib
from ._args import _stream, check_tensors

C, KS = 128, 3
IDENTITY, SIGMOID, SOFTPLUS_CENTI = 0, 1, 2    # DROID_HEAD_* of the header
F16, F16_OR_F32 = torch.float16, (torch.float16, torch.float32)


def pack(weight, bias):
    """The packed parameters of one head (include/droid_heads_hip.h): float32 [128][3][3][n] of float(half(weight)),
    then float(half(bias)) [n], then zeros up to a multiple of 16 bytes."""
    n = int(weight.shape[0])
    w = weight.detach().to(torch.float16).to(torch.float32).permute(1, 2, 3, 0).reshape(-1)
    b = bias.detach().to(torch.float16).to(torch.float32).reshape(-1)
    pad = (-(w.numel() + b.numel())) % 4
    return torch.cat([w, b, torch.zeros(pad, dtype=torch.float32, device=w.device)]).contiguous()


def _no_grad(what, tensors):
    for x, name, _ in tensors:
        if x.requires_grad:
            raise RuntimeError(f"{what}: {name} requires grad, but the operator has no autograd: it is for "
                               "inference, training keeps the stock layers")


def _params(what, weight, bias, n, names):
    tensors = [(weight, names[0], F16_OR_F32), (bias, names[1], F16_OR_F32)]
    check_tensors(what, tensors, placement=False)
    if tuple(weight.shape) != (n, C, KS, KS):
        raise RuntimeError(f"{what}: {names[0]} must be [{n},{C},{KS},{KS}], got {list(weight.shape)}")
    if tuple(bias.shape) != (n,):
        raise RuntimeError(f"{what}: {names[1]} must be [{n}], got {list(bias.shape)}")
    return tensors


class UpdateHeads:
    """The last layers of `delta`, `weight` and (optionally) `GraphAgg.eta`.  The parameters are the layers' own
    ([2,128,3,3] / [2], eta: [1,128,3,3] / [1]; fp32 or half, on the device); they are rounded to half (autocast's cast)
    and packed once.  Rebuild the object after the weights change."""

    def __init__(self, delta_weight, delta_bias, weight_weight, weight_bias, eta_weight=None, eta_bias=None):
        what = "UpdateHeads"
        tensors = (_params(what, delta_weight, delta_bias, 2, ("delta_weight", "delta_bias"))
                   + _params(what, weight_weight, weight_bias, 2, ("weight_weight", "weight_bias")))
        if (eta_weight is None) != (eta_bias is None):
            raise RuntimeError(f"{what}: eta_weight and eta_bias go together")
        if eta_weight is not None:
            tensors += _params(what, eta_weight, eta_bias, 1, ("eta_weight", "eta_bias"))
        check_tensors(what, tensors, types=False, contiguous=False, on=(delta_weight, "delta_weight"))
        lib = _lib.load()
        self.packed_delta = pack(delta_weight, delta_bias)
        self.packed_weight = pack(weight_weight, weight_bias)
        self.packed_eta = pack(eta_weight, eta_bias) if eta_weight is not None else None
        assert self.packed_delta.numel() * 4 == lib.droid_head_packed_bytes(2)
        assert self.packed_eta is None or self.packed_eta.numel() * 4 == lib.droid_head_packed_bytes(1)

    @staticmethod
    def _hidden(what, tensors):
        """The checks of the hidden tensors of a call, in the package's order; returns them as [B,128,h,w]."""
        check_tensors(what, tensors, placement=False)
        rows = [x[0] if x.dim() == 5 and x.shape[0] == 1 else x for x, _, _ in tensors]
        for x, (_, name, _) in zip(rows, tensors):
            if x.dim() != 4 or x.shape[1] != C or x.shape[2] < 1 or x.shape[3] < 1:
                raise RuntimeError(f"{what}: {name} must be [B,{C},h,w] or [1,B,{C},h,w], got {list(x.shape)}")
            if tuple(x.shape) != tuple(rows[0].shape):
                raise RuntimeError(f"{what}: {name} must have the shape of {tensors[0][1]}, {list(rows[0].shape)}, "
                                   f"got {list(x.shape)}")
        _no_grad(what, tensors)
        return rows

    @staticmethod
    def _run(what, xs, packed, n_out, act):
        lib = _lib.load()
        k = len(xs)
        B, _, H, W = (int(v) for v in xs[0].shape)
        outs = [torch.empty((B, H, W, n), dtype=F16, device=xs[0].device) for n in n_out]
        ptrs = lambda ts: (ctypes.c_void_p * k)(*[t.data_ptr() for t in ts])
        ints = lambda vs: (ctypes.c_int * k)(*vs)
        _lib.check(lib.droid_update_heads(ptrs(xs), ptrs(packed), ptrs(outs), ints(n_out), ints(act), k, B, H, W, C,
                                          _stream()), what)
        return outs

    def __call__(self, hd, hw):
        """hd = delta[0:2](net), hw = weight[0:2](net): [E,128,h,w] or [1,E,128,h,w] half, contiguous.  Returns
        (delta, weight), both [1,E,h,w,2] half, as `UpdateModule.forward` returns them; one launch."""
        what = "update_heads"
        tensors = [(hd, "hd", F16), (hw, "hw", F16)]
        hd, hw = self._hidden(what, tensors)
        check_tensors(what, tensors, types=False, on=(self.packed_delta, "the packed weights"))
        delta, weight = self._run(what, [hd, hw], [self.packed_delta, self.packed_weight], [2, 2], [IDENTITY, SIGMOID])
        return delta[None], weight[None]

    def eta(self, net):
        """net = relu(agg.conv2(...)) of `GraphAgg.forward`: [G,128,h,w] or [1,G,128,h,w] half, contiguous.  Returns
        eta [1,G,h,w] half = .01 * softplus(conv), as `GraphAgg.forward` returns it; one launch."""
        what = "update_heads.eta"
        tensors = [(net, "net", F16)]
        net, = self._hidden(what, tensors)
        if self.packed_eta is None:
            raise RuntimeError(f"{what}: this UpdateHeads was built without eta_weight / eta_bias")
        check_tensors(what, tensors, types=False, on=(self.packed_eta, "the packed weights"))
        eta, = self._run(what, [net], [self.packed_eta], [1], [SOFTPLUS_CENTI])
        return eta.view(1, eta.shape[0], eta.shape[1], eta.shape[2])
