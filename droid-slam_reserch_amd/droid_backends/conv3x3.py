"""The 3 x 3 convolutions of the update operator on the f16 matrix cores.

Between its fused ends (`CorrEncoder`, `FlowEncoder`, `UpdateHeads`) the update module holds one layer shape six times, a
Conv2d(128, N, 3, padding=1) and a ReLU on half planes under autocast (droid_slam/droid_net.py:83-109):
`corr_encoder[2:4]`, `flow_encoder[2:4]`, `delta[0:2]`, `weight[0:2]`, `agg.conv1` and `agg.conv2`.  `Conv3x3` computes
such a layer (droid_conv3x3, include/droid_conv3x3_hip.h): fp32 accumulation, the bias, one rounding to half, the ReLU.

    conv = Conv3x3(weight, bias, relu=True)                 # one layer, packed once per network
    pair = Conv3x3([(wd, bd), (ww, bw)], relu=True)         # layers that read one input: one launch, one output each
    y = conv(x)                          # x [B,C_in,h,w] or [1,B,C_in,h,w] half -> [B,C_out,h,w] / [1,B,C_out,h,w]
    hd, hw = pair(net)                   # two contiguous [E,128,h,w]: what UpdateHeads takes
    conv(x, out=buf[:, 256:384])         # into a channel slice of a wider half tensor; x may be such a slice too
"""
from __future__ import annotations

import torch

from . import _lib
from ._args import _stream, check_tensors

KS, SLAB = 3, 32
F16, F16_OR_F32 = torch.float16, (torch.float16, torch.float32)


def supported(c_in, c_out):
    """The layer sizes of the contract: C_in a multiple of 32 in [32, 512], C_out a multiple of 64 in [64, 256]."""
    return 32 <= c_in <= 512 and c_in % 32 == 0 and 64 <= c_out <= 256 and c_out % 64 == 0


def pack(weight, bias):
    """The packed parameters of a layer (include/droid_conv3x3_hip.h): halves [C_in / 32][9][C_out / 16][64][8] with
    element (s, t, nt, lane, j) = w16[16 nt + (lane & 15)][32 s + 8 (lane >> 4) + j][t / 3][t % 3], then b16 [C_out]."""
    n, c = int(weight.shape[0]), int(weight.shape[1])
    w16 = weight.detach().to(F16).reshape(n // 16, 16, c // SLAB, 4, 8, KS * KS)     # (nt, c16, s, g, j, t)
    w16 = w16.permute(2, 5, 0, 3, 1, 4).reshape(-1)                                  # (s, t, nt, g, c16, j)
    return torch.cat([w16, bias.detach().to(F16).reshape(-1)]).contiguous()


def _no_grad(what, tensors):
    for x, name, _ in tensors:
        if x.requires_grad:
            raise RuntimeError(f"{what}: {name} requires grad, but the operator has no autograd: it is for "
                               "inference, training keeps the stock layers")


def _planes(what, t, name, channels):
    """t as [B,channels,h,w] rows with strides (anything >= channels * h * w, h * w, w, 1); returns (rows, batched)."""
    batched = t.dim() == 5 and t.shape[0] == 1
    rows = t[0] if batched else t
    if rows.dim() != 4 or rows.shape[1] != channels or rows.shape[2] < 1 or rows.shape[3] < 1:
        raise RuntimeError(f"{what}: {name} must be [B,{channels},h,w] or [1,B,{channels},h,w], got {list(t.shape)}")
    B, _, h, w = (int(v) for v in rows.shape)
    sb, sc, sv, su = (int(v) for v in rows.stride())
    if (w > 1 and su != 1) or (h > 1 and sv != w) or sc != h * w or (B > 1 and sb < channels * h * w):
        raise RuntimeError(f"{what}: {name} must have the strides (at least {channels * h * w}, {h * w}, {w}, 1) of a "
                           f"channel slice of a contiguous tensor, got {tuple(rows.stride())}")
    return rows, batched


def _span(t):
    """(first byte, batch stride in bytes, bytes of a batch entry, B) of rows as `_planes` returns them."""
    B, C, h, w = (int(v) for v in t.shape)
    return t.data_ptr(), int(t.stride(0)) * 2, C * h * w * 2, B


def _overlap(x, y):
    """Whether the halves of two `_planes` tensors share memory.  Exact where the batch strides are equal (two channel
    slices of one buffer interleave without touching); otherwise the enclosing byte ranges decide."""
    (px, sx, nx, bx), (py, sy, ny, by) = _span(x), _span(y)
    if bx == 0 or by == 0:
        return False
    ex, ey = px + (bx - 1) * sx + nx, py + (by - 1) * sy + ny
    if ex <= py or ey <= px:
        return False
    if sx != sy or bx == 1 or by == 1 or nx + ny > sx:
        return True
    d = (py - px) % sx      # where y's entries begin inside x's period
    return not (nx <= d and d + ny <= sx)


class Conv3x3:
    """One Conv2d(C_in, C_out, 3, padding=1) with or without its ReLU, or several such layers that read one input.
    weight [C_out,C_in,3,3] and bias [C_out] are the layer's parameters as they are (fp32 or half, on the device); they
    are rounded to half (autocast's cast) and packed once.  With a list of (weight, bias) the layers share C_in and have
    equal C_out; one launch computes them all and a call returns one contiguous tensor per layer.  Rebuild the object
    after the weights change."""

    def __init__(self, weight, bias=None, relu=True):
        what = "Conv3x3"
        layers = list(weight) if isinstance(weight, (list, tuple)) else [(weight, bias)]
        if isinstance(weight, (list, tuple)) and bias is not None:
            raise RuntimeError(f"{what}: with a list of (weight, bias) layers, bias must be None")
        if not layers or any(not isinstance(l, (list, tuple)) or len(l) != 2 for l in layers):
            raise RuntimeError(f"{what}: weight must be a tensor or a non-empty list of (weight, bias)")
        multi = isinstance(weight, (list, tuple))
        names = [(f"weight[{k}]", f"bias[{k}]") if multi else ("weight", "bias") for k in range(len(layers))]
        tensors = [(t, nm, F16_OR_F32) for l, pair in zip(layers, names) for t, nm in zip(l, pair)]
        check_tensors(what, tensors, placement=False)
        w0 = layers[0][0]
        for (w, b), (wn, bn) in zip(layers, names):
            if w.dim() != 4 or tuple(w.shape[2:]) != (KS, KS) or not supported(int(w.shape[1]), int(w.shape[0])):
                raise RuntimeError(f"{what}: {wn} must be [C_out,C_in,{KS},{KS}] with C_in a multiple of 32 in 32 .. 512 "
                                   f"and C_out a multiple of 64 in 64 .. 256, got {list(w.shape)}")
            if tuple(w.shape) != tuple(w0.shape):
                raise RuntimeError(f"{what}: {wn} must have the shape of {names[0][0]}, {list(w0.shape)}, got {list(w.shape)}")
            if tuple(b.shape) != (int(w.shape[0]),):
                raise RuntimeError(f"{what}: {bn} must be [{int(w.shape[0])}], got {list(b.shape)}")
        self.c_in, self.group_channels = int(w0.shape[1]), int(w0.shape[0])
        self.groups = len(layers)
        self.c_out = self.groups * self.group_channels
        if not supported(self.c_in, self.c_out):
            raise RuntimeError(f"{what}: the layers stack to C_out = {self.c_out}, above 256")
        check_tensors(what, tensors, types=False, contiguous=False, on=(w0, names[0][0]))
        self.relu = bool(relu)
        lib = _lib.load()
        self.packed = pack(torch.cat([w.detach().to(F16) for w, _ in layers]),
                           torch.cat([b.detach().to(F16) for _, b in layers]))
        assert self.packed.numel() * 2 == lib.droid_conv3x3_packed_bytes(self.c_in, self.c_out)

    def __call__(self, x, out=None):
        """x [B,C_in,h,w] or [1,B,C_in,h,w] half, contiguous or a channel slice of a contiguous tensor.  Returns
        [B,C_out,h,w] (or [1,B,C_out,h,w] for a batched x), contiguous -- for several layers a tuple of them -- or `out`,
        a half tensor of that shape (possibly a channel slice) which must not share memory with x."""
        what = "conv3x3"
        tensors = [(x, "x", F16)] + ([(out, "out", F16)] if out is not None else [])
        check_tensors(what, tensors, placement=False)
        rows, batched = _planes(what, x, "x", self.c_in)
        B, _, h, w = (int(v) for v in rows.shape)
        orows = None
        if out is not None:
            if self.groups != 1:
                raise RuntimeError(f"{what}: out is for a single layer, this Conv3x3 holds {self.groups} and returns "
                                   f"one tensor per layer")
            orows, obatched = _planes(what, out, "out", self.c_out)
            if tuple(orows.shape) != (B, self.c_out, h, w) or obatched != batched:
                want = [B, self.c_out, h, w]
                raise RuntimeError(f"{what}: out must be {[1] + want if batched else want}, got {list(out.shape)}")
        _no_grad(what, tensors)
        check_tensors(what, tensors, types=False, contiguous=False, on=(self.packed, "the packed weights"))
        if orows is not None and _overlap(rows, orows):
            raise RuntimeError(f"{what}: out must not overlap x in memory")
        lib = _lib.load()
        if orows is None:
            ys = torch.empty((self.groups, B, self.group_channels, h, w), dtype=F16, device=x.device)
            yptr, ybs, ygs = ys.data_ptr(), self.group_channels * h * w, B * self.group_channels * h * w
        else:
            yptr, ybs, ygs = orows.data_ptr(), int(orows.stride(0)), 0
        _lib.check(lib.droid_conv3x3(rows.data_ptr(), self.packed.data_ptr(), yptr, B, self.c_in, self.c_out, h, w,
                                     int(rows.stride(0)), ybs, ygs, self.group_channels, int(self.relu), _stream()), what)
        if orows is not None:
            return out
        res = tuple(y[None] if batched else y for y in ys.unbind(0))
        return res[0] if self.groups == 1 else res
