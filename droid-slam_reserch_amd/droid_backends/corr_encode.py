"""The correlation lookup of an update step fused with `corr_encoder[0:2]` of the update module.

`UpdateModule.forward` starts with `corr = self.corr_encoder(corr)` (droid_slam/droid_net.py:83-87, :125): a
Conv2d(196, 128, 1), a ReLU, a Conv2d(128, 128, 3) and a ReLU.  The first two layers only need the 196 lookup values of
one pixel at a time, so `CorrEncoder` computes them inside the lookup (droid_corr_encode, include/droid_update_hip.h)
and the [E, 196, h, w] tensor is never written.  A caller keeps `corr_encoder[2:]` and hands it the result.

    enc = CorrEncoder(update.corr_encoder[0].weight, update.corr_encoder[0].bias)    # once per network
    corr = enc(pyramid, coords)                    # [E,128,h,w] half = relu(conv1x1(corr_pyramid_forward(...)))
    corr = store.encode(coords1, enc)              # the same through a PyramidStore, coords1 as reproject returns it
"""
from __future__ import annotations

import ctypes

import torch

from . import _lib
from ._args import _stream, check_tensors

LEVELS, RADIUS, K, KP, N = 4, 3, 49, 64, 128   # what the kernel is built for; K is padded to KP per level
F32, I64, F16_OR_F32 = torch.float32, torch.int64, (torch.float16, torch.float32)
_DT = {torch.float16: _lib.DROID_F16, torch.float32: _lib.DROID_F32}
_LAYOUT = {"2hw": 0, "hw2": 1}   # DROID_COORDS_2HW, DROID_COORDS_HW2


def packed_halves():
    """Halves in the packed parameter buffer: the weights [4][2][8][64][8], then the bias [128]."""
    return LEVELS * KP * N + N


def pack_index(device=None):
    """int64 [4*64*128]: element i of the packed weights is entry pack_index[i] of the flat [128*196 + 1] table
    (w16.flatten(), 0): the layout of include/droid_update_hip.h, element (l, s, nt, lane, j) =
    w16[16 nt + (lane & 15)][49 l + 32 s + 8 (lane >> 4) + j], zero where the K index within the level is >= 49."""
    l, s, nt, lane, j = torch.meshgrid(torch.arange(LEVELS), torch.arange(2), torch.arange(8), torch.arange(64),
                                       torch.arange(8), indexing="ij")
    n = 16 * nt + (lane & 15)
    kk = 32 * s + 8 * (lane >> 4) + j
    idx = torch.where(kk < K, n * (LEVELS * K) + l * K + kk, torch.full_like(kk, N * LEVELS * K))
    return idx.reshape(-1).to(device)


class CorrEncoder:
    """`corr_encoder[0:2]` fused into the lookup.  weight [128,196,1,1] or [128,196] and bias [128] are the layer's
    parameters as they are (fp32 or half, on the device); they are rounded to half (autocast's cast) and packed once."""

    def __init__(self, weight, bias):
        what = "CorrEncoder"
        check_tensors(what, [(weight, "weight", F16_OR_F32), (bias, "bias", F16_OR_F32)], placement=False)
        if weight.dim() == 4 and tuple(weight.shape[2:]) == (1, 1):
            weight = weight.reshape(weight.shape[0], weight.shape[1])
        if tuple(weight.shape) != (N, LEVELS * K):
            raise RuntimeError(f"{what}: weight must be [{N},{LEVELS * K},1,1] or [{N},{LEVELS * K}], "
                               f"got {list(weight.shape)}")
        if tuple(bias.shape) != (N,):
            raise RuntimeError(f"{what}: bias must be [{N}], got {list(bias.shape)}")
        check_tensors(what, [(weight, "weight", None), (bias, "bias", None)], types=False, contiguous=False,
                      on=(weight, "weight"))
        w16 = weight.detach().to(torch.float16).reshape(-1)
        table = torch.cat([w16, torch.zeros(1, dtype=torch.float16, device=w16.device)])
        self.packed = torch.cat([table[pack_index(w16.device)], bias.detach().to(torch.float16)]).contiguous()
        assert self.packed.numel() * 2 == _lib.load().droid_corr_encode_packed_bytes()

    def __call__(self, pyramid, coords, slots=None, layout="2hw"):
        """pyramid: the levels [B,h,w,h>>l,w>>l] (with `slots` [E] int64: capacity buffers [cap,...]), half or fp32;
        coords fp32, [E,2,h,w] (layout "2hw") or [E,h,w,2] ("hw2").  Returns [E,128,h,w] half."""
        what = "corr_encode"
        lib = _lib.load()
        levels = list(pyramid)
        if layout not in _LAYOUT:
            raise ValueError(f'{what}: layout must be "2hw" or "hw2", got {layout!r}')
        tensors = [(p, f"pyramid[{i}]", F16_OR_F32) for i, p in enumerate(levels)] + [(coords, "coords", F32)] \
            + ([(slots, "slots", I64)] if slots is not None else [])
        check_tensors(what, tensors, placement=False)
        if len(levels) != LEVELS:
            raise RuntimeError(f"{what}: the pyramid must have {LEVELS} levels, got {len(levels)}")
        if any(p.dtype != levels[0].dtype for p in levels):
            raise RuntimeError(f"{what}: pyramid levels must share one dtype")
        if levels[0].dim() != 5:
            raise RuntimeError(f"{what}: pyramid[0] must be [B,h,w,h,w], got {list(levels[0].shape)}")
        cap, H1, W1 = (int(x) for x in levels[0].shape[:3])
        for l, p in enumerate(levels):
            if tuple(p.shape) != (cap, H1, W1, H1 >> l, W1 >> l):
                raise RuntimeError(f"{what}: pyramid[{l}] must be [{cap},{H1},{W1},{H1 >> l},{W1 >> l}], "
                                   f"got {list(p.shape)}")
        B = cap
        if slots is not None:
            if slots.dim() != 1:
                raise RuntimeError(f"{what}: slots must be [E], got {list(slots.shape)}")
            B = int(slots.shape[0])
        want = (B, 2, H1, W1) if layout == "2hw" else (B, H1, W1, 2)
        if tuple(coords.shape) != want:
            raise RuntimeError(f"{what}: coords must be {list(want)} for layout {layout!r}, got {list(coords.shape)}")
        for x, name, _ in tensors:
            if x.requires_grad:
                raise RuntimeError(f"{what}: {name} requires grad, but the operator has no autograd: it is for "
                                   "inference, training keeps the unfused layers")
        check_tensors(what, tensors, types=False, on=(self.packed, "the packed weights"))
        out = torch.empty((B, N, H1, W1), dtype=torch.float16, device=coords.device)
        ptrs = (ctypes.c_void_p * LEVELS)(*[p.data_ptr() for p in levels])
        _lib.check(lib.droid_corr_encode(ptrs, None if slots is None else slots.data_ptr(), coords.data_ptr(),
                                         self.packed.data_ptr(), out.data_ptr(), B, cap, H1, W1, RADIUS, LEVELS, N,
                                         _DT[levels[0].dtype], _LAYOUT[layout], _stream()), what)
        return out
