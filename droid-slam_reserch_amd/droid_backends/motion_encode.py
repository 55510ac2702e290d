"""Reproject + motion features of an update step fused with `flow_encoder[0:2]` of the update module.

Every `FactorGraph.update` reprojects its edges, builds the four motion planes (droid_slam/factor_graph.py:203-205) and
`UpdateModule.forward` runs `flow = self.flow_encoder(flow)` on them (droid_slam/droid_net.py:89-93, :126): a
Conv2d(4, 128, 7, padding=3), a ReLU, a Conv2d(128, 64, 3) and a ReLU.  `FlowEncoder` computes the first two layers inside
the reprojection (droid_motion_encode, include/droid_motion_encode_hip.h): the [E, 4, h, w] planes are never written and
the vendor convolution never sees a four-channel 7 x 7 layer.  A caller keeps `flow_encoder[2:]` and hands it the result.

    enc = FlowEncoder(update.flow_encoder[0].weight, update.flow_encoder[0].bias)    # once per network
    flow, coords1, mask = enc(poses, disps, intrinsics, ii, jj, target)   # [E,128,h,w] half, [1,E,h,w,2], [1,E,h,w,1]
    flow = enc.conv(motn)                                                 # the same layers on given planes [E,4,h,w]
"""
from __future__ import annotations

import torch

from . import _lib
from ._args import _stream, check_tensors
from .corr_encode import K, LEVELS, N, pack_index

CHANNELS, KSIZE = LEVELS, 7     # the four motion channels stand where the four pyramid levels stand; K = 7 * 7 taps
F32, I64, F16_OR_F32 = torch.float32, torch.int64, (torch.float16, torch.float32)


def _no_grad(what, tensors):
    for x, name, _ in tensors:
        if x.requires_grad:
            raise RuntimeError(f"{what}: {name} requires grad, but the operator has no autograd: it is for "
                               "inference, training keeps the unfused layers")


class FlowEncoder:
    """`flow_encoder[0:2]` fused into reproject + motion features.  weight [128,4,7,7] and bias [128] are the layer's
    parameters as they are (fp32 or half, on the device); they are rounded to half (autocast's cast) and packed once, by
    the packer of `CorrEncoder`: weight.reshape(128, 196) has k = 49 c + 7 ky + kx."""

    def __init__(self, weight, bias):
        what = "FlowEncoder"
        check_tensors(what, [(weight, "weight", F16_OR_F32), (bias, "bias", F16_OR_F32)], placement=False)
        if tuple(weight.shape) != (N, CHANNELS, KSIZE, KSIZE):
            raise RuntimeError(f"{what}: weight must be [{N},{CHANNELS},{KSIZE},{KSIZE}], got {list(weight.shape)}")
        if tuple(bias.shape) != (N,):
            raise RuntimeError(f"{what}: bias must be [{N}], got {list(bias.shape)}")
        check_tensors(what, [(weight, "weight", None), (bias, "bias", None)], types=False, contiguous=False,
                      on=(weight, "weight"))
        w16 = weight.detach().to(torch.float16).reshape(-1)
        table = torch.cat([w16, torch.zeros(1, dtype=torch.float16, device=w16.device)])
        self.packed = torch.cat([table[pack_index(w16.device)], bias.detach().to(torch.float16)]).contiguous()
        assert self.packed.numel() * 2 == _lib.load().droid_motion_encode_packed_bytes()

    def __call__(self, poses, disps, intrinsics, ii, jj, target):
        """The arguments of `droid_backends.reproject` with a target: poses [nbuf,7], disps [nbuf,h,w] (or the batched
        [1,nbuf,...] state), intrinsics [nbuf,4] or [4], ii, jj [E] int64, target [1,E,h,w,2] or [E,h,w,2].  Returns
        (flow [E,128,h,w] half, coords1 [1,E,h,w,2], mask [1,E,h,w,1]): coords1 and mask are `reproject`'s bits."""
        what = "motion_encode"
        lib = _lib.load()
        tensors = [(poses, "poses", F32), (disps, "disps", F32), (intrinsics, "intrinsics", F32), (ii, "ii", I64),
                   (jj, "jj", I64), (target, "target", F32)]
        check_tensors(what, tensors, placement=False)
        if poses.dim() == 3 and disps.dim() == 4 and poses.shape[0] == 1 and disps.shape[0] == 1:
            poses, disps = poses[0], disps[0]      # the batched [1,nbuf,...] tensors the caller holds
            if intrinsics.dim() == 3 and intrinsics.shape[0] == 1:
                intrinsics = intrinsics[0]
        if poses.dim() != 2 or poses.shape[1] != 7:
            raise RuntimeError(f"{what}: poses must be [nbuf,7] or [1,nbuf,7], got {list(poses.shape)}")
        if disps.dim() != 3:
            raise RuntimeError(f"{what}: disps must be [nbuf,h,w] or [1,nbuf,h,w], got {list(disps.shape)}")
        nbuf, H, W = (int(x) for x in disps.shape)
        nbuf = min(nbuf, int(poses.shape[0]))
        if tuple(intrinsics.shape) != (4,) and not (intrinsics.dim() == 2 and intrinsics.shape[1] == 4
                                                    and int(intrinsics.shape[0]) >= nbuf):
            raise RuntimeError(f"{what}: intrinsics must be [4] or [nbuf,4] with a row per frame, "
                               f"got {list(intrinsics.shape)}")
        if ii.dim() != 1 or tuple(jj.shape) != tuple(ii.shape):
            raise RuntimeError(f"{what}: ii and jj must be [E], got {list(ii.shape)} and {list(jj.shape)}")
        E = int(ii.shape[0])
        if tuple(target.shape) not in ((E, H, W, 2), (1, E, H, W, 2)):
            raise RuntimeError(f"{what}: target must be [{E}, {H}, {W}, 2] or [1, {E}, {H}, {W}, 2], "
                               f"got {list(target.shape)}")
        _no_grad(what, tensors)
        tensors = [(poses, "poses", F32), (disps, "disps", F32), (intrinsics, "intrinsics", F32), (ii, "ii", I64),
                   (jj, "jj", I64), (target, "target", F32)]
        check_tensors(what, tensors, types=False, on=(self.packed, "the packed weights"))
        dev = poses.device
        out = torch.empty((E, N, H, W), dtype=torch.float16, device=dev)
        coords = torch.empty((1, E, H, W, 2), dtype=torch.float32, device=dev)
        valid = torch.empty((1, E, H, W, 1), dtype=torch.float32, device=dev)
        _lib.check(lib.droid_motion_encode(poses.data_ptr(), disps.data_ptr(), intrinsics.data_ptr(),
                                           4 if intrinsics.dim() == 2 else 0, ii.data_ptr(), jj.data_ptr(),
                                           target.data_ptr(), None, self.packed.data_ptr(), coords.data_ptr(),
                                           valid.data_ptr(), out.data_ptr(), E, nbuf, H, W, N, _stream()), what)
        return out, coords, valid

    def conv(self, motn):
        """The two layers on given motion planes: motn [E,4,h,w] or [1,E,4,h,w] fp32 (`motion_features`' first result)
        -> [E,128,h,w] half = relu(conv2d(half(motn), w16, b16, padding=3))."""
        what = "motion_encode.conv"
        lib = _lib.load()
        tensors = [(motn, "motn", F32)]
        check_tensors(what, tensors, placement=False)
        if motn.dim() == 5 and motn.shape[0] == 1:
            motn = motn[0]
        if motn.dim() != 4 or motn.shape[1] != CHANNELS or motn.shape[2] < 1 or motn.shape[3] < 1:
            raise RuntimeError(f"{what}: motn must be [E,{CHANNELS},h,w] or [1,E,{CHANNELS},h,w], got {list(motn.shape)}")
        _no_grad(what, tensors)
        check_tensors(what, [(motn, "motn", F32)], types=False, on=(self.packed, "the packed weights"))
        E, _, H, W = (int(x) for x in motn.shape)
        out = torch.empty((E, N, H, W), dtype=torch.float16, device=motn.device)
        _lib.check(lib.droid_motion_encode(None, None, None, 0, None, None, None, motn.data_ptr(), self.packed.data_ptr(),
                                           None, None, out.data_ptr(), E, 1, H, W, N, _stream()), what)
        return out
