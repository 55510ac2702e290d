"""What every operator does with its arguments on the way to the C ABI: the current stream, the tensor checks in one
fixed order, and the grow-only scratch buffers.  Private to the package."""
from __future__ import annotations

import torch


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _ptr(t):
    return None if t is None else t.data_ptr()


def _ws_key(device):
    """(device index, stream handle) of the current stream on `device`; `cuda` without an index is the current device."""
    idx = device.index if device.index is not None else torch.cuda.current_device()
    return (idx, torch.cuda.current_stream(idx).cuda_stream)


def _dtype_text(dtype):
    if isinstance(dtype, tuple):
        return " or ".join(_dtype_text(d) for d in dtype)
    return "int64 (torch.long)" if dtype == torch.int64 else str(dtype).replace("torch.", "")


def check_tensors(what, tensors, types=True, placement=True, contiguous=True, on=None):
    """The checks of `tensors` = [(tensor, name, dtype)], dtype one torch dtype, a tuple of them or None (any), in one
    order for every operator `what`: is a tensor, dtype (`types`), then contiguous, on a HIP device, on one device
    (`placement`) -- a caller's mistake is named before the device is looked at.  An operator with shape checks of its own
    calls the two halves around them.  `on` = (tensor, text) names the device every tensor has to share."""
    if types:
        for x, name, dtype in tensors:
            if not isinstance(x, torch.Tensor):
                raise TypeError(f"{what}: {name} must be a tensor, got {type(x).__name__}")
            if dtype is not None and x.dtype != dtype and not (isinstance(dtype, tuple) and x.dtype in dtype):
                raise RuntimeError(f"{what}: {name} must be {_dtype_text(dtype)}, got {x.dtype}")
    if not placement:
        return
    if contiguous:
        for x, name, _ in tensors:
            if not x.is_contiguous():
                raise RuntimeError(f"{what}: {name} must be contiguous")
    for x, name, _ in tensors:
        if not x.is_cuda:
            raise RuntimeError(f"{what}: {name} must be a HIP (cuda) tensor: droid_backends has no CPU path")
        if on is not None and x.device != on[0].device:
            raise RuntimeError(f"{what}: {name} is on {x.device}, {on[1]} on {on[0].device}")


class ScratchCache(dict):
    """Grow-only uint8 scratch buffers of one operator, one per key (`_ws_key`: device and stream)."""

    def get_bytes(self, key, nbytes, device):
        ws = self.get(key)
        if ws is None or ws.numel() < nbytes:
            ws = self[key] = torch.empty(max(int(nbytes * 1.25), 4096), dtype=torch.uint8, device=device)
        return ws
