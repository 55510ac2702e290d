"""`ba_inputs`: the tail of `FactorGraph.update` between the update operator and `cuda_ba` on the device
(include/droid_update_hip.h, csrc/ba_inputs.hip).  Host side only: checks, output tensors, one call into the C ABI."""
from __future__ import annotations

import torch

from . import _lib
from ._args import ScratchCache, _ptr, _stream, _ws_key, check_tensors

F32, I64, F16_OR_F32 = torch.float32, torch.int64, (torch.float16, torch.float32)
_DT = {torch.float16: _lib.DROID_F16, torch.float32: _lib.DROID_F32}
_bi_ws = ScratchCache()   # _ws_key(device) -> grow-only uint8 scratch of ba_inputs

_FLAG_TEXT = {1: "an emitted edge index lies outside the damping buffer [0, nbuf)",
              2: "damping has another number of rows than the active edges have distinct sources"}


class BaInputs:
    """What `ba_inputs` returns.  target_state, weight_state [1, E, h, w, 2]: the graph's new `target` / `weight`;
    ii, jj [Eb], target, weight [Eb, 2, h, w], eta [M, h, w]: the arguments of `cuda_ba`; frames [G]: unique(ii) of the
    active edges, what `upsample` takes; t0, t1: ints.  With sync=False the edge and frame tensors keep their capacity
    (rows beyond the counts are unwritten), t0 and t1 are None and `info` holds the counts on the device:
    {Eb, M, G, t0, t1, flags, K, 0}."""
    __slots__ = ("target_state", "weight_state", "ii", "jj", "target", "weight", "eta", "frames", "frames_eta", "t0",
                 "t1", "info")

    def __init__(self, **kw):
        for k in self.__slots__:
            setattr(self, k, kw[k])


def _rows(x, dims):
    """x without its leading batch dimension of 1, when it has one"""
    return x[0] if x.dim() == dims + 1 and x.shape[0] == 1 else x


def ba_inputs(coords1, delta, weight, damping, damping_buf, ii, jj, inactive=None, t0=None, EP=1e-7, sync=True):
    """factor_graph.py:213-238 in two launches: `target = coords1 + delta.float()`, `weight.float()`,
    `damping_buf[unique(ii)] = damping`, the inactive edges at or after t0 - 3 in front of the active ones, `eta = .2 *
    damping_buf[unique(ii)] + EP`, the [Eb, 2, h, w] planes and t0 / t1 of `cuda_ba`.
    coords1 [1, E, h, w, 2] or [E, h, w, 2] float32; delta, weight the same shape, float16 or float32 (one dtype);
    damping [1, G, h, w] or [G, h, w], float16 or float32, or None; damping_buf [nbuf, h, w] float32, updated in place;
    ii, jj [E] int64; inactive = (ii_inac, jj_inac, target_inac, weight_inac) with [Ei] int64 and [1, Ei, h, w, 2] or
    [Ei, h, w, 2] float32, or None; t0 an int or None (max(1, ii.min() + 1), taken on the device).
    delta=None is emit-only mode (update_lowmem, :292-294): coords1 is the held target, weight float32, nothing is added
    and target_state / weight_state are the two inputs themselves.
    sync=True reads the 8 ints of `info` once, trims the outputs by leading-dimension slices and raises RuntimeError on
    a flag; sync=False reads nothing.  Returns a BaInputs.  Contract: include/droid_update_hip.h.  An addition."""
    what = "ba_inputs"
    lib = _lib.load()
    absorb = delta is not None
    inac = tuple(inactive) if inactive is not None else None
    if inac is not None and len(inac) != 4:
        raise RuntimeError(f"{what}: inactive must be (ii_inac, jj_inac, target_inac, weight_inac)")
    tensors = [(coords1, "coords1", F32)]
    if absorb:
        tensors += [(delta, "delta", F16_OR_F32), (weight, "weight", delta.dtype if isinstance(delta, torch.Tensor) else None)]
    else:
        tensors += [(weight, "weight", F32)]
    if damping is not None:
        tensors += [(damping, "damping", F16_OR_F32)]
    tensors += [(damping_buf, "damping_buf", F32), (ii, "ii", I64), (jj, "jj", I64)]
    if inac is not None:
        tensors += [(inac[0], "ii_inac", I64), (inac[1], "jj_inac", I64), (inac[2], "target_inac", F32),
                    (inac[3], "weight_inac", F32)]
    check_tensors(what, tensors, placement=False)

    a = _rows(coords1, 4)
    if a.dim() != 4 or a.shape[-1] != 2:
        raise RuntimeError(f"{what}: coords1 must be [1, E, h, w, 2] or [E, h, w, 2], got {tuple(coords1.shape)}")
    E, h, w = (int(v) for v in a.shape[:3])
    for x, name in ((delta, "delta"), (weight, "weight")):
        if x is not None and tuple(_rows(x, 4).shape) != (E, h, w, 2):
            raise RuntimeError(f"{what}: {name} must be [{E}, {h}, {w}, 2] like coords1, got {tuple(x.shape)}")
    if tuple(ii.shape) != (E,) or tuple(jj.shape) != (E,):
        raise RuntimeError(f"{what}: ii and jj must be [E] = [{E}], got {tuple(ii.shape)} and {tuple(jj.shape)}")
    if damping_buf.dim() != 3 or tuple(damping_buf.shape[1:]) != (h, w):
        raise RuntimeError(f"{what}: damping_buf must be [nbuf, {h}, {w}], got {tuple(damping_buf.shape)}")
    nbuf = int(damping_buf.shape[0])
    n_damp = 0
    if damping is not None:
        d = _rows(damping, 3)
        if d.dim() != 3 or tuple(d.shape[1:]) != (h, w):
            raise RuntimeError(f"{what}: damping must be [1, G, {h}, {w}] or [G, {h}, {w}], got {tuple(damping.shape)}")
        n_damp = int(d.shape[0])
    Ei = 0
    if inac is not None:
        Ei = int(inac[0].shape[0]) if inac[0].dim() == 1 else -1
        if Ei < 0 or tuple(inac[1].shape) != (Ei,):
            raise RuntimeError(f"{what}: ii_inac and jj_inac must be [Ei], got {tuple(inac[0].shape)} and {tuple(inac[1].shape)}")
        for x, name in ((inac[2], "target_inac"), (inac[3], "weight_inac")):
            if tuple(_rows(x, 4).shape) != (Ei, h, w, 2):
                raise RuntimeError(f"{what}: {name} must be [{Ei}, {h}, {w}, 2], got {tuple(x.shape)}")
    if t0 is not None and int(t0) < 0:
        raise RuntimeError(f"{what}: t0 must not be negative (None: taken from ii on the device)")
    check_tensors(what, tensors, types=False, on=(coords1, "coords1"))

    dev = coords1.device
    cap_e, cap_m = E + Ei, min(nbuf, E + Ei)
    new = lambda shape, dtype: torch.empty(shape, dtype=dtype, device=dev)   # noqa: E731
    target_state = new((1, E, h, w, 2), F32) if absorb else None
    weight_state = new((1, E, h, w, 2), F32) if absorb else None
    ii_ba, jj_ba = new((cap_e,), I64), new((cap_e,), I64)
    target_ba, weight_ba = new((cap_e, 2, h, w), F32), new((cap_e, 2, h, w), F32)
    eta, frames, frames_eta = new((cap_m, h, w), F32), new((cap_m,), I64), new((cap_m,), I64)
    info = new((8,), torch.int32)
    nbytes = lib.droid_ba_inputs_workspace_bytes(E, Ei, nbuf)   # 0 for sizes the call below refuses by name
    ws = _bi_ws.get_bytes(_ws_key(dev), nbytes, dev)
    use_inac = Ei > 0
    _lib.check(lib.droid_ba_inputs(
        ii.data_ptr(), jj.data_ptr(), coords1.data_ptr(), _ptr(delta), weight.data_ptr(), _ptr(damping),
        damping_buf.data_ptr(), *(_ptr(x) if use_inac else None for x in (inac or (None,) * 4)),
        E, Ei, h, w, nbuf, n_damp, _DT[delta.dtype] if absorb else _lib.DROID_F32,
        _DT[damping.dtype] if damping is not None else _lib.DROID_F32, -1 if t0 is None else int(t0), float(EP),
        _ptr(target_state), _ptr(weight_state), ii_ba.data_ptr(), jj_ba.data_ptr(), target_ba.data_ptr(),
        weight_ba.data_ptr(), cap_e, eta.data_ptr(), frames.data_ptr(), frames_eta.data_ptr(), cap_m, info.data_ptr(),
        ws.data_ptr(), ws.numel(), _stream()), what)
    if not absorb:
        target_state, weight_state = coords1.view(1, E, h, w, 2), weight.view(1, E, h, w, 2)
    out = dict(target_state=target_state, weight_state=weight_state, ii=ii_ba, jj=jj_ba, target=target_ba,
               weight=weight_ba, eta=eta, frames=frames, frames_eta=frames_eta, t0=None, t1=None, info=info)
    if not sync:
        return BaInputs(**out)
    Eb, M, G, t0_dev, t1_dev, flags = (int(v) for v in info.cpu()[:6])   # the one host read
    bad = [txt for bit, txt in _FLAG_TEXT.items() if flags & bit]
    if bad:
        raise RuntimeError(f"{what}: " + "; ".join(bad))
    out.update(ii=ii_ba[:Eb], jj=jj_ba[:Eb], target=target_ba[:Eb], weight=weight_ba[:Eb], eta=eta[:M], frames=frames[:G],
               frames_eta=frames_eta[:M], t0=t0_dev, t1=t1_dev)
    return BaInputs(**out)
