#!/usr/bin/env python
"""Times the lookup fused with corr_encoder[0:2] (PyramidStore.encode -> droid_corr_encode) against the stock sequence
on this library's best lookup, with HIP events, per shape and in one process, ALTERNATING the variants:
  stock_a, stock_b    store(coords1) -> F.conv2d under autocast -> relu_      (three launches and the permuted copy
                      of the coordinates; the A/A pair is the noise of this path in this run)
  fused_a, fused_b    store.encode(coords1, enc)                              (one launch; A/A pair)
  stock_noperm        corr_pyramid_forward(pyramid, coords [E,2,h,w], slots=) -> conv2d -> relu_
  fused_2hw           enc(pyramid, coords [E,2,h,w], slots=, layout="2hw")    (the pair without the permuted copy on the
                      stock side: what the coordinate layout alone saves)
Half, C = 128, 4 levels, radius 3, a PyramidStore of 96 slots; 48x64 with E = 1 (motion filter), 24 (frontend window)
and 64, and 30x40 with E = 64.  Acceptance per shape (`within`): median(fused_a) <= median(stock_a) + the A/A spread of
the two paths.  The baseline is the stock sequence of the same run.
Algorithmic bytes per pixel: stock 392 (lookup write) + 392 + 256 (convolution) + 256 + 256 (ReLU) = 1552, fused 256,
both on top of the gather's reads (not counted: the same on both sides).

    python tools/corr_encode_bench.py [--out profiles/corr_encode_bench.json] [--reps 30]
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "droid-slam_reserch_amd"))

import droid_backends as db                                  # noqa: E402
from droid_backends.pyramid_store import PyramidStore        # noqa: E402

CAP, C, NBUF = 96, 128, 64
SHAPES = [(48, 64, 1), (48, 64, 24), (48, 64, 64), (30, 40, 64)]
STOCK_BYTES_PX, FUSED_BYTES_PX, HBM_BYTES_PER_US = 1552, 256, 8e6     # 8 TB/s


def timed(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) * 1e3   # microseconds


def stats(us):
    return dict(median_us=float(np.median(us)), min_us=float(np.min(us)), max_us=float(np.max(us)))


def alternate(group, reps, warm=3):
    for _ in range(warm):
        for fn in group.values():
            fn()
    torch.cuda.synchronize()
    us = {k: [] for k in group}
    for _ in range(reps):
        for k, fn in group.items():
            us[k].append(timed(fn))
    return {k: stats(v) for k, v in us.items()}


def one(h, w, E, reps):
    g = torch.Generator(device="cuda").manual_seed(h * w + E)
    fmaps = torch.randn((NBUF, 1, C, h, w), generator=g, device="cuda", dtype=torch.float16)
    store = PyramidStore(fmaps, CAP)
    filler = CAP - E                      # occupy and free slots first, so that the E edges sit at shuffled slots
    ii = torch.randint(0, NBUF, (CAP,), generator=g, device="cuda")
    jj = (ii + 1 + torch.randint(0, NBUF - 1, (CAP,), generator=g, device="cuda")) % NBUF
    store.add(ii, jj)
    keep = torch.zeros(CAP, dtype=torch.bool)
    keep[torch.randperm(CAP)[:E]] = True
    store.keep(keep)
    assert len(store) == E and store.grows == 0 and filler >= 0
    gy, gx = torch.meshgrid(torch.arange(h, device="cuda", dtype=torch.float32),
                            torch.arange(w, device="cuda", dtype=torch.float32), indexing="ij")
    c2hw = (torch.stack([gx, gy])[None] + 2.0 * torch.randn((E, 2, h, w), generator=g, device="cuda")).contiguous()
    coords1 = c2hw.permute(0, 2, 3, 1).contiguous()[None]                        # [1,E,h,w,2], as reproject returns it
    k = 1.0 / np.sqrt(196)
    weight = (torch.rand((128, 196, 1, 1), generator=g, device="cuda") * 2 - 1) * k
    bias = (torch.rand((128,), generator=g, device="cuda") * 2 - 1) * k
    enc = db.CorrEncoder(weight, bias)
    slots = store._slots_dev

    def tail(corr):
        with torch.autocast("cuda", dtype=torch.float16):
            return torch.relu_(torch.nn.functional.conv2d(corr, weight, bias))

    def stock():
        return tail(store(coords1)[0])

    def stock_noperm():
        return tail(db.corr_pyramid_forward(store.pyramid, c2hw, 3, slots=slots)[0])

    def fused():
        return store.encode(coords1, enc)

    def fused_2hw():
        return enc(store.pyramid, c2hw, slots=slots, layout="2hw")

    a, b = stock().float(), fused().float()
    assert a.shape == b.shape == (E, 128, h, w)
    gap = float((a - b).abs().max())
    assert gap < 0.05, gap                 # the same function (tests/test_gpu_corr_encode.py holds each to its bound)
    res = alternate(dict(stock_a=stock, fused_a=fused, stock_b=stock, fused_b=fused, stock_noperm=stock_noperm,
                         fused_2hw=fused_2hw), reps)
    aa_stock = abs(res["stock_a"]["median_us"] - res["stock_b"]["median_us"])
    aa_fused = abs(res["fused_a"]["median_us"] - res["fused_b"]["median_us"])
    s, f = res["stock_a"]["median_us"], res["fused_a"]["median_us"]
    px = E * h * w
    r = dict(h=h, w=w, E=E, cap=CAP, reps=reps, **res, aa_spread_stock_us=aa_stock, aa_spread_fused_us=aa_fused,
             fused_over_stock=f / s, fused_minus_stock_us=f - s, within=bool(f <= s + aa_stock + aa_fused),
             noperm_fused_over_stock=res["fused_2hw"]["median_us"] / res["stock_noperm"]["median_us"],
             stock_output_bytes_share_of_8TBs=STOCK_BYTES_PX * px / HBM_BYTES_PER_US / s,
             fused_output_bytes_share_of_8TBs=FUSED_BYTES_PX * px / HBM_BYTES_PER_US / f,
             max_abs_difference=gap)
    print(json.dumps(r), flush=True)
    del store
    torch.cuda.empty_cache()
    return r


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--reps", type=int, default=30)
    a = ap.parse_args()
    assert a.reps >= 20
    db._lib.load()
    res = [one(h, w, E, a.reps) for h, w, E in SHAPES]
    doc = dict(what="correlation lookup fused with corr_encoder[0:2] (one launch) vs store(coords1) -> conv2d under "
                    "autocast -> relu_ (stock); half, C = 128, PyramidStore of 96 slots; HIP-event time per call in "
                    "microseconds, alternating in one process, median of `reps`; `within`: fused median <= stock median "
                    "+ the A/A spread of both paths",
               device=torch.cuda.get_device_name(0), library=os.path.basename(db._lib.LIB_PATH), results=res)
    if a.out:
        with open(a.out, "w") as f:
            json.dump(doc, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
