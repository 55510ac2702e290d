#!/usr/bin/env python
"""Times `DepthVideo.upsample` with HIP events, per shape and in one process, ALTERNATING
  (a) the stock sequence -- tests/cvx_upsample_ref.py `stock`: gather, softmax over 9, F.unfold, multiply, sum, pixel
      shuffle, index_put -- and
  (b) droid_backends.upsample_disps (one launch) on the same tensors.
Each round runs a, b, a, b: two series of `reps` samples per path, so that every path has an A/A spread (the distance
between the medians of its own two series) next to its time (the median of the first series).  `not_slower` is the
acceptance: fused - stock <= the larger of the two A/A spreads.  Bytes are computed from the shapes: per coarse pixel the
fused kernel reads 576 s + 4 (s = bytes per logit) and writes 256; `TBps` = those bytes / median time, `share_of_8TBps`
its share of the HBM peak (between repetitions the mask can stay in the 256 MiB last-level cache, as it can in the
pipeline, where the update operator has just written it).

    python tools/cvx_upsample_bench.py [--out profiles/cvx_upsample_bench.json] [--reps 30]
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "droid-slam_reserch_amd"))
sys.path.insert(0, os.path.join(ROOT, "tests"))

import droid_backends as db          # noqa: E402
from cvx_upsample_ref import stock   # noqa: E402

NBUF = 64


def timed(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) * 1e3   # microseconds


def stats(us, us2):
    return dict(median_us=float(np.median(us)), min_us=float(np.min(us)), max_us=float(np.max(us)),
                aa_spread_us=float(abs(np.median(us) - np.median(us2))))


def algorithmic_bytes(n, h, w, s):
    return n * h * w * (576 * s + 4 + 256)


def one(h, w, n, dtype, reps):
    g = torch.Generator(device="cuda").manual_seed(h * w + n)
    disps = torch.rand((NBUF, h, w), generator=g, device="cuda") * 10 + 0.001
    ix = torch.randperm(NBUF, generator=g, device="cuda")[:n].sort().values     # torch.unique(ii): sorted, distinct
    mask = (torch.randn((1, n, 576, h, w), generator=g, device="cuda") * 4).to(dtype)
    out_a = torch.zeros((NBUF, 8 * h, 8 * w), device="cuda")
    out_b = torch.zeros_like(out_a)
    runs = dict(stock=lambda: stock(disps, mask[0], ix, out_a), fused=lambda: db.upsample_disps(disps, ix, mask, out_b))
    for _ in range(3):                          # every shape and every path warmed up
        for fn in runs.values():
            fn()
    torch.cuda.synchronize()
    us = {(k, r): [] for k in runs for r in (0, 1)}
    for _ in range(reps):                       # alternating, same process
        for r in (0, 1):
            for k, fn in runs.items():
                us[k, r].append(timed(fn))
    res = {k: stats(us[k, 0], us[k, 1]) for k in runs}
    s = mask.element_size()
    nbytes = algorithmic_bytes(n, h, w, s)
    res["fused"]["TBps"] = nbytes / res["fused"]["median_us"] * 1e-6
    res["fused"]["share_of_8TBps"] = res["fused"]["TBps"] / 8.0
    diff = float((out_a[ix] - out_b[ix]).abs().max())
    r = dict(h=h, w=w, n=n, mask_dtype=str(dtype).replace("torch.", ""), reps=reps, algorithmic_bytes=nbytes, **res,
             stock_over_fused=res["stock"]["median_us"] / res["fused"]["median_us"],
             not_slower=bool(res["fused"]["median_us"] - res["stock"]["median_us"]
                             <= max(res["stock"]["aa_spread_us"], res["fused"]["aa_spread_us"])),
             max_abs_difference=diff)
    print(json.dumps(r), flush=True)
    return r


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--reps", type=int, default=30)
    a = ap.parse_args()
    assert a.reps >= 20
    db._lib.load()
    half, f32 = torch.float16, torch.float32
    res = [one(48, 64, 8, half, a.reps), one(48, 64, 16, half, a.reps), one(48, 64, 48, half, a.reps),
           one(96, 128, 8, half, a.reps), one(48, 64, 16, f32, a.reps)]
    doc = dict(what="DepthVideo.upsample (convex upsampling of n disparity maps, 8x): HIP-event time per call in "
                    "microseconds, stock PyTorch sequence vs upsample_disps (one launch), alternating in one process; "
                    "median of the first of two interleaved series per path, aa_spread_us = distance between the "
                    "medians of the two series", device=torch.cuda.get_device_name(0), results=res)
    if a.out:
        with open(a.out, "w") as f:
            json.dump(doc, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
