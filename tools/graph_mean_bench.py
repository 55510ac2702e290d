#!/usr/bin/env python
"""Times `GraphAgg.forward`'s source-frame mean with HIP events, per shape and in one process, ALTERNATING
  (a) the stock sequence a user without torch_scatter writes -- torch.unique(ii, return_inverse=True), zeros +
      index_add_, bincount, divide -- and
  (b) droid_backends.graph_mean(net, ii) (the same unique for M, then two launches), and
  (c) droid_backends.graph_mean(net, ii, num_groups=M, nbuf=NBUF) (no host read: what a caller that knows M pays).
Each round runs a, b, c, a, b, c: two series of `reps` samples per path, so that every path has an A/A spread (the
distance between the medians of its own two series) next to its time (the median of the first series).  `faster` is the
acceptance: stock - fused > the A/A spreads of the two paths together, for (b) and for (c).  Bytes are computed from the
shapes, (E + M) * plane * sizeof(T): `TBps` = those bytes / median time of (c), `share_of_8TBps` its share of the HBM
peak (between repetitions the smaller inputs stay in the 256 MiB last-level cache, as they do in the pipeline, where
conv1 has just written them).  `prepare_us` is the same call at plane = 8 -- the prepare kernel plus a reduce launch with
next to nothing to do -- and `prepare_share` its share of (c).

    python tools/graph_mean_bench.py [--out profiles/graph_mean_bench.json] [--reps 30]
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "droid-slam_reserch_amd"))

import droid_backends as db          # noqa: E402

NBUF = 512
C = 128


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


def stock(net, ii):
    uniq, ix = torch.unique(ii, return_inverse=True)
    m = int(uniq.numel())
    s = torch.zeros((1, m) + tuple(net.shape[2:]), dtype=net.dtype, device=net.device).index_add_(1, ix, net)
    n = torch.bincount(ix, minlength=m)
    return s / n.view(1, m, 1, 1, 1).to(net.dtype)


def one(h, w, E, sources, dtype, reps):
    g = torch.Generator(device="cuda").manual_seed(h * w + E)
    frames = torch.randperm(NBUF, generator=g, device="cuda")[:sources]
    ii = frames[torch.randint(0, sources, (E,), generator=g, device="cuda")]
    ii[:sources] = frames                                   # every source has at least one edge
    net = torch.randn((1, E, C, h, w), generator=g, device="cuda").to(dtype)
    small = net[:, :, :1, :1, :8].contiguous()              # plane = 8: the prepare step next to alone
    runs = dict(stock=lambda: stock(net, ii), fused=lambda: db.graph_mean(net, ii),
                fused_known=lambda: db.graph_mean(net, ii, num_groups=sources, nbuf=NBUF),
                prepare=lambda: db.graph_mean(small, ii, num_groups=sources, nbuf=NBUF))
    for _ in range(3):                                      # every shape and every path warmed up
        for fn in runs.values():
            fn()
    torch.cuda.synchronize()
    us = {(k, r): [] for k in runs for r in (0, 1)}
    for _ in range(reps):                                   # alternating, same process
        for r in (0, 1):
            for k, fn in runs.items():
                us[k, r].append(timed(fn))
    res = {k: stats(us[k, 0], us[k, 1]) for k in runs}
    nbytes = (E + sources) * C * h * w * net.element_size()
    res["fused_known"]["TBps"] = nbytes / res["fused_known"]["median_us"] * 1e-6
    res["fused_known"]["share_of_8TBps"] = res["fused_known"]["TBps"] / 8.0
    a, b = stock(net, ii), db.graph_mean(net, ii)
    same = bool(torch.equal(b, db.graph_mean(net, ii, num_groups=sources, nbuf=NBUF)))
    faster = {k: bool(res["stock"]["median_us"] - res[k]["median_us"]
                      > res["stock"]["aa_spread_us"] + res[k]["aa_spread_us"]) for k in ("fused", "fused_known")}
    r = dict(h=h, w=w, E=E, sources=sources, dtype=str(dtype).replace("torch.", ""), reps=reps, algorithmic_bytes=nbytes,
             stock=res["stock"], fused=res["fused"], fused_known=res["fused_known"],
             prepare_us=res["prepare"]["median_us"],
             prepare_share=res["prepare"]["median_us"] / res["fused_known"]["median_us"],
             stock_over_fused=res["stock"]["median_us"] / res["fused"]["median_us"],
             stock_over_fused_known=res["stock"]["median_us"] / res["fused_known"]["median_us"],
             faster=faster, both_fused_paths_same_bits=same,
             max_abs_difference_from_stock=float((a.float() - b.float()).abs().max()))
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
    res = [one(48, 64, 24, 8, half, a.reps), one(48, 64, 96, 16, half, a.reps), one(48, 64, 2000, 256, half, a.reps),
           one(30, 40, 96, 16, half, a.reps), one(48, 64, 96, 16, f32, a.reps)]
    doc = dict(what="GraphAgg's source-frame mean (scatter_mean of [1, E, 128, h, w] over the edges' sources): HIP-event "
                    "time per call in microseconds, stock PyTorch sequence (unique, zeros + index_add_, bincount, divide) "
                    "vs graph_mean (prepare + reduce launch; `fused` takes M from the same unique, `fused_known` is told "
                    "M and reads nothing), alternating in one process; median of the first of two interleaved series per "
                    "path, aa_spread_us = distance between the medians of the two series",
               device=torch.cuda.get_device_name(0), results=res)
    if a.out:
        with open(a.out, "w") as f:
            json.dump(doc, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
