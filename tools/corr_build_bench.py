#!/usr/bin/env python
"""Times the build of the all-pairs correlation pyramid with HIP events, per shape and in one process, ALTERNATING
  (a) the stock sequence as VolumeLookup.__init__ / CorrBlock.__init__ run it, in half: two gathers of the feature
      maps, two `/ 4.0`, torch.matmul, three avg_pool2d;
  (b) droid_backends.corr_volume_pyramid (one launch) on the same tensors;
and separately
  (c) `CorrBlock.cat`: torch.cat of the new edges onto a pyramid that already holds E_old edges, against
  (d) corr_volume_pyramid(out=capacity buffers, offset=E_old), which makes that copy unnecessary.
Also timed alone: the stock matmul of (a).  Bytes are computed from the shapes: `bytes_written` is the pyramid of the
E new edges, `write_TBps` = bytes_written / median time, `share_of_8TBps` its share of the HBM peak.

    python tools/corr_build_bench.py [--out profiles/corr_build_bench.json] [--reps 30]
"""
import argparse
import json
import os
import sys

import numpy as np
import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "droid-slam_reserch_amd"))

import droid_backends as db          # noqa: E402

LEVELS = 4


def stock_build(fmaps, ii, jj):
    f1 = fmaps[ii, 0]
    f2 = fmaps[jj, 0]
    n, c, h, w = f1.shape
    a = f1.reshape(n, c, h * w) / 4.0
    b = f2.reshape(n, c, h * w) / 4.0
    vol = torch.matmul(a.transpose(1, 2), b).reshape(n * h * w, 1, h, w)
    pyr = []
    for l in range(LEVELS):
        pyr.append(vol.view(n, h, w, h // 2 ** l, w // 2 ** l))
        vol = F.avg_pool2d(vol, 2, stride=2)
    return pyr


def timed(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) * 1e3   # microseconds


def stats(us):
    return dict(median_us=float(np.median(us)), min_us=float(np.min(us)), max_us=float(np.max(us)))


def pyramid_bytes(E, h, w):
    return sum(2 * E * h * w * (h >> l) * (w >> l) for l in range(LEVELS))


def one(h, w, E, E_old, reps, C=128, nbuf=64):
    g = torch.Generator(device="cuda").manual_seed(h * w + E)
    fmaps = torch.randn((nbuf, 1, C, h, w), generator=g, device="cuda", dtype=torch.float16)
    ii = torch.randint(0, nbuf, (E,), generator=g, device="cuda")
    jj = (ii + 1 + torch.randint(0, nbuf - 1, (E,), generator=g, device="cuda")) % nbuf
    a_mat = (fmaps[ii, 0].reshape(E, C, h * w) / 4.0).transpose(1, 2)
    b_mat = fmaps[jj, 0].reshape(E, C, h * w) / 4.0
    cap = [torch.empty((E_old + E, h, w, h >> l, w >> l), device="cuda", dtype=torch.float16) for l in range(LEVELS)]
    old = [c[:E_old].clone() for c in cap]
    runs = dict(
        stock=lambda: stock_build(fmaps, ii, jj),
        device=lambda: db.corr_volume_pyramid(fmaps, ii, jj, LEVELS),
        stock_matmul_alone=lambda: torch.matmul(a_mat, b_mat),
    )
    new = stock_build(fmaps, ii, jj)
    runs_cat = dict(
        stock_cat=lambda: [torch.cat([o, n], 0) for o, n in zip(old, new)],
        device_into_capacity=lambda: db.corr_volume_pyramid(fmaps, ii, jj, LEVELS, out=cap, offset=E_old),
    )
    res = {}
    for group in (runs, runs_cat):
        for _ in range(3):                      # every shape and every path warmed up
            for fn in group.values():
                fn()
        torch.cuda.synchronize()
        us = {k: [] for k in group}
        for _ in range(reps):                   # alternating, same process
            for k, fn in group.items():
                us[k].append(timed(fn))
        res.update({k: stats(v) for k, v in us.items()})
    nbytes = pyramid_bytes(E, h, w)
    for k in ("device", "device_into_capacity"):
        res[k]["write_TBps"] = nbytes / res[k]["median_us"] * 1e-6
        res[k]["share_of_8TBps"] = res[k]["write_TBps"] / 8.0
    r = dict(h=h, w=w, C=C, E=E, E_old=E_old, reps=reps, bytes_written=nbytes,
             bytes_copied_by_cat=2 * pyramid_bytes(E_old + E, h, w), **res,
             speedup_build=res["stock"]["median_us"] / res["device"]["median_us"],
             build_gap_exceeds_spreads=bool(res["stock"]["median_us"] - res["device"]["median_us"] > max(
                 res["stock"]["max_us"] - res["stock"]["min_us"], res["device"]["max_us"] - res["device"]["min_us"])))
    print(json.dumps(r))
    return r


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--reps", type=int, default=30)
    a = ap.parse_args()
    assert a.reps >= 20
    db._lib.load()
    res = [one(48, 64, 32, 64, a.reps), one(48, 64, 6, 64, a.reps), one(30, 40, 32, 64, a.reps)]
    doc = dict(what="build of the half correlation pyramid (4 levels, C = 128): HIP-event time per call in microseconds, "
                    "stock PyTorch sequence vs corr_volume_pyramid, alternating in one process; torch.cat onto E_old "
                    "edges vs a build into capacity buffers", device=torch.cuda.get_device_name(0), results=res)
    if a.out:
        with open(a.out, "w") as f:
            json.dump(doc, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
