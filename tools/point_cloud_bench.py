#!/usr/bin/env python
"""Times the viewers' point cloud of n dirty keyframes with HIP events, per shape and in one process, ALTERNATING
  (a) the stock sequence (visualization.py:100-142 of the reference fork) through this module's own operators --
      index_select, SE3(poses).inv(), iproj, depth_filter, the count / disparity mask -- and
  (b) droid_backends.point_cloud(...),
each in two forms: `device` ends with the results on the device (stock: points, counts and mask, not yet compacted;
fused: sync=False, compacted), `host` ends with the per-frame point and colour arrays on the host, copies included
(stock: the full-resolution images, all points, counts and disparities cross, then boolean indexing frame by frame on the
CPU; fused: one read of offsets, one copy of the trimmed tensors, slicing by offsets_host).  The host forms are timed
with the HIP events around them too: the closing event is recorded after the last copy has completed.
Each round runs the four paths twice: two series of `reps` samples per path, so that every path has an A/A spread (the
distance between the medians of its own two series) next to its time (the median of the first series).  `faster` is the
acceptance: stock - fused > the larger of the two A/A spreads.  Bytes moved to the host are computed from the shapes and
the number of points kept.  The inputs are the two-plane scene of tests/point_cloud_cases.py at 48 x 64, extended to n
frames.

    python tools/point_cloud_bench.py [--out profiles/point_cloud_bench.json] [--reps 30]
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (os.path.join(ROOT, "tests"), ROOT, os.path.join(ROOT, "droid-slam_reserch_amd")):
    sys.path.insert(0, p)

import droid_backends as db          # noqa: E402
import point_cloud_cases as pcc      # noqa: E402

H, W = 48, 64
THRESH = 0.1


def scene(n):
    """n frames: the nine frames of the 48 x 64 case, repeated in mirrored order (0 .. 8, 7 .. 0, 1 ..), so that every
    temporal neighbourhood is one the case has or its mirror image, and depths stay consistent across neighbours."""
    case = pcc.Case(H, W, "aniso", THRESH)
    period = np.concatenate([np.arange(pcc.NBUF), np.arange(pcc.NBUF - 2, 0, -1)])
    f = period[np.arange(n) % len(period)]
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()
    return t(case.poses[f]), t(case.disps[f]), t(case.K), t(case.images[f])


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


def stock_device(poses, disps, K, images, index, thresh):
    p = torch.index_select(poses, 0, index)
    d = torch.index_select(disps, 0, index)
    Ps = db.SE3(p).inv().matrix()
    points = db.iproj(db.SE3(p).inv().data, d, K)
    count = db.depth_filter(poses, disps, K, index, thresh)
    masks = (count >= 2) & (d > .5 * d.mean(dim=[1, 2], keepdim=True))
    return Ps, points, masks, d, count


def stock_host(poses, disps, K, images, index, thresh):
    p = torch.index_select(poses, 0, index)
    d = torch.index_select(disps, 0, index)
    Ps = db.SE3(p).inv().matrix().cpu().numpy()
    imgs = torch.index_select(images, 0, index).cpu()[:, [2, 1, 0], 3::8, 3::8].permute(0, 2, 3, 1) / 255.0
    points = db.iproj(db.SE3(p).inv().data, d, K).cpu()
    count = db.depth_filter(poses, disps, K, index, thresh).cpu()
    dc = d.cpu()
    masks = (count >= 2) & (dc > .5 * dc.mean(dim=[1, 2], keepdim=True))
    out = []
    for i in range(len(index)):
        m = masks[i].reshape(-1)
        out.append((points[i].reshape(-1, 3)[m].numpy(), imgs[i].reshape(-1, 3)[m].numpy()))
    return Ps, out


def fused_device(poses, disps, K, images, index, thresh):
    return db.point_cloud(poses, disps, K, index, thresh, images, sync=False)


def fused_host(poses, disps, K, images, index, thresh):
    pc = db.point_cloud(poses, disps, K, index, thresh, images)
    pts, clr, Ps, off = pc.points.cpu().numpy(), pc.colors.cpu().numpy(), pc.matrices.cpu().numpy(), pc.offsets_host
    return Ps, [(pts[off[b]:off[b + 1]], clr[off[b]:off[b + 1]]) for b in range(len(off) - 1)]


def one(n, reps):
    poses, disps, K, images = scene(n)
    index = torch.arange(n, device="cuda")          # after a global BA every keyframe is dirty
    thresh = torch.full((n,), THRESH, device="cuda")
    args = (poses, disps, K, images, index, thresh)
    runs = dict(stock_device=stock_device, fused_device=fused_device, stock_host=stock_host, fused_host=fused_host)
    for _ in range(3):                              # every shape and every path warmed up
        for fn in runs.values():
            fn(*args)
    torch.cuda.synchronize()
    us = {(k, r): [] for k in runs for r in (0, 1)}
    for _ in range(reps):                           # alternating, same process
        for r in (0, 1):
            for k, fn in runs.items():
                us[k, r].append(timed(lambda: fn(*args)))
    res = {k: stats(us[k, 0], us[k, 1]) for k in runs}
    # same answer: membership may differ only at undecided pixels (none of the two chains is the fp64 reference)
    Ps_s, out_s = stock_host(*args)
    Ps_f, out_f = fused_host(*args)
    rows_s, rows_f = sum(len(p) for p, _ in out_s), sum(len(p) for p, _ in out_f)
    same_rows = [b for b in range(n) if len(out_s[b][0]) == len(out_f[b][0])]
    dist = max(float(np.abs(out_s[b][0] - out_f[b][0]).max()) for b in same_rows if len(out_s[b][0]))
    colours_equal = all(np.array_equal(out_s[b][1], out_f[b][1]) for b in same_rows)
    hw = H * W
    stock_bytes = n * (3 * 64 * hw + 12 * hw + 4 * hw + 4 * hw + 64)     # images, points, counts, disparities, matrices
    fused_bytes = rows_f * 24 + (n + 1) * 4 + n * 64                     # points, colours, offsets, matrices
    faster = {form: bool(res["stock_" + form]["median_us"] - res["fused_" + form]["median_us"]
                         > max(res["stock_" + form]["aa_spread_us"], res["fused_" + form]["aa_spread_us"]))
              for form in ("device", "host")}
    r = dict(h=H, w=W, image=[8 * H, 8 * W], n=n, reps=reps, points_kept=rows_f, points_kept_stock=rows_s,
             frames_with_equal_membership=len(same_rows), largest_point_distance=dist, colours_equal=colours_equal,
             bytes_to_host=dict(stock=stock_bytes, fused=fused_bytes),
             stock_device=res["stock_device"], fused_device=res["fused_device"], stock_host=res["stock_host"],
             fused_host=res["fused_host"],
             stock_over_fused=dict(device=res["stock_device"]["median_us"] / res["fused_device"]["median_us"],
                                   host=res["stock_host"]["median_us"] / res["fused_host"]["median_us"]),
             faster=faster)
    print(json.dumps(r), flush=True)
    return r


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--reps", type=int, default=30)
    a = ap.parse_args()
    assert a.reps >= 20
    db._lib.load()
    res = [one(n, a.reps) for n in (8, 64, 512)]
    doc = dict(what="filtered, coloured point cloud of n dirty keyframes (48 x 64 maps, 384 x 512 images): HIP-event time per "
                    "call in microseconds, the stock sequence of the viewers through this module's SE3 / iproj / depth_filter "
                    "vs droid_backends.point_cloud, alternating in one process; `device`: results left on the device (fused: "
                    "sync=False), `host`: per-frame arrays on the host, copies included; median of the first of two "
                    "interleaved series per path, aa_spread_us = distance between the medians of the two series",
               device=torch.cuda.get_device_name(0), results=res)
    if a.out:
        with open(a.out, "w") as f:
            json.dump(doc, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
