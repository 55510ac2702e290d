#!/usr/bin/env python
"""Times reproject + motion features fused with flow_encoder[0:2] (FlowEncoder -> droid_motion_encode) against the stock
sequence, with HIP events, per shape and in one process, ALTERNATING the variants:
  stock_a, stock_b    droid_backends.motion_features -> F.conv2d(..., padding=3) under autocast -> relu_
                      (the reprojection, the cast of the planes, the vendor's 7 x 7 convolution, the ReLU; the A/A
                      pair is the noise of this path in this run)
  fused_a, fused_b    enc(poses, disps, intrinsics, ii, jj, target)                (one launch; A/A pair)
  conv_stock          F.conv2d(motn, ..., padding=3) under autocast -> relu_        (the layers alone, on given planes)
  conv_fused          enc.conv(motn)
  reproject_new, reproject_parent, reproject_new_b, reproject_parent_b (with --parent-lib)   the C entry point
                      droid_reproject_motion without a target on preallocated outputs, this library against the parent
                      commit's build of it, interleaved: the per-pixel body moved into a shared device function
A 512-frame buffer with per-frame intrinsics; 48x64 with E = 1 (motion filter), 24 (frontend window), 64 and 2000
(global BA), and 30x40 with E = 64.  Acceptance per shape (`faster`): median(fused_a) < median(stock_a) - the A/A spread
of the two paths.  The baseline is the stock sequence of the same run.
Algorithmic bytes per pixel on top of what both sides read (disps 4, target 8) and write (coords 8, valid 4): stock 16
(planes written) + 16 + 8 (cast) + 8 + 256 (convolution) + 256 + 256 (ReLU) = 816, fused 256; on given planes 800
against 16 + 256 = 272.

    python tools/motion_encode_bench.py [--out profiles/motion_encode_bench.json] [--reps 30] [--parent-lib PATH]
"""
import argparse
import ctypes
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "droid-slam_reserch_amd"))

import droid_backends as db                                  # noqa: E402

NBUF = 512
SHAPES = [(48, 64, 1), (48, 64, 24), (48, 64, 64), (48, 64, 2000), (30, 40, 64)]
STOCK_BYTES_PX, FUSED_BYTES_PX, CONV_STOCK_BYTES_PX, CONV_FUSED_BYTES_PX = 816, 256, 800, 272
HBM_BYTES_PER_US = 8e6     # 8 TB/s


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


def scene(h, w, E, g):
    """A 512-frame buffer on a gentle trajectory, per-frame intrinsics, E edges between near frames (every 16th a
    stereo edge), target = the reprojection + noise."""
    poses = torch.zeros((NBUF, 7), device="cuda")
    poses[:, :3] = 0.02 * torch.randn((NBUF, 3), generator=g, device="cuda") \
        + 0.01 * torch.arange(NBUF, device="cuda")[:, None] * torch.tensor([1.0, 0.2, 0.1], device="cuda")
    q = torch.cat([0.02 * torch.randn((NBUF, 3), generator=g, device="cuda"), torch.ones((NBUF, 1), device="cuda")], 1)
    poses[:, 3:] = q / q.norm(dim=1, keepdim=True)
    disps = 0.3 + 1.7 * torch.rand((NBUF, h, w), generator=g, device="cuda")
    K = torch.tensor([0.9 * w, 0.62 * w, 0.38 * w + 0.5, 0.36 * h - 0.75], device="cuda")
    Ks = (K[None] * (1.0 + 0.01 * (torch.arange(NBUF, device="cuda") % 5)[:, None])).contiguous()
    ii = torch.randint(0, NBUF, (E,), generator=g, device="cuda")
    jj = (ii + torch.randint(1, 4, (E,), generator=g, device="cuda")) % NBUF
    jj[::16] = ii[::16]
    coords, _ = db.reproject(poses, disps, Ks, ii, jj)
    target = (coords + 2.0 * torch.randn(coords.shape, generator=g, device="cuda")).contiguous()
    return poses, disps, Ks, ii, jj, target


def parent_reproject(path):
    """droid_reproject_motion of another build of the library, bound like the package binds its own."""
    lib = ctypes.CDLL(path)
    fn = lib.droid_reproject_motion
    fn.restype, fn.argtypes = db._lib.signature("droid_reproject_motion")
    return fn


def one(h, w, E, reps, parent):
    g = torch.Generator(device="cuda").manual_seed(h * w + E)
    poses, disps, Ks, ii, jj, target = scene(h, w, E, g)
    k = 1.0 / np.sqrt(196)
    weight = (torch.rand((128, 4, 7, 7), generator=g, device="cuda") * 2 - 1) * k
    bias = (torch.rand((128,), generator=g, device="cuda") * 2 - 1) * k
    enc = db.FlowEncoder(weight, bias)
    motn = db.motion_features(poses, disps, Ks, ii, jj, target)[0][0].contiguous()

    def tail(m):
        with torch.autocast("cuda", dtype=torch.float16):
            return torch.relu_(torch.nn.functional.conv2d(m, weight, bias, padding=3))

    def stock():
        return tail(db.motion_features(poses, disps, Ks, ii, jj, target)[0][0])

    def fused():
        return enc(poses, disps, Ks, ii, jj, target)[0]

    def conv_stock():
        return tail(motn)

    def conv_fused():
        return enc.conv(motn)

    coords_n = torch.empty((1, E, h, w, 2), device="cuda")
    valid_n = torch.empty((1, E, h, w, 1), device="cuda")

    def raw_reproject(fn, coords, valid):   # the C entry point itself on preallocated outputs: the same host work for both builds
        rc = fn(poses.data_ptr(), disps.data_ptr(), Ks.data_ptr(), 4, ii.data_ptr(), jj.data_ptr(), None, E, NBUF, h, w,
                coords.data_ptr(), valid.data_ptr(), None, torch.cuda.current_stream().cuda_stream)
        assert rc == 0

    def reproject_new():
        raw_reproject(db._lib.load().droid_reproject_motion, coords_n, valid_n)

    a, b = stock().float(), fused().float()
    assert a.shape == b.shape == (E, 128, h, w)
    gap = float((a - b).abs().max())
    # the same function up to the stock half convolution's own error, a few half ulps of the largest output
    # (tests/test_gpu_motion_encode.py holds the fused one to its bound and prints the stock chain's distance)
    assert gap <= 2.0 ** -8 * max(1.0, float(a.abs().max())), gap
    group = dict(stock_a=stock, fused_a=fused, stock_b=stock, fused_b=fused, conv_stock=conv_stock, conv_fused=conv_fused,
                 reproject_new=reproject_new)
    if parent is not None:
        coords = torch.empty((1, E, h, w, 2), device="cuda")
        valid = torch.empty((1, E, h, w, 1), device="cuda")
        want_c, want_v = db.reproject(poses, disps, Ks, ii, jj)

        def reproject_parent():
            raw_reproject(parent, coords, valid)
        reproject_parent()
        torch.cuda.synchronize()
        same_bits = bool(torch.equal(coords.view(torch.int32), want_c.view(torch.int32))
                         and torch.equal(valid.view(torch.int32), want_v.view(torch.int32)))
        group["reproject_parent"] = reproject_parent      # new, parent, new, parent: neither build always runs second
        group["reproject_new_b"] = reproject_new
        group["reproject_parent_b"] = reproject_parent
    else:
        group["reproject_new_b"] = reproject_new
    res = alternate(group, reps)
    aa_stock = abs(res["stock_a"]["median_us"] - res["stock_b"]["median_us"])
    aa_fused = abs(res["fused_a"]["median_us"] - res["fused_b"]["median_us"])
    s, f = res["stock_a"]["median_us"], res["fused_a"]["median_us"]
    cs, cf = res["conv_stock"]["median_us"], res["conv_fused"]["median_us"]
    px = E * h * w
    r = dict(h=h, w=w, E=E, nbuf=NBUF, reps=reps, **res, aa_spread_stock_us=aa_stock, aa_spread_fused_us=aa_fused,
             fused_over_stock=f / s, fused_minus_stock_us=f - s, faster=bool(f < s - (aa_stock + aa_fused)),
             conv_fused_over_stock=cf / cs,
             stock_bytes_share_of_8TBs=STOCK_BYTES_PX * px / HBM_BYTES_PER_US / s,
             fused_bytes_share_of_8TBs=FUSED_BYTES_PX * px / HBM_BYTES_PER_US / f,
             conv_stock_bytes_share_of_8TBs=CONV_STOCK_BYTES_PX * px / HBM_BYTES_PER_US / cs,
             conv_fused_bytes_share_of_8TBs=CONV_FUSED_BYTES_PX * px / HBM_BYTES_PER_US / cf,
             aa_spread_reproject_us=abs(res["reproject_new"]["median_us"] - res["reproject_new_b"]["median_us"]),
             max_abs_difference=gap)
    if parent is not None:
        r["reproject_new_minus_parent_us"] = res["reproject_new"]["median_us"] - res["reproject_parent"]["median_us"]
        r["reproject_new_b_minus_parent_b_us"] = res["reproject_new_b"]["median_us"] - res["reproject_parent_b"]["median_us"]
        r["aa_spread_reproject_parent_us"] = abs(res["reproject_parent"]["median_us"] - res["reproject_parent_b"]["median_us"])
        r["reproject_bits_equal_parent"] = same_bits
    print(json.dumps(r), flush=True)
    torch.cuda.empty_cache()
    return r


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--parent-lib", default=None, help="the parent commit's libdroid_backends_hip.so: A/B of plain reproject")
    a = ap.parse_args()
    assert a.reps >= 20
    db._lib.load()
    parent = parent_reproject(a.parent_lib) if a.parent_lib else None
    res = [one(h, w, E, a.reps, parent) for h, w, E in SHAPES]
    doc = dict(what="reproject + motion features fused with flow_encoder[0:2] (one launch) vs motion_features -> conv2d "
                    "(padding=3) under autocast -> relu_ (stock); 512-frame buffer, per-frame intrinsics; HIP-event time "
                    "per call in microseconds, alternating in one process, median of `reps`; `faster`: fused median < "
                    "stock median - the A/A spread of both paths; conv_*: the two layers alone on given planes; "
                    "reproject_*: plain reproject of this library and of the parent commit's",
               device=torch.cuda.get_device_name(0), library=os.path.basename(db._lib.LIB_PATH), results=res)
    if a.out:
        with open(a.out, "w") as f:
            json.dump(doc, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
