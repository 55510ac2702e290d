#!/usr/bin/env python
"""Times the 3 x 3 convolution + ReLU of the update operator (Conv3x3 -> droid_conv3x3) against the stock layer, with HIP
events, per shape and in one process, ALTERNATING the variants:
  stock_a, stock_b    F.conv2d(x, w16, b16, padding=1) -> relu_ on half tensors, the weights cast beforehand: what
                      autocast runs with its cast cache warm (the A/A pair is the noise of this path in this run); for a
                      pair, the two stock layers one after the other
  fused_a, fused_b    conv(x)                                                      (one launch; A/A pair)
48x64: 128->128 with E = 1 (motion filter), 24 (frontend window), 64, 256 and 2000 (global BA), 128->64 with E = 24, the
pair 128->2x128 with E = 24 and 64, 128->128 with G = 8 (agg.conv2); 30x40: 128->128 with E = 64.  Acceptance per shape
(`faster`): median(fused_a) < median(stock_a) - the A/A spread of the two paths.  Also per shape: the TFLOP/s achieved
against the 2.5 PF f16 peak and the algorithmic bytes (x read once, y written once, the packed weights once) against
8 TB/s.

    python tools/conv3x3_bench.py [--out profiles/conv3x3_bench.json] [--reps 30] [--only-fused]
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

# (h, w, C_in, C_out of a layer, layers, batch, what)
SHAPES = [(48, 64, 128, 128, 1, 1, "E=1"), (48, 64, 128, 128, 1, 24, "E=24"), (48, 64, 128, 128, 1, 64, "E=64"),
          (48, 64, 128, 128, 1, 256, "E=256"), (48, 64, 128, 128, 1, 2000, "E=2000"), (48, 64, 128, 64, 1, 24, "E=24"),
          (48, 64, 128, 128, 2, 24, "pair E=24"), (48, 64, 128, 128, 2, 64, "pair E=64"),
          (48, 64, 128, 128, 1, 8, "agg.conv2 G=8"), (30, 40, 128, 128, 1, 64, "E=64")]
ACCEPTANCE = {(48, 64, 128, 128, 1, 1), (48, 64, 128, 128, 1, 24), (48, 64, 128, 128, 1, 64), (48, 64, 128, 128, 2, 24)}
HBM_BYTES_PER_US, PEAK_FLOP_PER_US = 8e6, 2.5e9     # 8 TB/s, 2.5 PFLOP/s


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


def one(h, w, c_in, c_out, k, B, what, reps, only_fused):
    g = torch.Generator(device="cuda").manual_seed(h * w + B + c_out + k)
    bound = 1.0 / np.sqrt(9 * c_in)     # nn.Conv2d's init scale
    ws = [((torch.rand((c_out, c_in, 3, 3), generator=g, device="cuda") * 2 - 1) * bound).half() for _ in range(k)]
    bs = [((torch.rand((c_out,), generator=g, device="cuda") * 2 - 1) * bound).half() for _ in range(k)]
    x = torch.relu(torch.randn((B, c_in, h, w), generator=g, device="cuda")).half()      # a ReLU's output, as in the network
    conv = db.Conv3x3(ws[0], bs[0], relu=True) if k == 1 else db.Conv3x3(list(zip(ws, bs)), relu=True)

    def stock():
        return [torch.relu_(torch.nn.functional.conv2d(x, wt, b, padding=1)) for wt, b in zip(ws, bs)]

    def fused():
        return conv(x)

    group = dict(fused_a=fused, fused_b=fused) if only_fused else dict(stock_a=stock, fused_a=fused, stock_b=stock, fused_b=fused)
    f0 = fused()
    f0 = [f0] if k == 1 else list(f0)
    gap = None
    if not only_fused:
        gap = max(float((a.float() - b.float()).abs().max()) for a, b in zip(stock(), f0))
        # the same function up to the stock half convolution's own error (tests/test_gpu_conv3x3.py holds the fused one
        # to its bound and prints the stock chain's distance)
        assert gap <= 2.0 ** -7 * max(1.0, max(float(a.abs().max()) for a in f0)), gap
    res = alternate(group, reps)
    f = res["fused_a"]["median_us"]
    aa_fused = abs(f - res["fused_b"]["median_us"])
    flop = 2.0 * B * h * w * k * c_out * 9 * c_in
    nbytes = 2.0 * (B * h * w * (c_in + k * c_out) + k * c_out * (9 * c_in + 1))
    r = dict(h=h, w=w, c_in=c_in, c_out=c_out, layers=k, batch=B, what=what, reps=reps, **res, aa_spread_fused_us=aa_fused,
             fused_tflops=flop / f / 1e6, fused_share_of_2_5PF=flop / f / PEAK_FLOP_PER_US,
             fused_bytes_share_of_8TBs=nbytes / HBM_BYTES_PER_US / f, acceptance_shape=(h, w, c_in, c_out, k, B) in ACCEPTANCE)
    if not only_fused:
        s = res["stock_a"]["median_us"]
        aa_stock = abs(s - res["stock_b"]["median_us"])
        r.update(aa_spread_stock_us=aa_stock, fused_over_stock=f / s, fused_minus_stock_us=f - s,
                 faster=bool(f < s - (aa_stock + aa_fused)), stock_tflops=flop / s / 1e6, max_abs_difference=gap)
    print(json.dumps(r), flush=True)
    del x, f0
    torch.cuda.empty_cache()
    return r


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--only-fused", action="store_true", help="no stock side: for a kernel trace of the fused launches")
    a = ap.parse_args()
    assert a.reps >= 5
    db._lib.load()
    res = [one(*shape, a.reps, a.only_fused) for shape in SHAPES]
    doc = dict(what="Conv2d(C_in, C_out, 3, padding=1) + ReLU on half planes: Conv3x3 (one launch) vs F.conv2d on half "
                    "tensors -> relu_ (stock, weights cast beforehand; a pair against its two stock layers); HIP-event time "
                    "per call in microseconds, alternating in one process, median of `reps`; `faster`: fused median < stock "
                    "median - the A/A spread of both paths",
               device=torch.cuda.get_device_name(0), library=os.path.basename(db._lib.LIB_PATH), results=res)
    if a.out:
        with open(a.out, "w") as f:
            json.dump(doc, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
