#!/usr/bin/env python
"""Times the ConvGRU of the update operator (ConvGRU -> droid_conv_gru, four launches) against the stock module, with HIP
events, per shape and in one process, ALTERNATING the variants:
  stock_a, stock_b    the module's lines on half tensors with its three torch.cat, the weights cast beforehand: what
                      autocast runs with its cast cache warm (the A/A pair is the noise of this path in this run)
  fused_a, fused_b    gru(net, inp, corr, flow)                                   (A/A pair)
48x64 with E = 1 (motion filter), 24 (frontend window), 64 and 256; 30x40 with E = 64.  Acceptance at 48x64, E = 1, 24,
64 (`faster`): median(fused_a) < median(stock_a) - the A/A spread of the two paths.  Also per shape: the TFLOP/s achieved
against the 2.5 PF f16 peak and the algorithmic bytes (the four inputs read once -- inp, corr and flow twice, for the two
gate launches -- z and rnet written and read, out written, the packed weights once) against 8 TB/s.

    python tools/conv_gru_bench.py [--out profiles/conv_gru_bench.json] [--reps 30] [--only-fused] [--shape 48x64x24]
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

import droid_backends as db                                  # noqa: E402
from droid_backends.conv_gru import LAYERS                   # noqa: E402

sys.path.insert(0, os.path.join(ROOT, "tools"))
from conv3x3_bench import HBM_BYTES_PER_US, PEAK_FLOP_PER_US, alternate      # noqa: E402

SHAPES = [(48, 64, 1), (48, 64, 24), (48, 64, 64), (48, 64, 256), (30, 40, 64)]
ACCEPTANCE = {(48, 64, 1), (48, 64, 24), (48, 64, 64)}
SPLITS, C_IN = (128, 128, 64), 448


def one(h, w, B, reps, only_fused):
    g = torch.Generator(device="cuda").manual_seed(h * w + B)
    p = {}
    for k in LAYERS:
        c, ks = (C_IN, 3) if k in LAYERS[:3] else (128, 1)
        bound = 1.0 / np.sqrt(ks * ks * c)     # nn.Conv2d's init scale
        p[k] = (((torch.rand((128, c, ks, ks), generator=g, device="cuda") * 2 - 1) * bound).half(),
                ((torch.rand((128,), generator=g, device="cuda") * 2 - 1) * bound).half())
    net = torch.tanh(torch.randn((B, 128, h, w), generator=g, device="cuda")).half()
    inputs = [torch.relu(torch.randn((B, c, h, w), generator=g, device="cuda")).half() for c in SPLITS]
    gru = db.ConvGRU(**p)
    cv = lambda k, x, pad: F.conv2d(x, p[k][0], p[k][1], padding=pad)

    def stock():
        inp = torch.cat(inputs, dim=1)
        net_inp = torch.cat([net, inp], dim=1)
        glo = torch.sigmoid(cv("w", net, 0)) * net
        glo = glo.view(B, 128, h * w).mean(-1).view(B, 128, 1, 1)
        z = torch.sigmoid(cv("convz", net_inp, 1) + cv("convz_glo", glo, 0))
        r = torch.sigmoid(cv("convr", net_inp, 1) + cv("convr_glo", glo, 0))
        q = torch.tanh(cv("convq", torch.cat([r * net, inp], dim=1), 1) + cv("convq_glo", glo, 0))
        return (1 - z) * net + z * q

    def fused():
        return gru(net, *inputs)

    group = dict(fused_a=fused, fused_b=fused) if only_fused else dict(stock_a=stock, fused_a=fused, stock_b=stock, fused_b=fused)
    f0 = fused()
    gap = None
    if not only_fused:
        gap = float((stock().float() - f0.float()).abs().max())
        assert gap <= 2.0 ** -5, gap      # the same function up to the stock half chain's roundings (tests/test_gpu_conv_gru.py)
    res = alternate(group, reps)
    f = res["fused_a"]["median_us"]
    aa_fused = abs(f - res["fused_b"]["median_us"])
    P = B * h * w
    flop = 2.0 * P * 128 * (3 * 9 * C_IN + 128)
    nbytes = 2.0 * (P * (2 * 128 + 2 * 320 + 4 * 128 + 128) + 3 * 128 * 9 * C_IN + 4 * 128 * 128)
    r = dict(h=h, w=w, batch=B, reps=reps, **res, aa_spread_fused_us=aa_fused, fused_tflops=flop / f / 1e6,
             fused_share_of_2_5PF=flop / f / PEAK_FLOP_PER_US, fused_bytes_share_of_8TBs=nbytes / HBM_BYTES_PER_US / f,
             acceptance_shape=(h, w, B) in ACCEPTANCE)
    if not only_fused:
        s = res["stock_a"]["median_us"]
        aa_stock = abs(s - res["stock_b"]["median_us"])
        r.update(aa_spread_stock_us=aa_stock, fused_over_stock=f / s, fused_minus_stock_us=f - s,
                 faster=bool(f < s - (aa_stock + aa_fused)), stock_tflops=flop / s / 1e6, max_abs_difference=gap)
    print(json.dumps(r), flush=True)
    del net, inputs, f0
    torch.cuda.empty_cache()
    return r


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--only-fused", action="store_true", help="no stock side: for a kernel trace of the fused launches")
    ap.add_argument("--shape", default=None, help="one shape h x w x E instead of the table, e.g. 48x64x24")
    a = ap.parse_args()
    assert a.reps >= 5
    db._lib.load()
    shapes = [tuple(int(v) for v in a.shape.split("x"))] if a.shape else SHAPES
    res = [one(*shape, a.reps, a.only_fused) for shape in shapes]
    doc = dict(what="ConvGRU(128, 320) on half planes: ConvGRU (four launches, no cat) vs the module's lines on half tensors "
                    "(stock, weights cast beforehand); HIP-event time per call in microseconds, alternating in one process, "
                    "median of `reps`; `faster`: fused median < stock median - the A/A spread of both paths",
               device=torch.cuda.get_device_name(0), library=os.path.basename(db._lib.LIB_PATH), results=res)
    if a.out:
        with open(a.out, "w") as f:
            json.dump(doc, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
