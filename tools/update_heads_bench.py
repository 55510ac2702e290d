#!/usr/bin/env python
"""Times the output heads of the update operator on the device (UpdateHeads -> droid_update_heads) against the stock
layers, with HIP events, per shape and in one process, ALTERNATING the variants:
  heads:  stock_a, stock_b   under autocast, half inputs on the device: the two F.conv2d(..., padding=1), torch.sigmoid
                             on the second, and the two view -> permute(0,1,3,4,2) -> [..., :2] -> contiguous
                             (droid_slam/droid_net.py:95-106, :130-134; the A/A pair is the noise of this path in this run)
          fused_a, fused_b   heads(hd, hw)                                   (one launch; A/A pair)
  eta:    stock_a, stock_b   F.conv2d(..., padding=1), F.softplus, `.01 *`, view          (droid_net.py:51-54, :72-75)
          fused_a, fused_b   heads.eta(net)                                  (one launch; A/A pair)
Heads: 48x64 with E = 1 (motion filter), 24 (frontend window), 64, 256 and 30x40 with E = 64.  Eta: 48x64 with G = 1, 8,
16 and 30x40 with G = 16.  Per shape `faster`: median(fused_a) < median(stock_a) - the A/A spreads of the two paths; the
baseline is the stock sequence of the same run.  ACCEPT lists the shapes the frontend runs, where `faster` is required;
the others are reported with the same fields.
Algorithmic bytes per pixel: heads fused 2 * (256 + 4) = 520, stock 520 + 8 (sigmoid) + 16 (the two permuted copies) =
544; eta fused 256 + 2 = 258, stock 258 + 4 (softplus) + 4 (`.01 *`) = 266.

    python tools/update_heads_bench.py [--out profiles/update_heads_bench.json] [--reps 30]
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

HEADS_SHAPES = [(48, 64, 1), (48, 64, 24), (48, 64, 64), (48, 64, 256), (30, 40, 64)]
ETA_SHAPES = [(48, 64, 1), (48, 64, 8), (48, 64, 16), (30, 40, 16)]
ACCEPT = {"heads": [(48, 64, 1), (48, 64, 24), (48, 64, 64)], "eta": [(48, 64, 8)]}
BYTES_PX = {"heads": dict(stock=544, fused=520), "eta": dict(stock=266, fused=258)}
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


def conv_params(n, g):
    """nn.Conv2d(128, n, 3)'s default init (fp32, as the network holds them)."""
    k = 1.0 / np.sqrt(1152)
    return ((torch.rand((n, 128, 3, 3), generator=g, device="cuda") * 2 - 1) * k,
            (torch.rand((n,), generator=g, device="cuda") * 2 - 1) * k)


def hidden(B, h, w, g):
    """A ReLU output: half of a rectified normal."""
    return torch.relu(torch.randn((B, 128, h, w), generator=g, device="cuda")).half().contiguous()


def report(path, h, w, B, reps, res, gap):
    aa_stock = abs(res["stock_a"]["median_us"] - res["stock_b"]["median_us"])
    aa_fused = abs(res["fused_a"]["median_us"] - res["fused_b"]["median_us"])
    s, f = res["stock_a"]["median_us"], res["fused_a"]["median_us"]
    px = B * h * w
    r = dict(path=path, h=h, w=w, B=B, reps=reps, **res, aa_spread_stock_us=aa_stock, aa_spread_fused_us=aa_fused,
             fused_over_stock=f / s, fused_minus_stock_us=f - s, faster=bool(f < s - (aa_stock + aa_fused)),
             acceptance_shape=(h, w, B) in ACCEPT[path],
             stock_bytes_per_px=BYTES_PX[path]["stock"], fused_bytes_per_px=BYTES_PX[path]["fused"],
             stock_bytes_share_of_8TBs=BYTES_PX[path]["stock"] * px / HBM_BYTES_PER_US / s,
             fused_bytes_share_of_8TBs=BYTES_PX[path]["fused"] * px / HBM_BYTES_PER_US / f,
             max_abs_difference=gap)
    print(json.dumps(r), flush=True)
    torch.cuda.empty_cache()
    return r


def one_heads(heads, params, h, w, E, reps):
    g = torch.Generator(device="cuda").manual_seed(h * w + E)
    hd, hw = hidden(E, h, w, g), hidden(E, h, w, g)
    (wd, bd), (ww, bw) = params

    def stock():
        with torch.autocast("cuda", dtype=torch.float16):
            d = torch.nn.functional.conv2d(hd, wd, bd, padding=1)
            s = torch.sigmoid(torch.nn.functional.conv2d(hw, ww, bw, padding=1))
        d = d.view(1, E, 2, h, w).permute(0, 1, 3, 4, 2)[..., :2].contiguous()
        s = s.view(1, E, 2, h, w).permute(0, 1, 3, 4, 2)[..., :2].contiguous()
        return d, s

    def fused():
        return heads(hd, hw)

    (d0, s0), (d1, s1) = stock(), fused()
    assert d0.shape == d1.shape == s0.shape == s1.shape == (1, E, h, w, 2) and d1.dtype == s1.dtype == torch.float16
    gap = max(float((d0.float() - d1.float()).abs().max()), float((s0.float() - s1.float()).abs().max()))
    # the same function up to the stock half chain's own roundings, a few half ulps of the largest output
    # (tests/test_gpu_update_heads.py holds the fused one to its bound and prints the stock chain's distance)
    assert gap <= 2.0 ** -8 * max(1.0, float(d0.float().abs().max())), gap
    res = alternate(dict(stock_a=stock, fused_a=fused, stock_b=stock, fused_b=fused), reps)
    return report("heads", h, w, E, reps, res, gap)


def one_eta(heads, params, h, w, G, reps):
    g = torch.Generator(device="cuda").manual_seed(7 * h * w + G)
    net = hidden(G, h, w, g)
    we, be = params

    def stock():
        with torch.autocast("cuda", dtype=torch.float16):
            e = .01 * torch.nn.functional.softplus(torch.nn.functional.conv2d(net, we, be, padding=1))
        return e.view(1, G, h, w)

    def fused():
        return heads.eta(net)

    e0, e1 = stock(), fused()
    assert e0.shape == e1.shape == (1, G, h, w) and e1.dtype == torch.float16
    gap = float((e0.float() - e1.float()).abs().max())
    assert gap <= 2.0 ** -8 * 0.01 * max(1.0, float(e0.float().abs().max()) * 100), gap
    res = alternate(dict(stock_a=stock, fused_a=fused, stock_b=stock, fused_b=fused), reps)
    return report("eta", h, w, G, reps, res, gap)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--reps", type=int, default=30)
    a = ap.parse_args()
    assert a.reps >= 20
    db._lib.load()
    g = torch.Generator(device="cuda").manual_seed(1)
    pd, pw, pe = conv_params(2, g), conv_params(2, g), conv_params(1, g)
    heads = db.UpdateHeads(*pd, *pw, *pe)
    res = [one_heads(heads, (pd, pw), h, w, E, a.reps) for h, w, E in HEADS_SHAPES]
    res += [one_eta(heads, pe, h, w, G, a.reps) for h, w, G in ETA_SHAPES]
    missed = [(r["path"], r["h"], r["w"], r["B"]) for r in res if r["acceptance_shape"] and not r["faster"]]
    doc = dict(what="the last layers of delta + weight (one launch) and of eta (one launch) on the device vs the stock "
                    "layers under autocast on half inputs (heads: two conv2d(padding=1), sigmoid, two permuted copies; "
                    "eta: conv2d, softplus, .01 *, view); HIP-event time per call in microseconds, alternating in one "
                    "process, median of `reps`; `faster`: fused median < stock median - the A/A spread of both paths; "
                    "`acceptance_shape`: a shape the frontend runs, where `faster` is required",
               device=torch.cuda.get_device_name(0), library=os.path.basename(db._lib.LIB_PATH),
               acceptance_missed=missed, results=res)
    if a.out:
        with open(a.out, "w") as f:
            json.dump(doc, f, indent=1)
            f.write("\n")
    print("acceptance missed at:", missed if missed else "no shape")


if __name__ == "__main__":
    main()
