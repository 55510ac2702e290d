#!/usr/bin/env python
"""Times the slot-indexed correlation pyramid with HIP events, per shape and in one process, ALTERNATING the variants:
  1. lookup: corr_pyramid_forward on a contiguous pyramid of 64 edges, timed as TWO variants (`contig_a`, `contig_b`:
     an A/A pair, whose difference of medians is the noise of this run), against corr_pyramid_forward(slots=) on
     capacity buffers of 96 slots that hold the same 64 edges at a shuffled slot list (`slotted`);
     the pair again without the Python wrapper (`raw_*`); and, to say where a distance comes from, the contiguous
     pyramid read through slots 0 .. 63 (`slotted_in_order`: the indirection alone) and through a permutation of them;
  2. the identity path: droid_corr_pyramid_forward of this library (`identity_a`, `identity_b`) against the library of
     the PARENT commit (`parent_identity`, --parent-lib PATH: a build of the parent's csrc/ loaded next to this one),
     all three called without the Python wrapper; without --parent-lib it is not measured;
  3. dropping 8 of 64 edges: `[p[keep] for p in pyramid]` (CorrBlock.__getitem__) against PyramidStore.keep(mask), and a
     replay of 20 frontend-like steps (drop 4-8, add 4-8, look up) on the stock sequence (corr_volume_pyramid +
     torch.cat + boolean indexing + corr_pyramid_forward) and on a PyramidStore, with the peak of
     torch.cuda.max_memory_allocated over what was allocated before the replay.
Gate of 1 and 2 (`within_noise`): the median may exceed its baseline by at most the A/A spread.  3 is reported only.
Half, C = 128, 4 levels, radius 3; 48x64, then 30x40.

    python tools/pyramid_store_bench.py [--out profiles/pyramid_store_bench.json] [--reps 30] [--parent-lib PATH]
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
from droid_backends.pyramid_store import PyramidStore        # noqa: E402

LEVELS, RADIUS, E, CAP, C, NBUF = 4, 3, 64, 96, 128, 64


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
    for _ in range(warm):                       # every shape and every path warmed up
        for fn in group.values():
            fn()
    torch.cuda.synchronize()
    us = {k: [] for k in group}
    for _ in range(reps):                       # alternating, same process
        for k, fn in group.items():
            us[k].append(timed(fn))
    return {k: stats(v) for k, v in us.items()}


def raw_lookup(path):
    """droid_corr_pyramid_forward of a build of the library, called without the Python wrapper: the same host path
    for this commit's library and for the parent's."""
    lib = ctypes.CDLL(path)
    vp, c_int = ctypes.c_void_p, ctypes.c_int
    lib.droid_corr_pyramid_forward.argtypes = [ctypes.POINTER(vp), vp, vp] + [c_int] * 6 + [vp]
    lib.droid_corr_pyramid_forward.restype = c_int

    def run(pyr, coords, out):
        ptrs = (vp * len(pyr))(*[p.data_ptr() for p in pyr])
        B, h, w = pyr[0].shape[:3]
        rc = lib.droid_corr_pyramid_forward(ptrs, coords.data_ptr(), out.data_ptr(), B, h, w, RADIUS, len(pyr),
                                            db._lib.DROID_F16, torch.cuda.current_stream().cuda_stream)
        assert rc == 0, rc

    def run_slots(pyr, slots, coords, out):
        ptrs = (vp * len(pyr))(*[p.data_ptr() for p in pyr])
        cap, h, w = pyr[0].shape[:3]
        rc = lib.droid_corr_pyramid_forward_slots(ptrs, slots.data_ptr(), coords.data_ptr(), out.data_ptr(), slots.shape[0],
                                                  cap, h, w, RADIUS, len(pyr), db._lib.DROID_F16,
                                                  torch.cuda.current_stream().cuda_stream)
        assert rc == 0, rc
    if hasattr(lib, "droid_corr_pyramid_forward_slots"):
        lib.droid_corr_pyramid_forward_slots.argtypes = ([ctypes.POINTER(vp), vp, vp, vp, c_int, ctypes.c_int64]
                                                         + [c_int] * 5 + [vp])
        lib.droid_corr_pyramid_forward_slots.restype = c_int
        run.slots = run_slots
    return run


def edges(g, n):
    ii = torch.randint(0, NBUF, (n,), generator=g, device="cuda")
    jj = (ii + 1 + torch.randint(0, NBUF - 1, (n,), generator=g, device="cuda")) % NBUF
    return ii, jj


def coords_for(g, n, h, w):
    """[n,2,h,w]: every query within a few pixels of its own position, as the frontend's reprojections are."""
    gy, gx = torch.meshgrid(torch.arange(h, device="cuda", dtype=torch.float32),
                            torch.arange(w, device="cuda", dtype=torch.float32), indexing="ij")
    return (torch.stack([gx, gy])[None] + 2.0 * torch.randn((n, 2, h, w), generator=g, device="cuda")).contiguous()


def replay_plan(seed, steps=20):
    rng = np.random.default_rng(seed)
    plan, n = [], E
    for _ in range(steps):
        drop = int(rng.integers(4, 9))
        mask = np.ones(n, bool)
        mask[rng.choice(n, size=drop, replace=False)] = False
        add = int(rng.integers(4, 9))
        n = n - drop + add
        plan.append((torch.from_numpy(mask).cuda(), add))
    return plan


def replay_stock(fmaps, ii0, jj0, plan, new_edges, coords):
    """coords [1, n_max, h, w, 2], as CorrBlock.__call__ takes them."""
    pyr = db.corr_volume_pyramid(fmaps, ii0, jj0, LEVELS)
    for (mask, add), (ii, jj) in zip(plan, new_edges):
        pyr = [p[mask] for p in pyr]
        new = db.corr_volume_pyramid(fmaps, ii, jj, LEVELS)
        pyr = [torch.cat([a, b], 0) for a, b in zip(pyr, new)]
        n = pyr[0].shape[0]
        c = coords[:, :n].permute(0, 1, 4, 2, 3).contiguous().view(n, 2, *coords.shape[2:4])
        db.corr_pyramid_forward(pyr, c, RADIUS)


def replay_store(fmaps, ii0, jj0, plan, new_edges, coords):
    store = PyramidStore(fmaps, CAP, LEVELS, RADIUS)
    store.add(ii0, jj0)
    for (mask, add), (ii, jj) in zip(plan, new_edges):
        store.keep(mask)
        store.add(ii, jj)
        store(coords[:, :len(store)])
    return store.grows


def with_peak(fn):
    torch.cuda.synchronize()
    base = torch.cuda.memory_allocated()
    torch.cuda.reset_peak_memory_stats()
    us = timed(fn)
    return us, torch.cuda.max_memory_allocated() - base


def one(h, w, reps, parent):
    g = torch.Generator(device="cuda").manual_seed(h * w)
    fmaps = torch.randn((NBUF, 1, C, h, w), generator=g, device="cuda", dtype=torch.float16)
    ii, jj = edges(g, E)
    coords = coords_for(g, 2 * CAP, h, w)
    c64 = coords[:E].contiguous()
    coords5 = coords.permute(0, 2, 3, 1).contiguous()[None]                      # [1, n, h, w, 2]
    slots = torch.randperm(CAP, generator=g, device="cuda")[:E].contiguous()      # shuffled, 64 of 96
    cap = [torch.zeros((CAP, h, w, h >> l, w >> l), device="cuda", dtype=torch.float16) for l in range(LEVELS)]
    db.corr_volume_pyramid(fmaps, ii, jj, LEVELS, out=cap, slots=slots)
    contig = [p[slots].contiguous() for p in cap]                                # the same content, in edge order
    want, = db.corr_pyramid_forward(contig, c64, RADIUS)
    got, = db.corr_pyramid_forward(cap, c64, RADIUS, slots=slots)
    assert torch.equal(want.view(torch.int16), got.view(torch.int16)), "slotted lookup differs from the contiguous one"

    # ---- 1: lookups as a caller makes them.  The two buffers take turns, so that neither finds more of itself in the
    # 256 MB memory-side cache than the other (the 30x40 pyramid of 64 edges is 245 MB).
    res = alternate(dict(contig_a=lambda: db.corr_pyramid_forward(contig, c64, RADIUS),
                         slotted=lambda: db.corr_pyramid_forward(cap, c64, RADIUS, slots=slots),
                         contig_b=lambda: db.corr_pyramid_forward(contig, c64, RADIUS),
                         slotted_b=lambda: db.corr_pyramid_forward(cap, c64, RADIUS, slots=slots)), reps)
    aa = abs(res["contig_a"]["median_us"] - res["contig_b"]["median_us"])
    res["aa_spread_us"] = aa
    res["slotted_minus_contig_us"] = res["slotted"]["median_us"] - res["contig_a"]["median_us"]
    res["slotted_within_noise"] = bool(res["slotted_minus_contig_us"] <= aa)
    # where a distance comes from, all three on the CONTIGUOUS pyramid: `slotted_in_order` reads it through slots
    # 0 .. 63 (the addresses of `contig_c`: the indirection alone, kernel and wrapper), `slotted_permuted` through a
    # permutation of 0 .. 63 (the same bytes in another order)
    in_order = torch.arange(E, device="cuda")
    permuted = torch.randperm(E, generator=g, device="cuda")
    att = alternate(dict(contig_c=lambda: db.corr_pyramid_forward(contig, c64, RADIUS),
                         slotted_in_order=lambda: db.corr_pyramid_forward(contig, c64, RADIUS, slots=in_order),
                         slotted_permuted=lambda: db.corr_pyramid_forward(contig, c64, RADIUS, slots=permuted)), reps)
    res.update(att, slotted_in_order_minus_contig_us=att["slotted_in_order"]["median_us"] - att["contig_c"]["median_us"],
               slotted_permuted_minus_contig_us=att["slotted_permuted"]["median_us"] - att["contig_c"]["median_us"])
    # pair 1 again without the Python wrapper: what the kernels and the C entry point alone add
    this = raw_lookup(db._lib.LIB_PATH)
    out_r = torch.empty_like(want)
    raw = alternate(dict(raw_contig_a=lambda: this(contig, c64, out_r),
                         raw_slotted=lambda: this.slots(cap, slots, c64, out_r),
                         raw_contig_b=lambda: this(contig, c64, out_r),
                         raw_slotted_b=lambda: this.slots(cap, slots, c64, out_r)), reps)
    res.update(raw, raw_aa_spread_us=abs(raw["raw_contig_a"]["median_us"] - raw["raw_contig_b"]["median_us"]),
               raw_slotted_minus_contig_us=raw["raw_slotted"]["median_us"] - raw["raw_contig_a"]["median_us"])

    # ---- 2: the identity path of this commit's library against the parent's, both without the Python wrapper
    if parent:
        out_p = torch.empty_like(want)
        parent(contig, c64, out_p)
        assert torch.equal(want.view(torch.int16), out_p.view(torch.int16)), "parent library computes other bits"
        raw = alternate(dict(identity_a=lambda: this(contig, c64, out_p), parent_identity=lambda: parent(contig, c64, out_p),
                             identity_b=lambda: this(contig, c64, out_p)), reps)
        aa_raw = abs(raw["identity_a"]["median_us"] - raw["identity_b"]["median_us"])
        res.update(raw, identity_aa_spread_us=aa_raw,
                   identity_minus_parent_us=raw["identity_a"]["median_us"] - raw["parent_identity"]["median_us"])
        res["identity_within_noise"] = bool(res["identity_minus_parent_us"] <= aa_raw)
    else:
        res["identity_minus_parent_us"] = res["identity_within_noise"] = None     # not measured

    # ---- 3a: drop 8 of 64
    keep = torch.ones(E, dtype=torch.bool, device="cuda")
    keep[torch.randperm(E, generator=g, device="cuda")[:8]] = False
    gone = (~keep).nonzero().flatten()
    store = PyramidStore(fmaps, CAP, LEVELS, RADIUS)
    store.add(ii, jj)
    stock_us, store_us = [], []
    for rep in range(reps + 3):
        t_stock = timed(lambda: [p[keep] for p in contig])
        t_store = timed(lambda: store.keep(keep))
        store.add(ii[gone], jj[gone])                     # the 8 edges come back, untimed
        if rep >= 3:
            stock_us.append(t_stock)
            store_us.append(t_store)
    res["drop8_stock_index"] = stats(stock_us)
    res["drop8_store_keep"] = stats(store_us)
    res["drop8_bytes_copied_by_stock"] = 2 * sum(2 * (E - 8) * h * w * (h >> l) * (w >> l) for l in range(LEVELS))
    del store, cap, contig, want, got
    torch.cuda.empty_cache()

    # ---- 3b: 20 frontend-like steps, both ways
    plan = replay_plan(h * w)
    new_edges = [edges(g, add) for _, add in plan]
    runs = dict(replay_stock=lambda: replay_stock(fmaps, ii, jj, plan, new_edges, coords5),
                replay_store=lambda: replay_store(fmaps, ii, jj, plan, new_edges, coords5))
    us, peak = {k: [] for k in runs}, {k: 0 for k in runs}
    for rep in range(2 + 7):
        for k, fn in runs.items():
            t, p = with_peak(fn)
            if rep >= 2:
                us[k].append(t)
                peak[k] = max(peak[k], p)
    for k in runs:
        res[k] = dict(**stats(us[k]), peak_bytes_over_baseline=int(peak[k]))
    r = dict(h=h, w=w, C=C, E=E, cap=CAP, reps=reps, replay_steps=len(plan), **res)
    print(json.dumps(r))
    return r


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--parent-lib", default=None)
    a = ap.parse_args()
    assert a.reps >= 20
    db._lib.load()
    parent = raw_lookup(a.parent_lib) if a.parent_lib else None
    res = [one(48, 64, a.reps, parent), one(30, 40, a.reps, parent)]
    doc = dict(what="slot-indexed half correlation pyramid (4 levels, C = 128, 64 edges in 96 slots): HIP-event time per "
                    "call in microseconds, alternating in one process; lookup through a shuffled slot list vs the "
                    "contiguous lookup (A/A pair = noise), this library's contiguous lookup vs the parent commit's, "
                    "dropping 8 of 64 edges by boolean indexing vs PyramidStore.keep, and a 20-step replay both ways",
               device=torch.cuda.get_device_name(0), parent_lib=bool(a.parent_lib), results=res)
    if a.out:
        with open(a.out, "w") as f:
            json.dump(doc, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
