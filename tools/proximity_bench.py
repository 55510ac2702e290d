#!/usr/bin/env python
"""Times the proximity-edge selection (droid_proximity_edges) with HIP events, for the global backend's call
(t0 = t1 = 0, rad 2, nms 3, thresh 22, max_factors 16 t; t = 256, 512) and the frontend's (t0 = t - 5,
t1 = max(t - 25, 0), rad 2, nms 1, thresh 16, max_factors 48), on the frame distances of a synthetic trajectory.
Next to it: the wall time of the test suite's HOST RESTATEMENT (tests/proximity_ref.py) on the same matrix copied to
the CPU.  That restatement walks a numpy array; the reference's loop reads every candidate from the device with
.item(), which is far dearer, so the ratio printed here UNDERSTATES the gain over the reference.

    python tools/proximity_bench.py [--out profiles/proximity_bench.json] [--reps 50]
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (os.path.join(ROOT, "tests"), os.path.join(ROOT, "droid-slam_reserch_amd")):
    sys.path.insert(0, p)

import droid_backends as db          # noqa: E402
import proximity_ref as pr           # noqa: E402
from droid_backends import synth     # noqa: E402


def one(name, dist, t, t0, t1, rad, nms, thresh, mf, reps):
    lib = db._lib.load()
    cap = db.proximity_edge_bound(t, t0, t1, rad, mf, False)
    ws = torch.empty(lib.droid_proximity_workspace_bytes(t, t0, t1, 0, cap), dtype=torch.uint8, device="cuda")
    out = torch.empty((cap, 2), dtype=torch.int64, device="cuda")
    cnt = torch.zeros(1, dtype=torch.int32, device="cuda")
    s = torch.cuda.current_stream().cuda_stream

    def call():
        rc = lib.droid_proximity_edges(dist.data_ptr(), dist.stride(0), 1, t, t0, t1, rad, nms, thresh, mf, 0, None, None, 0,
                                       None, None, 0, out.data_ptr(), cap, cnt.data_ptr(), ws.data_ptr(), ws.numel(), s)
        assert rc == 0, lib.droid_last_error()

    for _ in range(5):
        call()
    torch.cuda.synchronize()
    ms = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        call()
        b.record()
        b.synchronize()
        ms.append(a.elapsed_time(b))
    n = int(cnt.item())
    host = dist.cpu().numpy()
    st, hs = {}, []
    for _ in range(3):
        t_0 = time.perf_counter()
        want = pr.proximity_edges(host, t, t0, t1, rad, nms, thresh, mf, False, [], stats=st)
        hs.append((time.perf_counter() - t_0) * 1e3)
    same = n == len(want) and bool(np.array_equal(out[:n].cpu().numpy(), want))
    r = dict(case=name, t=t, t0=t0, t1=t1, rad=rad, nms=nms, thresh=thresh, max_factors=mf, edges=n,
             forced=st["forced"], accepted_pairs=st["accepted"], candidates_under_thresh=st["under"],
             device_ms_median=float(np.median(ms)), device_ms_min=float(np.min(ms)),
             host_restatement_ms_min=float(np.min(hs)), equal_to_restatement=same)
    print(json.dumps(r))
    return r


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--reps", type=int, default=50)
    a = ap.parse_args()
    res = []
    for t in (256, 512):
        p = synth.make_ba_problem(N=t, E=2 * t, H=24, W=32, seed=3)
        dev = lambda x: torch.from_numpy(np.ascontiguousarray(x)).cuda()
        poses, disps, intr = dev(p.poses), dev(p.disps), dev(p.intrinsics)
        dist = db.frame_distance_matrix(poses, disps, intr, t, 0.25, bidirectional=False)
        res.append(one(f"backend t={t}", dist, t, 0, 0, 2, 3, 22.0, 16 * t, a.reps))
        res.append(one(f"frontend t={t}", dist, t, t - 5, max(t - 25, 0), 2, 1, 16.0, 48, a.reps))
    doc = dict(what="droid_proximity_edges, HIP-event time of the 4 stream operations (no count read-back, distance "
                    "matrix given) vs wall time of the numpy host restatement of tests/proximity_ref.py on the same "
                    "matrix; the restatement is much cheaper than the reference's per-candidate device reads, so the "
                    "ratio understates the gain", device=torch.cuda.get_device_name(0), results=res)
    if a.out:
        with open(a.out, "w") as f:
            json.dump(doc, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
