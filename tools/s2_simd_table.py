#!/usr/bin/env python3
"""Which SIMD does wave w of a ba_schur2_kernel workgroup run on?  (profiles/update_launch_ab.txt, part 3)

Needs a DIAGNOSTIC build of the library, never shipped (run with DROID_HIP_LIB=, tools/README.md), in which every wave of
ba_schur2_kernel that has work stores, by lane 0, eight words at g_s2_stamp[8 * ((blockIdx.y * gridDim.x + blockIdx.x) * 4
+ wave)], a __device__ array of 2^15 such records:
  [0] 1 + s_getreg(HW_ID)  [1] s_getreg(XCC_ID)  [2] s_memtime at the start  [3] after the Gram-tile store  [4] at the end
  [5] edges of the slot  [6] blockIdx.x  [7] blockIdx.y
and which exports  int droid_diag_s2_stamps(unsigned* dst, int words, int clear)  (clear != 0: zero the array; else copy
it to the host).  One `ba` iteration of the headline graph is recorded after a warm-up call.
HW_ID (gfx9): wave slot [3:0], SIMD [5:4], CU [11:8], SH [12], SE [15:13].
"""
import collections
import ctypes
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "droid-slam_reserch_amd")]


def main():
    import torch
    import droid_backends as db
    from droid_backends import synth
    lib = db._lib.load()
    fn = lib.droid_diag_s2_stamps
    fn.restype, fn.argtypes = ctypes.c_int, [ctypes.c_void_p, ctypes.c_int, ctypes.c_int]
    p = synth.make_config("cfg3")
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()
    args = [t(p.intrinsics), t(p.disps_sens), t(p.targets), t(p.weights), t(p.eta), t(p.ii), t(p.jj)]
    for k in range(2):
        torch.cuda.synchronize()
        assert fn(None, 0, 1) == 0
        db.ba(t(p.poses), t(p.disps), *args, p.t0, p.t1, 1, p.lm, p.ep, False)
        torch.cuda.synchronize()
    n = 8 << 15
    buf = np.zeros(n, np.uint32)
    assert fn(buf.ctypes.data, n, 0) == 0
    rec = buf.reshape(-1, 8)
    ids = np.flatnonzero(rec[:, 0])
    rec = rec[ids].astype(np.int64)
    wave = ids & 3
    hw = rec[:, 0] - 1
    simd, cu, sh, se, xcc = (hw >> 4) & 3, (hw >> 8) & 15, (hw >> 12) & 1, (hw >> 13) & 7, rec[:, 1] & 15
    where = ((xcc * 8 + se) * 2 + sh) * 16 + cu
    wg = ids >> 2
    print(f"{len(ids)} wave records, {len(set(wg.tolist()))} workgroups, {len(set(where.tolist()))} CUs")

    # 1. the SIMDs of waves 0..3 of one workgroup
    by_wg = collections.defaultdict(dict)
    for i in range(len(ids)):
        by_wg[int(wg[i])][int(wave[i])] = i
    pat = collections.Counter()
    for g, ws in by_wg.items():
        if len(ws) == 4:
            pat[tuple(int(simd[ws[w]]) for w in range(4))] += 1
    print("SIMD of waves (0,1,2,3) of a workgroup: " + ", ".join(f"{k}: {c}" for k, c in pat.most_common()))

    # 2. per wave index: on which SIMD
    tab = np.zeros((4, 4), int)
    for i in range(len(ids)):
        tab[wave[i], simd[i]] += 1
    print("waves by (wave index, SIMD):")
    for w in range(4):
        print(f"  wave {w}: " + "  ".join(f"SIMD{s} {tab[w, s]:5d}" for s in range(4)))

    # 3. workgroups that were on one CU at the same time (their [start, end] intervals overlap): SIMD of their wave 0
    same = diff = 0
    sets = collections.Counter()
    per_cu = collections.defaultdict(list)
    for g, ws in by_wg.items():
        if 0 in ws:
            i = ws[0]
            t0 = min(rec[j, 2] for j in ws.values())
            t1 = max(rec[j, 4] for j in ws.values())
            per_cu[int(where[i])].append((int(t0), int(t1), int(simd[i]), g))
    for c, lst in per_cu.items():
        lst.sort()
        for a in range(len(lst)):
            live = [x for x in lst if x[0] <= lst[a][0] < x[1] and (x[1] - x[0]) < (1 << 30)]
            if len(live) >= 2:
                sets[tuple(sorted(x[2] for x in live))] += 1
            for b in range(a + 1, len(lst)):
                if lst[b][0] < lst[a][1] and (lst[a][1] - lst[a][0]) < (1 << 30):
                    same, diff = same + (lst[a][2] == lst[b][2]), diff + (lst[a][2] != lst[b][2])
    print(f"pairs of workgroups on one CU at one time: wave 0 on the same SIMD {same}, on different SIMDs {diff}")
    print("SIMDs of wave 0 of the workgroups resident on a CU when another one starts there: "
          + ", ".join(f"{k}: {c}" for k, c in sets.most_common(12)))

    # 4. what each SIMD carried: clocks between a wave's start and its Gram-tile store, summed per SIMD index
    busy = np.zeros(4)
    for i in range(len(ids)):
        d = (rec[i, 3] - rec[i, 2]) & 0xFFFFFFFF
        if d < (1 << 30):
            busy[simd[i]] += d
    print("sum of (Gram-tile store - start) clocks by SIMD index, relative to the mean: "
          + "  ".join(f"SIMD{s} {busy[s] / busy.mean():.3f}" for s in range(4)))
    wbusy = np.zeros(4)
    for i in range(len(ids)):
        d = (rec[i, 3] - rec[i, 2]) & 0xFFFFFFFF
        if d < (1 << 30):
            wbusy[wave[i]] += d
    print("the same by wave index: " + "  ".join(f"wave{w} {wbusy[w] / wbusy.mean():.3f}" for w in range(4)))


if __name__ == "__main__":
    main()
