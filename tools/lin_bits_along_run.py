#!/usr/bin/env python3
"""The two bodies of the BA linearisation compared at every state a multi-iteration run visits.

    python tools/lin_bits_along_run.py [CONFIG [ITERATIONS]]        # default: cfg3 (the headline graph), 16

tests/test_gpu_lin_pinned.py compares the FULL body of ba_lin_kernel (roundings pinned in source) with the ragged body
on a few million words.  A wrong fusion in the fp64 part of the pinned arithmetic changes about one float in 10^9
evaluations (the point is rounded to float before anything reads it), which that volume does not show: the first version
of the pinned body passed it and differed from the ragged body in ONE word of 37 million along the headline's 16
iterations (profiles/lin_pinned_ab.txt section 5).  This tool is that comparison: one `ba` iteration at a time through the
phase ABI, and before each, droid_test_ba_lin with either body, twice each (so that a difference that does not repeat is told
apart from one that does), `Hpart`, `Q`, `w`, `Ebuf` as uint32.  Run it after a compiler change, or after touching
lin_fuse / lin_pixel_pinned.  Exit status 1 if any word differs.  Needs a FULL shape (H*W a multiple of 512).
"""
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
    from droid_backends._args import _stream
    from droid_backends.ba_binding import BAProblemDev, BaBinding
    cfg = sys.argv[1] if len(sys.argv) > 1 else "cfg3"
    iters = int(sys.argv[2]) if len(sys.argv) > 2 else 16
    lib = db._lib.load()
    p = synth.make_config(cfg)
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()
    d = BAProblemDev(poses=t(p.poses), disps=t(p.disps), intrinsics=t(p.intrinsics), disps_sens=t(p.disps_sens),
                     targets=t(p.targets), weights=t(p.weights), eta=t(p.eta), ii=t(p.ii), jj=t(p.jj))
    b = BaBinding(status_mirror=False)
    E, nbuf, H, W, M, t0, t1 = b.begin(d, p.t0, p.t1, False)
    assert (H * W) % 512 == 0, "the product runs the ragged body on this shape: nothing to compare"
    b.buf.zero_()
    dx = torch.zeros((t1 - t0, 6), dtype=torch.float32, device="cuda")
    dz = torch.zeros((M, H * W), dtype=torch.float32, device="cuda")
    words = (ctypes.c_size_t * 6)()
    names = ("Hpart", "Q", "w", "Ebuf")
    b.prepare(d, (0, nbuf), False)
    worst = 0
    for it in range(iters):
        res = []
        for ragged in (0, 1, 0, 1):
            args = (*b._build_args(d), 0, ragged, b.buf.data_ptr(), b.buf.numel())
            db._lib.check(lib.droid_test_ba_lin(*args, None, None, None, None, words, _stream()), "test_ba_lin (sizes)")
            n4 = [int(n) for n in list(words)[:4]]
            out = [torch.full((max(n, 1),), float("nan"), dtype=torch.float32, device="cuda") for n in n4]
            db._lib.check(lib.droid_test_ba_lin(*args, *[o.data_ptr() if n else None for o, n in zip(out, n4)], None, _stream()),
                          "test_ba_lin")
            torch.cuda.synchronize()
            res.append([o[:n].view(torch.int32) for o, n in zip(out, n4)])
        nd = [int((a != c).sum()) for a, c in zip(res[0], res[1])]
        rep = [int((a != c).sum()) for a, c in zip(res[0] + res[1], res[2] + res[3])]
        worst = max(worst, max(nd), max(rep))
        print(f"iteration {it}: differing words " + "  ".join(f"{k} {x} of {a.numel()}" for k, x, a in zip(names, nd, res[0])),
              flush=True)
        if max(rep):
            print("   NOT REPEATABLE: FULL against FULL", rep[:4], " ragged against ragged", rep[4:])
        for k, (a, c) in enumerate(zip(res[0], res[1])):
            for i in torch.nonzero(a != c).flatten()[:8].tolist():
                print(f"   {names[k]} word {i}: FULL {int(a[i]) & 0xffffffff:#010x} = {float(a[i:i + 1].view(torch.float32)[0]):.9e}"
                      f"  ragged {int(c[i]) & 0xffffffff:#010x}")
        b.build(d, False)
        b.solve_update(d, p.lm, p.ep, False, dx, dz)
        torch.cuda.synchronize()
    b.close()
    print("all words equal at every visited state" if worst == 0 else f"WORDS DIFFER (most in one array: {worst})")
    return 0 if worst == 0 else 1


if __name__ == "__main__":
    sys.exit(main())
