#!/usr/bin/env python3
"""The two bodies of the BA linearisation compared at every state a multi-iteration run visits.

    python tools/lin_bits_along_run.py [CONFIG [ITERATIONS]]        # default: cfg3 (the headline graph), 16

The FULL body of ba_lin_kernel has its roundings pinned in source and must leave the bits of the ragged body.  A wrong
fusion in the fp32 part shows on every input.  One in the fp64 part (the point, the Newton steps of 1 / z, ru / rv)
changes about one float in 10^9 evaluations on generic inputs, because the point is rounded to float before anything
reads it: test volume cannot show it.  The first version of the pinned body passed a comparison of a few million words
and differed from the ragged body in ONE word of 37 million along the headline's 16 iterations (profiles/lin_pinned_ab.txt
section 5), which this tool found.

The instrument for that defect is now tests/test_gpu_lin_directed.py: inputs on which an fp64 ulp reaches the floats at
several per cent of the pixels (tests/lin_directed.py; the condition is checked on the CPU by tests/test_lin_directed.py,
the mutants it catches are listed in profiles/lin_directed.txt).  This tool remains the look at real converging states, at
any size: one `ba` iteration at a time through the phase ABI, and before each, droid_test_ba_lin with either body, twice
each (so that a difference that does not repeat is told apart from one that does), `Hpart`, `Q`, `w`, `Ebuf` compared as
32-bit words on the device.  compare_along_run is the loop; the suite runs it on three small graphs as a smoke test.
Run the tool after a compiler change, or after touching lin_fuse / lin_pixel_pinned.  Exit status 1 if any word differs.
Needs a FULL shape (H*W a multiple of 512).
"""
import ctypes
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "droid-slam_reserch_amd")]


NAMES = ("Hpart", "Q", "w", "Ebuf")


def compare_along_run(db, p, iters, motion_only=False, twice=True, log=print):
    """`iters` iterations of `p` through the phase ABI on a workspace of its own; before each, the linearisation of the
    current state by the FULL and by the ragged body (twice each if `twice`), compared word by word on the device.
    Returns per iteration {"diff": words that differ per array, "repeat": words that differ between two runs of the same
    body (FULL, then ragged; empty without `twice`), "size": words per array, "live": non-zero words per array}."""
    import torch
    from droid_backends._args import _stream
    from droid_backends.ba_binding import BAProblemDev, BaBinding
    lib = db._lib.load()
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()
    d = BAProblemDev(poses=t(p.poses), disps=t(p.disps), intrinsics=t(p.intrinsics), disps_sens=t(p.disps_sens),
                     targets=t(p.targets), weights=t(p.weights), eta=t(p.eta), ii=t(p.ii), jj=t(p.jj))
    b = BaBinding(status_mirror=False)
    out = []
    try:
        E, nbuf, H, W, M, t0, t1 = b.begin(d, p.t0, p.t1, motion_only)
        assert (H * W) % 512 == 0, "the product runs the ragged body on this shape: nothing to compare"
        b.buf.zero_()
        dx = torch.zeros((t1 - t0, 6), dtype=torch.float32, device="cuda")
        dz = torch.zeros((max(M, 1), H * W), dtype=torch.float32, device="cuda")
        words = (ctypes.c_size_t * 6)()
        b.prepare(d, (0, nbuf), motion_only)
        for it in range(iters):
            res = []
            for ragged in ((0, 1, 0, 1) if twice else (0, 1)):
                args = (*b._build_args(d), int(motion_only), ragged, b.buf.data_ptr(), b.buf.numel())
                db._lib.check(lib.droid_test_ba_lin(*args, None, None, None, None, words, _stream()), "test_ba_lin (sizes)")
                n4 = [int(n) for n in list(words)[:4]]
                o = [torch.full((max(n, 1),), float("nan"), dtype=torch.float32, device="cuda") for n in n4]
                db._lib.check(lib.droid_test_ba_lin(*args, *[x.data_ptr() if n else None for x, n in zip(o, n4)], None,
                                                    _stream()), "test_ba_lin")
                torch.cuda.synchronize()
                res.append([x[:n].view(torch.int32) for x, n in zip(o, n4)])
            nd = [int((a != c).sum()) for a, c in zip(res[0], res[1])]
            rep = [int((a != c).sum()) for a, c in zip(res[0] + res[1], res[2] + res[3])] if twice else []
            out.append(dict(diff=dict(zip(NAMES, nd)), repeat=rep, size={k: a.numel() for k, a in zip(NAMES, res[0])},
                            live={k: int((a != 0).sum()) for k, a in zip(NAMES, res[1])}))
            log(f"iteration {it}: differing words " + "  ".join(f"{k} {x} of {a.numel()}" for k, x, a in zip(NAMES, nd, res[0])))
            if rep and max(rep):
                log(f"   NOT REPEATABLE: FULL against FULL {rep[:4]}  ragged against ragged {rep[4:]}")
            for k, (a, c) in enumerate(zip(res[0], res[1])):
                for i in torch.nonzero(a != c).flatten()[:8].tolist():
                    log(f"   {NAMES[k]} word {i}: FULL {int(a[i]) & 0xffffffff:#010x} = "
                        f"{float(a[i:i + 1].view(torch.float32)[0]):.9e}  ragged {int(c[i]) & 0xffffffff:#010x}")
            b.build(d, motion_only)
            b.solve_update(d, p.lm, p.ep, motion_only, dx, dz)
            torch.cuda.synchronize()
        st, _ = b.status()
        assert st & 15 == 0, st
    finally:
        b.close()
    return out


def main():
    import droid_backends as db
    from droid_backends import synth
    cfg = sys.argv[1] if len(sys.argv) > 1 else "cfg3"
    iters = int(sys.argv[2]) if len(sys.argv) > 2 else 16
    res = compare_along_run(db, synth.make_config(cfg), iters, log=lambda s: print(s, flush=True))
    worst = max(max(list(r["diff"].values()) + r["repeat"]) for r in res)
    print("all words equal at every visited state" if worst == 0 else f"WORDS DIFFER (most in one array: {worst})")
    return 0 if worst == 0 else 1


if __name__ == "__main__":
    sys.exit(main())
