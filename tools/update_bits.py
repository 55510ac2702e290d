#!/usr/bin/env python3
"""Bit check of the update stage between builds of the library: one iteration of `droid_backends.ba` from the same
inputs, `poses`, `disps`, `dx_out` and `dz_out` compared as uint32.

    python tools/update_bits.py parent.so new.so [more.so ...]     # the first library is the reference, run twice

Each library runs in a process of its own (DROID_HIP_LIB, tools/README.md).  The reference runs a second time at the
end: the order of the build phase's fp64 atomics varies from run to run, so its own two runs say how many words a pair
of runs of ONE library may differ in.  Graphs: the headline (256 kf / 2000 e / 48x64), 8 kf / 32 e / 24x32,
36 kf / 1200 e / 16x32 (dense slots), 3 kf / 4 e / 5x7 and a motion-only graph.
"""
import os
import subprocess
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "droid-slam_reserch_amd")]


def graphs(synth):
    def motion():
        p = synth.make_ba_problem(N=10, E=36, H=32, W=48, seed=7)
        keep = (p.ii < 6) & (p.jj >= 6)
        p.ii, p.jj, p.targets, p.weights = p.ii[keep], p.jj[keep], p.targets[keep], p.weights[keep]
        p.t0, p.t1 = 6, 10
        return p
    return [("headline", synth.make_config("cfg3"), False),
            ("8kf_32e_24x32", synth.make_ba_problem(N=8, E=32, H=24, W=32, seed=2), False),
            ("36kf_1200e_16x32", synth.make_ba_problem(N=36, E=1200, H=16, W=32, seed=77, lm=1e-4, ep=0.1), False),
            ("3kf_4e_5x7", synth.make_ba_problem(N=3, E=4, H=5, W=7, seed=11), False),
            ("motion_only", motion(), True)]


def dump(path):
    import torch
    import droid_backends as db
    from droid_backends import synth
    out = {}
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()
    for name, p, mo in graphs(synth):
        poses, disps = t(p.poses), t(p.disps)
        dx, dz = db.ba(poses, disps, t(p.intrinsics), t(p.disps_sens), t(p.targets), t(p.weights), t(p.eta), t(p.ii),
                       t(p.jj), p.t0, p.t1, 1, p.lm, p.ep, mo)
        torch.cuda.synchronize()
        st, _ = db.ba_status()
        assert st & 15 == 0, (name, st)
        for k, a in (("poses", poses), ("disps", disps), ("dx", dx), ("dz", dz)):
            out[f"{name}.{k}"] = a.cpu().numpy()
    np.savez(path, **out)


def main():
    if sys.argv[1] == "--dump":
        return dump(sys.argv[2])
    libs = sys.argv[1:]
    runs = libs + [libs[0]]
    with tempfile.TemporaryDirectory() as tmp:
        files = []
        for k, lib in enumerate(runs):
            f = os.path.join(tmp, f"run{k}.npz")
            env = dict(os.environ, DROID_HIP_LIB=os.path.abspath(lib))
            subprocess.run([sys.executable, os.path.abspath(__file__), "--dump", f], env=env, check=True, timeout=300)
            files.append(np.load(f))
        ref = files[0]
        worst = 0
        for k in range(1, len(runs)):
            tag = "reference, second run" if k == len(runs) - 1 else runs[k]
            print(f"{tag} against {runs[0]}: differing 32-bit words")
            for key in ref.files:
                a, b = ref[key], files[k][key]
                assert a.shape == b.shape, key
                nd = int((np.ascontiguousarray(a).view(np.uint32) != np.ascontiguousarray(b).view(np.uint32)).sum())
                print(f"  {key:28s} {nd:8d} of {a.size}")
                if k < len(runs) - 1:
                    worst = max(worst, nd)
        print("all words equal" if worst == 0 else f"WORDS DIFFER (most in one array: {worst})")
        return 0 if worst == 0 else 1


if __name__ == "__main__":
    sys.exit(main())
