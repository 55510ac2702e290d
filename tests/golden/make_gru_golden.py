"""Writes tests/golden/reference_gru.npz: the reference's own ConvGRU (droid_slam/modules/gru.py, unchanged, loaded the way
tests/reference_programs.py loads the other programs) run on the CPU in float64 with h_planes = 32, i_planes = 64 on maps
5 x 9 and 3 x 3, seeded parameters and operands from tests/gru_ref.py.  The file holds the outputs and the SHA-256 of the
inputs, which tests/test_gru_reference_pin.py regenerates from the seeds.

    python tests/golden/make_gru_golden.py [out.npz]
"""
import hashlib
import importlib
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
for _p in (os.path.dirname(HERE), ROOT, os.path.join(ROOT, "droid-slam_reserch_amd")):     # modules/corr.py imports the package
    if _p not in sys.path:
        sys.path.insert(0, _p)

import gru_ref  # noqa: E402
import reference_programs  # noqa: E402

HIDDEN, INPUTS, SEED = 32, 64, 2024
CASES = [("5x9", (40, 24), 5, 9, 2), ("3x3", (64,), 3, 3, 3)]      # name, channels of the inputs, h, w, B


def inputs_of(case):
    name, splits, h, w, B = case
    params = gru_ref.random_params(SEED, HIDDEN, INPUTS)
    rng = np.random.default_rng(SEED + h * w)
    ops = [rng.normal(0, 1, (B, ch, h, w)) for ch in (HIDDEN,) + splits]      # float64
    return params, ops


def digest(params, ops):
    m = hashlib.sha256()
    for k in gru_ref.LAYERS:
        for a in params[k]:
            m.update(np.ascontiguousarray(a).tobytes())
    for a in ops:
        m.update(np.ascontiguousarray(a).tobytes())
    return m.hexdigest()


def generate():
    import torch
    out = {}
    with reference_programs.loaded():
        gru = importlib.import_module("modules.gru").ConvGRU(HIDDEN, INPUTS).double()
        for case in CASES:
            params, ops = inputs_of(case)
            with torch.no_grad():
                for k in gru_ref.LAYERS:
                    getattr(gru, k).weight.copy_(torch.from_numpy(params[k][0]))
                    getattr(gru, k).bias.copy_(torch.from_numpy(params[k][1]))
                res = gru(*[torch.from_numpy(a) for a in ops])
            out["out_" + case[0]] = res.numpy().copy()
            out["sha_" + case[0]] = np.array(digest(params, ops))
    return out


if __name__ == "__main__":
    path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(HERE, "reference_gru.npz")
    np.savez(path, **generate())
    print("wrote", path, os.path.getsize(path), "bytes")
