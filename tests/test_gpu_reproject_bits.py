"""droid_reproject_motion keeps the bits it had before its per-pixel body moved into csrc/reproject_pixel.hpp with every
rounding written out: tests/golden/reproject_motion_bits.npz holds the inputs of scene (11, 13, 3) of
tests/motion_encode_ref.py (per-frame anisotropic intrinsics, a stereo edge, an edge outside the buffer) and the coords,
valid and motn words the build of the commit before that move wrote for them on the MI355X.  tests/test_gpu_geom.py holds
the operator to the oracle with a tolerance; this holds it to itself with none."""
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "reproject_motion_bits.npz")


def test_reproject_motion_writes_the_recorded_bits(backends):
    g = np.load(GOLDEN)
    t = lambda k: torch.from_numpy(g[k]).cuda()
    coords, valid, motn = backends.reproject(t("poses"), t("disps"), t("intrinsics"), t("ii"), t("jj"), t("target"))
    torch.cuda.synchronize()
    assert np.abs(g["motn"]).max() > 1 and (g["valid"] == 1).any() and not g["coords"][2].any()   # edge 2 is outside the buffer
    for got, key in ((coords[0], "coords"), (valid[0, ..., 0], "valid"), (motn[0], "motn")):
        want = g[key]
        assert got.shape == want.shape
        assert np.array_equal(got.cpu().numpy().view(np.uint32), want.view(np.uint32)), key
