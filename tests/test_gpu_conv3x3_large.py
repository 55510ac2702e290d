"""droid_conv3x3 with batch strides beyond 2^32 elements (include/droid_conv3x3_hip.h: the addressing is 64-bit).  Two
8 x 8 images of a 128 -> 128 layer whose second image lies more than 8 GiB behind the first, in x and in y; about 17 GB
of device memory, none of it initialised beyond the two images."""
import numpy as np
import pytest
import torch

import conv3x3_ref as ref

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def test_batch_strides_beyond_2_to_32_elements(backends):
    c, h, w = 128, 8, 8
    x, wt, b = ref.operands(51, c, c, h, w, 2)
    x = torch.from_numpy(x).to(DEV)
    conv = backends.Conv3x3(torch.from_numpy(wt).to(DEV), torch.from_numpy(b).to(DEV), relu=True)
    base = conv(x)
    xs, ys = 2 ** 32 + 4096, 2 ** 32 + 8 * 4099          # y's is no multiple of the plane either
    xbuf = torch.empty(xs + c * h * w + 64, dtype=torch.float16, device=DEV)
    ybuf = torch.empty(ys + c * h * w + 64, dtype=torch.float16, device=DEV)
    xv = xbuf.as_strided((2, c, h, w), (xs, h * w, w, 1), 64)
    yv = ybuf.as_strided((2, c, h, w), (ys, h * w, w, 1), 8)
    xv.copy_(x)
    yv.fill_(float("nan"))
    assert conv(xv, out=yv) is yv
    torch.cuda.synchronize()
    assert torch.equal(yv.contiguous().view(torch.int16), base.view(torch.int16))
    assert np.isfinite(base.float().cpu().numpy()).all()     # so the NaN fill of y was overwritten everywhere
