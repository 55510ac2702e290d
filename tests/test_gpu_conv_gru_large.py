"""droid_conv_gru with batch strides beyond 2^32 elements (include/droid_gru_hip.h: the addressing is 64-bit).  Two 5 x 9
images whose second one lies more than 8 GiB behind the first, in net and in out; about 17 GB of device memory, none of
it initialised beyond the two images."""
import numpy as np
import pytest
import torch

import gru_ref as ref

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def test_batch_strides_of_net_and_out_beyond_2_to_32_elements(backends):
    h, w, B = 5, 9, 2
    t = lambda a: torch.from_numpy(a).to(DEV)
    gru = backends.ConvGRU(**{k: (t(wt), t(b)) for k, (wt, b) in ref.random_params(91, 128, 320).items()})
    net, inp, corr, flow = (t(a) for a in ref.operands(92, ref.SPLITS[0], h, w, B))
    base = gru(net, inp, corr, flow)
    ns, os_ = 2 ** 32 + 4096, 2 ** 32 + 8 * 4099          # out's is no multiple of the plane either
    nbuf = torch.empty(ns + 128 * h * w + 64, dtype=torch.float16, device=DEV)
    obuf = torch.empty(os_ + 128 * h * w + 64, dtype=torch.float16, device=DEV)
    nv = nbuf.as_strided((B, 128, h, w), (ns, h * w, w, 1), 64)
    ov = obuf.as_strided((B, 128, h, w), (os_, h * w, w, 1), 8)
    nv.copy_(net)
    ov.fill_(float("nan"))
    assert gru(nv, inp, corr, flow, out=ov) is ov
    torch.cuda.synchronize()
    assert torch.equal(ov.contiguous().view(torch.int16), base.view(torch.int16))
    assert np.isfinite(base.float().cpu().numpy()).all()     # so the NaN fill of out was overwritten everywhere
    assert gru(nv, inp, corr, flow, out=nv) is nv            # in place, across the same stride
    torch.cuda.synchronize()
    assert torch.equal(nv.contiguous().view(torch.int16), base.view(torch.int16))
