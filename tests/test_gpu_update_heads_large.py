"""droid_update_heads on a hidden tensor beyond 2^32 elements (include/droid_heads_hip.h: all offsets are 64-bit), with
the conventions of tests/test_gpu_large_offsets.py: batch position changes addresses, not arithmetic, so on the named
batch elements the large call must return, bit for bit, what the operator returns on a small tensor that holds copies of
only those elements.  Every byte of x that is no named element holds 0x7B; fills go in pieces of at most 2^30 bytes; one
large buffer lives at a time."""
import pytest
import torch

import large_offset_cases as lo
import update_heads_ref as uh
from test_gpu_large_offsets import _fill, _same

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
H, W, C = 48, 64, 128
PER = C * H * W          # 393 216 elements per batch element
B = 10925                # 4 295 884 800 elements, 8 591 769 600 bytes
# 2^31 = 5461 * PER + 131 072 lies inside element 5461, 2^32 = 10922 * PER + 262 144 inside element 10922: the elements on
# either side of both marks, the two that hold them, the first and the last
NAMED = (0, 5460, 5461, 5462, 10921, 10922, 10923, 10924)


def test_the_named_elements_lie_where_claimed():
    assert 5461 * PER < 1 << 31 < 5462 * PER and 10922 * PER < 1 << 32 < 10923 * PER
    assert B * PER > 1 << 32 and NAMED[-1] == B - 1 and B <= 65535
    assert B * PER * 2 + B * H * W * 2 + (1 << 30) <= lo.LIMIT


def test_one_head_beyond_2_to_the_32_elements(backends):
    torch.cuda.synchronize()
    torch.cuda.empty_cache()
    need = B * PER * 2 + B * H * W * 2 + (1 << 28)
    free, total = torch.cuda.mem_get_info()
    if need > free:
        pytest.skip(f"update_heads large: needs {need} bytes, {free} of {total} are free: {need - free} bytes missing")
    w, b = uh.params(uh.SOFTPLUS_CENTI, 40)
    to = lambda a: torch.from_numpy(a).to(DEV)
    heads = backends.UpdateHeads(*(to(a) for a in uh.params(uh.IDENTITY, 40) + uh.params(uh.SIGMOID, 40)), to(w), to(b))
    small = torch.stack([to(uh.hidden(1, H, W, 50 + k)[0]) for k in range(len(NAMED))]).contiguous()
    want = heads.eta(small)
    assert want.shape == (1, len(NAMED), H, W) and bool(torch.isfinite(want).all()) and float(want.float().max()) > 0
    x = torch.empty((B, C, H, W), dtype=torch.float16, device=DEV)
    assert x.numel() > 1 << 32
    _fill(x)
    for k, e in enumerate(NAMED):
        x[e].copy_(small[k])
    got = heads.eta(x)
    torch.cuda.synchronize()
    assert got.shape == (1, B, H, W)
    for k, e in enumerate(NAMED):
        assert _same(got[0, e], want[0, k]), e
    del x, got
    torch.cuda.empty_cache()
