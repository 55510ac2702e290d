"""CPU-side checks of corr_volume_pyramid's boundary: the symbol is exported and listed, the host-side argument checks
run before any HIP call (so they need no GPU), and the Python entry refuses CPU tensors."""
import ctypes

import pytest
import torch

F16, F32, F64 = 0, 1, 2


def _call(lib, E=2, nbuf=4, ncam=1, C=128, H=16, W=24, levels=4, slot0=0, cap=8, dtype=F16, ptr=None):
    return lib.droid_corr_volume_pyramid(ptr, ptr, ptr, None, E, nbuf, ncam, C, H, W, levels, slot0, cap, dtype, None)


def test_symbol_is_exported_and_listed(backends):
    lib = ctypes.CDLL(backends._lib.LIB_PATH)
    assert hasattr(lib, "droid_corr_volume_pyramid")
    assert "droid_corr_volume_pyramid" in backends._lib.SYMBOLS
    assert callable(backends.corr_volume_pyramid) and "corr_volume_pyramid" in backends.__all__


@pytest.mark.parametrize("kw,word", [
    (dict(dtype=F64), b"dtype"), (dict(dtype=7), b"dtype"), (dict(C=48), b"C"), (dict(C=288), b"C"),
    (dict(slot0=7, E=2, cap=8), b"cap"), (dict(levels=5), b"levels"), (dict(levels=0), b"levels"),
    (dict(H=4), b"map size"), (dict(H=10, W=12), b"map size"), (dict(ncam=3), b"ncam"),
    (dict(), b"null"),   # every size is fine, the pointers are not
])
def test_host_side_refusals_need_no_gpu(backends, kw, word):
    lib = backends._lib.load()
    assert _call(lib, **kw) == -1
    msg = lib.droid_last_error()
    assert b"corr_volume_pyramid" in msg and word in msg, msg


def test_no_edges_is_ok_and_launches_nothing(backends):
    lib = backends._lib.load()
    assert _call(lib, E=0) == 0
    assert _call(lib, E=0, slot0=8, cap=8) == 0


def test_cpu_tensors_are_refused_not_emulated(backends):
    f = torch.zeros((2, 1, 32, 8, 8), dtype=torch.float16)
    ix = torch.zeros(1, dtype=torch.int64)
    with pytest.raises(RuntimeError, match="no CPU path"):
        backends.corr_volume_pyramid(f, ix, ix)
