"""CPU-side checks of the slot-indexed pyramid entry points: the symbols are exported and listed, every host-side
argument check answers DROID_E_ARG with a message before any HIP call (so none of this needs a GPU), and the Python
keyword refuses what the contract excludes."""
import ctypes

import pytest
import torch

F16, F32, F64 = 0, 1, 2
DROID_OK, DROID_E_ARG = 0, -1
NEW = ("droid_corr_pyramid_forward_slots", "droid_corr_volume_pyramid_slots")


def _lookup(lib, B=2, cap=8, H1=16, W1=24, radius=3, levels=4, dtype=F16, ptr=None, slots=None):
    vols = (ctypes.c_void_p * 8)(*([ptr] * 8))
    return lib.droid_corr_pyramid_forward_slots(vols, slots, ptr, ptr, B, cap, H1, W1, radius, levels, dtype, None)


def _build(lib, E=2, nbuf=4, ncam=1, C=128, H=16, W=24, levels=4, cap=8, dtype=F16, ptr=None, slots=None):
    outs = (ctypes.c_void_p * 4)(*([ptr] * 4))
    return lib.droid_corr_volume_pyramid_slots(ptr, ptr, ptr, outs, slots, E, nbuf, ncam, C, H, W, levels, cap, dtype, None)


def test_symbols_are_exported_and_listed(backends):
    lib = ctypes.CDLL(backends._lib.LIB_PATH)
    for name in NEW:
        assert hasattr(lib, name), name
        assert name in backends._lib.SYMBOLS, name
    assert backends._lib.load().droid_abi_version() == 1   # adding symbols keeps the ABI version


def test_python_mirror_lists_the_slot_store(backends):
    from droid_backends import pyramid_store
    assert callable(pyramid_store.SlotTable) and callable(pyramid_store.PyramidStore)
    import inspect
    assert "slots" in inspect.signature(backends.corr_pyramid_forward).parameters
    assert "slots" in inspect.signature(backends.corr_volume_pyramid).parameters


# a non-null value for pointers the host never dereferences: the checks under test return before any HIP call
FAKE = 0x1000


@pytest.mark.parametrize("kw,word", [
    (dict(ptr=FAKE, slots=None), b"null slots"),
    (dict(ptr=FAKE, slots=FAKE, cap=0), b"cap"), (dict(ptr=FAKE, slots=FAKE, cap=-3), b"cap"),
    (dict(ptr=FAKE, slots=FAKE, dtype=3), b"dtype"), (dict(ptr=FAKE, slots=FAKE, dtype=-1), b"dtype"),
    (dict(ptr=FAKE, slots=FAKE, radius=2), b"radius"), (dict(ptr=FAKE, slots=FAKE, radius=5), b"radius"),
    (dict(ptr=FAKE, slots=FAKE, levels=0), b"levels"), (dict(ptr=FAKE, slots=FAKE, levels=9), b"levels"),
    (dict(ptr=FAKE, slots=FAKE, levels=6), b"levels"),   # 16 >> 5 == 0: no pixel left at the last level
    (dict(ptr=FAKE, slots=FAKE, B=-1), b"shape"), (dict(ptr=FAKE, slots=FAKE, H1=0), b"shape"),
    (dict(ptr=FAKE, slots=FAKE, B=65536), b"shape"),
    (dict(ptr=None, slots=FAKE), b"null pointer"),
])
def test_lookup_refusals_need_no_gpu(backends, kw, word):
    lib = backends._lib.load()
    assert _lookup(lib, **kw) == DROID_E_ARG
    msg = lib.droid_last_error()
    assert b"corr_pyramid_forward_slots" in msg and word in msg, msg


@pytest.mark.parametrize("kw,word", [
    (dict(ptr=FAKE, slots=None), b"null slots"),
    (dict(ptr=FAKE, slots=FAKE, cap=0), b"cap"), (dict(ptr=FAKE, slots=FAKE, cap=-1), b"cap"),
    (dict(ptr=FAKE, slots=FAKE, dtype=F64), b"dtype"), (dict(ptr=FAKE, slots=FAKE, dtype=7), b"dtype"),
    (dict(ptr=FAKE, slots=FAKE, levels=0), b"levels"), (dict(ptr=FAKE, slots=FAKE, levels=5), b"levels"),
    (dict(ptr=FAKE, slots=FAKE, C=48), b"C"), (dict(ptr=FAKE, slots=FAKE, C=288), b"C"),
    (dict(ptr=FAKE, slots=FAKE, H=4), b"map size"), (dict(ptr=FAKE, slots=FAKE, H=10, W=12), b"map size"),
    (dict(ptr=FAKE, slots=FAKE, ncam=3), b"ncam"), (dict(ptr=FAKE, slots=FAKE, nbuf=0), b"nbuf"),
    (dict(ptr=FAKE, slots=FAKE, E=-1), b"E"),
    (dict(ptr=None, slots=FAKE), b"null pointer"),
])
def test_build_refusals_need_no_gpu(backends, kw, word):
    lib = backends._lib.load()
    assert _build(lib, **kw) == DROID_E_ARG
    msg = lib.droid_last_error()
    assert b"corr_volume_pyramid_slots" in msg and word in msg, msg


def test_nothing_to_do_is_ok_and_launches_nothing(backends):
    lib = backends._lib.load()
    assert _lookup(lib, B=0) == DROID_OK          # null pointers, null slots: nothing is read
    assert _build(lib, E=0) == DROID_OK
    assert _lookup(lib, B=0, cap=0) == DROID_E_ARG   # the size checks still come first
    assert _build(lib, E=0, cap=0) == DROID_E_ARG


def test_python_keyword_refusals(backends):
    f = torch.zeros((2, 1, 32, 8, 8), dtype=torch.float16)
    ix = torch.zeros(1, dtype=torch.int64)
    out = [torch.zeros((4, 8, 8, 8 >> l, 8 >> l), dtype=torch.float16) for l in range(4)]
    with pytest.raises(RuntimeError, match="no CPU path"):     # CPU tensors are refused, not emulated
        backends.corr_volume_pyramid(f, ix, ix, out=out, slots=ix)
    with pytest.raises(RuntimeError, match="no CPU path"):
        backends.corr_pyramid_forward(out, torch.zeros((1, 2, 8, 8)), 3, slots=ix)
