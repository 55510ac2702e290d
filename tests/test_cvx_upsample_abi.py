"""CPU-side checks of the convex-upsampling entry point: the symbol is exported and listed, both Python names are
public, every host-side refusal answers DROID_E_ARG with the operator's name before any HIP call (so none of this needs
a GPU), and the Python wrappers refuse what the contract excludes."""
import ctypes

import pytest
import torch

F16, F32, F64 = 0, 1, 2
DROID_OK, DROID_E_ARG = 0, -1
FAKE = 0x1000   # a non-null value for pointers the host never dereferences: the checks return before any HIP call
BIG = 2 ** 31 - 1


def _call(lib, data=FAKE, ix=None, mask=FAKE, out=FAKE, n=2, nbuf_in=4, nbuf_out=4, H=6, W=8, dtype=F16):
    return lib.droid_cvx_upsample(data, ix, mask, out, n, nbuf_in, nbuf_out, H, W, dtype, None)


def test_symbol_is_exported_and_listed(backends):
    lib = ctypes.CDLL(backends._lib.LIB_PATH)
    assert hasattr(lib, "droid_cvx_upsample")
    assert "droid_cvx_upsample" in backends._lib.SYMBOLS
    assert backends._lib.load().droid_abi_version() == 1   # adding a symbol keeps the ABI version
    for name in ("upsample_disps", "cvx_upsample"):
        assert name in backends.__all__ and callable(getattr(backends, name))


@pytest.mark.parametrize("kw,word", [
    (dict(dtype=F64), b"dtype"), (dict(dtype=-1), b"dtype"), (dict(dtype=3), b"dtype"),
    (dict(H=0), b"map size"), (dict(W=0), b"map size"), (dict(H=-4), b"map size"),
    (dict(n=-1), b"n"),
    (dict(nbuf_in=0), b"nbuf"), (dict(nbuf_out=0), b"nbuf"), (dict(nbuf_out=-2), b"nbuf"),
    (dict(data=None), b"null pointer"), (dict(mask=None), b"null pointer"), (dict(out=None), b"null pointer"),
    (dict(H=BIG, W=BIG, nbuf_out=BIG), b"index range"),      # 8H * 8W * nbuf_out beyond 64 bits
    (dict(H=1 << 15, W=1 << 15, nbuf_out=BIG), b"index range"),
    (dict(H=1 << 16, W=1 << 15, nbuf_out=1), b"index range"),   # a coarse pixel index beyond 32 bits
])
def test_refusals_need_no_gpu(backends, kw, word):
    lib = backends._lib.load()
    assert _call(lib, **kw) == DROID_E_ARG
    msg = lib.droid_last_error()
    assert b"cvx_upsample" in msg and word in msg, msg


def test_refusals_from_null_pointers(backends):
    """The size and dtype checks come before the pointer check: all-NULL calls still name what is wrong."""
    lib = backends._lib.load()
    null = dict(data=None, mask=None, out=None)
    assert _call(lib, dtype=7, **null) == DROID_E_ARG and b"dtype" in lib.droid_last_error()
    assert _call(lib, H=0, **null) == DROID_E_ARG and b"map size" in lib.droid_last_error()
    assert _call(lib, **null) == DROID_E_ARG and b"null pointer" in lib.droid_last_error()


def test_nothing_to_do_is_ok_and_launches_nothing(backends):
    lib = backends._lib.load()
    assert _call(lib, n=0, data=None, mask=None, out=None) == DROID_OK
    assert _call(lib, n=0, data=None, mask=None, out=None, dtype=F32) == DROID_OK
    assert _call(lib, n=0, nbuf_in=0) == DROID_E_ARG          # the size checks still come first
    assert _call(lib, n=0, dtype=F64) == DROID_E_ARG


def test_python_refusals(backends):
    disps = torch.zeros((4, 6, 8))
    out = torch.zeros((4, 48, 64))
    ix = torch.zeros(2, dtype=torch.int64)
    mask = torch.zeros((1, 2, 576, 6, 8), dtype=torch.float16)
    data = torch.zeros((2, 6, 8, 1))
    with pytest.raises(RuntimeError, match="upsample_disps.*no CPU path"):     # CPU tensors are refused, not emulated
        backends.upsample_disps(disps, ix, mask, out)
    with pytest.raises(RuntimeError, match="cvx_upsample.*no CPU path"):
        backends.cvx_upsample(data, mask)
    with pytest.raises(RuntimeError, match="cvx_upsample.*dim = 1"):
        backends.cvx_upsample(torch.zeros((2, 6, 8, 2)), mask)
    with pytest.raises(RuntimeError, match="cvx_upsample.*view to"):           # 575 channels
        backends.cvx_upsample(data, torch.zeros((2, 575, 6, 8)))
    with pytest.raises(RuntimeError, match="upsample_disps.*576"):
        backends.upsample_disps(disps, ix, torch.zeros((1, 2, 575, 6, 8), dtype=torch.float16), out)
    with pytest.raises(RuntimeError, match="cvx_upsample: mask must be contiguous"):
        backends.cvx_upsample(data, torch.zeros((2, 576, 8, 6), dtype=torch.float16).transpose(2, 3))
    with pytest.raises(RuntimeError, match="upsample_disps: mask must be contiguous"):
        backends.upsample_disps(disps, ix, torch.zeros((2, 576, 6, 16), dtype=torch.float16)[..., ::2], out)
    with pytest.raises(RuntimeError, match="upsample_disps: out must be contiguous"):
        backends.upsample_disps(disps, ix, mask, torch.zeros((4, 48, 128))[..., ::2])
    with pytest.raises(RuntimeError, match=r"upsample_disps.*\[2, 576, 6, 8\]"):   # len(ix) != the mask's n
        backends.upsample_disps(disps, ix, torch.zeros((1, 3, 576, 6, 8), dtype=torch.float16), out)
    with pytest.raises(RuntimeError, match="upsample_disps.*out must be"):
        backends.upsample_disps(disps, ix, mask, torch.zeros((4, 48, 60)))
    with pytest.raises(RuntimeError, match="cvx_upsample.*autograd.*training"):
        backends.cvx_upsample(data, mask.float().requires_grad_())
    with pytest.raises(RuntimeError, match="upsample_disps.*float16 or float32"):
        backends.upsample_disps(disps, ix, mask.double(), out)
    with pytest.raises(RuntimeError, match="upsample_disps: disps must be float32"):
        backends.upsample_disps(disps.double(), ix, mask, out)
    with pytest.raises(RuntimeError, match="upsample_disps: ix must be int64"):
        backends.upsample_disps(disps, ix.int(), mask, out)
