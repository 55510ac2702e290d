"""CPU-side checks of the graph-aggregation entry point: the symbols are exported and listed, both Python names are
public, every host-side refusal answers DROID_E_ARG with the operator's name and the offending argument before any HIP
call (so none of this needs a GPU), sizes are named before pointers, the workspace query grows with E and range, and the
Python wrappers refuse what the contract excludes."""
import ctypes

import pytest
import torch

F16, F32, F64 = 0, 1, 2
DROID_OK, DROID_E_ARG, DROID_E_WORKSPACE = 0, -1, -2
FAKE = 0x1000   # a non-null value for pointers the host never dereferences: the checks return before any HIP call
BIG = 2 ** 31 - 1
MAX_RANGE = 16384   # DROID_GRAPH_MEAN_MAX_RANGE


def _call(lib, src=FAKE, index=FAKE, out=FAKE, E=9, plane=6144, M=4, range_=16, compact=1, dtype=F16, groups=None,
          ws=FAKE, ws_bytes=1 << 20):
    return lib.droid_graph_mean(src, index, out, E, plane, M, range_, compact, dtype, groups, ws, ws_bytes, None)


def test_symbols_are_exported_and_listed(backends):
    lib = ctypes.CDLL(backends._lib.LIB_PATH)
    for sym in ("droid_graph_mean", "droid_graph_mean_workspace_bytes"):
        assert hasattr(lib, sym) and sym in backends._lib.SYMBOLS
    assert backends._lib.load().droid_abi_version() == 1   # adding symbols keeps the ABI version
    for name in ("graph_mean", "scatter_mean"):
        assert name in backends.__all__ and callable(getattr(backends, name))


@pytest.mark.parametrize("kw,word", [
    (dict(E=-1), b"bad E"), (dict(E=65536), b"bad E"), (dict(E=BIG), b"bad E"),
    (dict(range_=0), b"range"), (dict(range_=-3), b"range"), (dict(range_=MAX_RANGE + 1), b"range"),
    (dict(M=0), b"bad M"), (dict(M=-1), b"bad M"),
    (dict(compact=0, M=4, range_=5), b"range == M"), (dict(compact=0, M=5, range_=4), b"range == M"),
    (dict(compact=2), b"compact"),
    (dict(plane=0), b"plane"), (dict(plane=-8), b"plane"),
    (dict(plane=2 ** 61, M=3), b"M * plane"), (dict(plane=2 ** 61, M=1, E=3), b"E * plane"),
    (dict(plane=2 ** 62 + 1, M=1, E=1), b"plane"),
    (dict(dtype=F64), b"dtype"), (dict(dtype=-1), b"dtype"), (dict(dtype=3), b"dtype"),
    (dict(src=None), b"null pointer"), (dict(index=None), b"null pointer"), (dict(out=None), b"null pointer"),
    (dict(E=0, out=None), b"null pointer"),
    (dict(ws=None), b"null workspace"),
])
def test_refusals_need_no_gpu(backends, kw, word):
    lib = backends._lib.load()
    assert _call(lib, **kw) == DROID_E_ARG
    msg = lib.droid_last_error()
    assert b"graph_mean" in msg and word in msg, msg


def test_sizes_come_before_pointers_and_pointers_before_the_workspace(backends):
    lib = backends._lib.load()
    null = dict(src=None, index=None, out=None, ws=None, ws_bytes=0)
    assert _call(lib, dtype=7, **null) == DROID_E_ARG and b"dtype" in lib.droid_last_error()
    assert _call(lib, E=70000, **null) == DROID_E_ARG and b"bad E" in lib.droid_last_error()
    assert _call(lib, range_=0, **null) == DROID_E_ARG and b"range" in lib.droid_last_error()
    assert _call(lib, M=0, **null) == DROID_E_ARG and b"bad M" in lib.droid_last_error()
    assert _call(lib, plane=0, **null) == DROID_E_ARG and b"plane" in lib.droid_last_error()
    assert _call(lib, **null) == DROID_E_ARG and b"null pointer" in lib.droid_last_error()
    assert _call(lib, ws=None, ws_bytes=0) == DROID_E_ARG and b"workspace" in lib.droid_last_error()
    assert _call(lib, ws_bytes=0, out=None) == DROID_E_ARG and b"null pointer" in lib.droid_last_error()


def test_a_small_workspace_is_its_own_error(backends):
    lib = backends._lib.load()
    need = lib.droid_graph_mean_workspace_bytes(9, 16)
    assert need > 0
    assert _call(lib, ws_bytes=need - 1) == DROID_E_WORKSPACE
    msg = lib.droid_last_error()
    assert b"graph_mean" in msg and b"workspace too small" in msg
    assert _call(lib, ws_bytes=0) == DROID_E_WORKSPACE


def test_workspace_grows_with_E_and_range(backends):
    ws = backends._lib.load().droid_graph_mean_workspace_bytes
    assert 0 < ws(1, 1) < ws(2, 1) < ws(2000, 1) < ws(65535, 1)
    assert ws(24, 1) < ws(24, 2) < ws(24, 512) < ws(24, MAX_RANGE)
    assert ws(0, 16) > 0
    assert ws(65535, MAX_RANGE) >= 4 * (65535 + MAX_RANGE + 1)           # offsets [range + 1] and entries [E], ints
    for bad in ((-1, 16), (65536, 16), (9, 0), (9, MAX_RANGE + 1)):      # sizes the call refuses: 0
        assert ws(*bad) == 0


def test_python_refusals(backends):
    net = torch.zeros((1, 9, 128, 6, 8), dtype=torch.float16)
    ii = torch.zeros(9, dtype=torch.int64)
    for fn, args in ((backends.graph_mean, (net, ii)), (backends.scatter_mean, (net, ii)),
                     (backends.graph_mean, (net[0], ii)), (backends.scatter_mean, (net[0], ii, 0))):
        with pytest.raises(RuntimeError, match=fn.__name__ + ": .*no CPU path"):   # CPU tensors are refused, not emulated
            fn(*args)
    for fn in (backends.graph_mean, backends.scatter_mean):
        name = fn.__name__
        with pytest.raises(RuntimeError, match=name + ": src must be contiguous"):
            fn(torch.zeros((1, 9, 128, 8, 6), dtype=torch.float16).transpose(3, 4), ii)
        with pytest.raises(RuntimeError, match=name + ": index must be contiguous"):
            fn(net, torch.zeros(18, dtype=torch.int64)[::2])
        with pytest.raises(RuntimeError, match=name + ": src must be float16 or float32"):
            fn(net.double(), ii)
        with pytest.raises(RuntimeError, match=name + ": src must be float16 or float32"):
            fn(net.bfloat16(), ii)
        with pytest.raises(RuntimeError, match=name + ": index must be int64"):
            fn(net, ii.int())
        with pytest.raises(RuntimeError, match=name + ": batch must be 1"):
            fn(torch.zeros((2, 9, 128, 6, 8), dtype=torch.float16), ii)
        with pytest.raises(RuntimeError, match=name + r": index must be \[E\] = \[9\]"):
            fn(net, torch.zeros(8, dtype=torch.int64))
        with pytest.raises(RuntimeError, match=name + r": index must be \[E\]"):
            fn(net, torch.zeros((1, 9), dtype=torch.int64))
        with pytest.raises(RuntimeError, match=name + ": .*autograd.*training"):
            fn(net.float().requires_grad_(), ii)
    with pytest.raises(RuntimeError, match="scatter_mean: only dim = 1"):
        backends.scatter_mean(net, ii, dim=2)
    with pytest.raises(RuntimeError, match="scatter_mean: only dim = 1"):
        backends.scatter_mean(net, ii, dim=-1)
    with pytest.raises(RuntimeError, match=r"graph_mean: net must be \[1, E, C, H, W\] or \[E, C, H, W\]"):
        backends.graph_mean(torch.zeros((9, 128, 48), dtype=torch.float16), ii)
