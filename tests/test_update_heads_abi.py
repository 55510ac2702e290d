"""CPU-side checks of droid_update_heads (include/droid_heads_hip.h): the symbols are exported and listed in their own
table, the binding table matches the prototypes, the ABI version is still 1, every host-side refusal answers DROID_E_ARG
with the operator's name before any HIP call (so none of this needs a GPU), and the Python class refuses what the
contract excludes."""
import ctypes
import os
import re

import pytest
import torch

DROID_OK, DROID_E_ARG = 0, -1
FAKE = 0x1000   # a non-null, 16-byte aligned value for pointers the host never dereferences
BIG = 2 ** 31 - 1
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ARRAYS = ("x", "packed", "out", "n_out", "act")
ALL_NULL = {k: None for k in ARRAYS}


def _ptrs(values, heads):
    return None if values is None else (ctypes.c_void_p * 2)(*(list(values) + [None, None])[:2])


def _ints(values):
    return None if values is None else (ctypes.c_int * 2)(*(list(values) + [0, 0])[:2])


def _call(lib, x=(FAKE, FAKE), packed=(FAKE, FAKE), out=(FAKE, FAKE), n_out=(2, 2), act=(0, 1), heads=2, B=3, H=6, W=8,
          in_channels=128):
    return lib.droid_update_heads(_ptrs(x, heads), _ptrs(packed, heads), _ptrs(out, heads), _ints(n_out), _ints(act),
                                  heads, B, H, W, in_channels, None)


def _prototypes(name):
    txt = open(os.path.join(ROOT, "include", name)).read()
    txt = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    txt = re.sub(r"//[^\n]*", "", txt)

    def cls(decl, is_param):
        if "*" in decl:
            return "pointer"
        words = decl.replace("const", " ").split()
        words = words[:-1] if is_param else words
        assert len(words) == 1 and words[0] in ("int", "int64_t", "size_t", "float", "double"), decl
        return words[0]

    protos = {}
    for res, fn, params in re.findall(r"([A-Za-z_][\w \t\*]*?)\b(droid_[a-z0-9_]+)\s*\(([^()]*)\)\s*;", txt):
        params = [p.strip() for p in params.split(",")]
        protos[fn] = (cls(res, False), [] if params == ["void"] else [cls(p, True) for p in params])
    return protos


def test_symbols_are_exported_listed_and_public(backends):
    L = backends._lib
    lib = ctypes.CDLL(L.LIB_PATH)
    for sym in ("droid_update_heads", "droid_head_packed_bytes"):
        assert hasattr(lib, sym) and sym in L.SYMBOLS_HEADS and sym in L.ABI_HEADS
        for other in (L.SYMBOLS, L.SYMBOLS_UPDATE, L.SYMBOLS_CORR_ENCODE, L.SYMBOLS_MOTION_ENCODE, L.SYMBOLS_TEST):
            assert sym not in other
    assert L.load().droid_abi_version() == 1   # adding a symbol keeps the ABI version
    assert "UpdateHeads" in backends.__all__ and callable(backends.UpdateHeads) and callable(backends.UpdateHeads.eta)
    assert "ba_inputs" in backends.__all__     # the consumer is as it was


def test_binding_table_matches_the_prototypes(backends):
    protos = _prototypes("droid_heads_hip.h")
    assert sorted(protos) == sorted(backends._lib.ABI_HEADS) == ["droid_head_packed_bytes", "droid_update_heads"]
    of_ctype = {ctypes.c_int: "int", ctypes.c_int64: "int64_t", ctypes.c_size_t: "size_t", ctypes.c_float: "float",
                ctypes.c_void_p: "pointer", ctypes.POINTER(ctypes.c_void_p): "pointer",
                ctypes.POINTER(ctypes.c_int): "pointer"}
    lib = backends._lib.load()
    for name, (res, params) in protos.items():
        restype, argtypes = backends._lib.signature(name)
        assert of_ctype[restype] == res and [of_ctype[a] for a in argtypes] == params, name
        fn = getattr(lib, name)
        assert fn.restype == restype and list(fn.argtypes) == argtypes, name
    hdr = open(os.path.join(ROOT, "include", "droid_heads_hip.h")).read()
    assert '#include "droid_update_hip.h"' in hdr and "Refusals" in hdr    # self-contained: contract and prototypes
    for word, value in (("DROID_HEAD_IDENTITY", 0), ("DROID_HEAD_SIGMOID", 1), ("DROID_HEAD_SOFTPLUS_CENTI", 2)):
        assert re.search(rf"{word}\s*=\s*{value}\b", hdr), word
    for other in ("droid_backends_hip.h", "droid_update_hip.h", "droid_motion_encode_hip.h"):
        assert "update_heads" not in open(os.path.join(ROOT, "include", other)).read(), other   # as they were


def test_packed_sizes(backends):
    lib = backends._lib.load()
    assert lib.droid_head_packed_bytes(2) == 9232 and lib.droid_head_packed_bytes(1) == 4624
    assert lib.droid_head_packed_bytes(0) == 0 and lib.droid_head_packed_bytes(3) == 0


@pytest.mark.parametrize("kw,word", [
    (dict(heads=0), b"bad heads"), (dict(heads=3), b"bad heads"), (dict(heads=-1), b"bad heads"),
    (dict(B=-1), b"bad B"), (dict(B=65536), b"bad B"),
    (dict(H=0), b"map size"), (dict(W=0), b"map size"), (dict(H=-3), b"map size"), (dict(H=BIG, W=BIG), b"map size"),
    (dict(H=1 << 16, W=1 << 15), b"map size"),
    (dict(in_channels=64), b"in_channels"), (dict(in_channels=256), b"in_channels"),
    (dict(n_out=(0, 2)), b"n_out"), (dict(n_out=(2, 3)), b"n_out"), (dict(n_out=(4,), heads=1), b"n_out"),
    (dict(act=(3, 0)), b"bad act"), (dict(act=(0, -1)), b"bad act"), (dict(act=(7,), heads=1), b"bad act"),
    (dict(x=(FAKE, None)), b"null pointer"), (dict(packed=(None, FAKE)), b"null pointer"),
    (dict(out=(FAKE, None)), b"null pointer"), (dict(x=(None,), heads=1), b"null pointer"),
    (dict(packed=(FAKE, FAKE + 8)), b"16-byte aligned"), (dict(packed=(FAKE + 4,), heads=1), b"16-byte aligned"),
] + [({k: None}, b"null pointer") for k in ARRAYS])
def test_refusals_need_no_gpu(backends, kw, word):
    lib = backends._lib.load()
    assert _call(lib, **kw) == DROID_E_ARG
    msg = lib.droid_last_error()
    assert b"update_heads" in msg and word in msg, msg


def test_the_order_is_sizes_then_pointers(backends):
    """All-NULL calls still name what is wrong with a size, in the order of the contract."""
    lib = backends._lib.load()
    assert _call(lib, heads=5, B=-1, **ALL_NULL) == DROID_E_ARG and b"bad heads" in lib.droid_last_error()
    assert _call(lib, B=-1, H=0, **ALL_NULL) == DROID_E_ARG and b"bad B" in lib.droid_last_error()
    assert _call(lib, H=0, in_channels=3, **ALL_NULL) == DROID_E_ARG and b"map size" in lib.droid_last_error()
    assert _call(lib, in_channels=3, **ALL_NULL) == DROID_E_ARG and b"in_channels" in lib.droid_last_error()
    assert _call(lib, **ALL_NULL) == DROID_E_ARG and b"null pointer" in lib.droid_last_error()
    nulls = dict(x=None, packed=None, out=None)
    assert _call(lib, in_channels=3, n_out=(5, 5), **nulls) == DROID_E_ARG and b"in_channels" in lib.droid_last_error()
    assert _call(lib, n_out=(5, 2), act=(9, 9), **nulls) == DROID_E_ARG and b"n_out" in lib.droid_last_error()
    assert _call(lib, act=(0, 9), **nulls) == DROID_E_ARG and b"bad act" in lib.droid_last_error()
    assert _call(lib, **nulls) == DROID_E_ARG and b"null pointer" in lib.droid_last_error()
    # a null entry comes before the alignment of another
    assert _call(lib, x=(None, FAKE), packed=(FAKE + 8, FAKE)) == DROID_E_ARG and b"null pointer" in lib.droid_last_error()
    # the second head of a one-head call is not looked at
    assert _call(lib, heads=1, B=0, n_out=(1, 9), act=(2, 9), x=(None, None)) == DROID_OK


def test_nothing_to_do_is_ok_and_launches_nothing(backends):
    lib = backends._lib.load()
    assert _call(lib, B=0, **ALL_NULL) == DROID_OK
    assert _call(lib, B=0, heads=1, **ALL_NULL) == DROID_OK
    assert _call(lib, B=0) == DROID_OK
    assert _call(lib, B=0, in_channels=64, **ALL_NULL) == DROID_E_ARG          # the size checks still come first
    assert _call(lib, B=0, heads=3, **ALL_NULL) == DROID_E_ARG
    assert _call(lib, B=0, W=0, **ALL_NULL) == DROID_E_ARG
    assert _call(lib, B=0, n_out=(2, 7), x=None, packed=None, out=None) == DROID_E_ARG
    assert _call(lib, B=0, act=(5, 0), x=None, packed=None, out=None) == DROID_E_ARG


def test_python_refusals_of_the_constructor(backends):
    w2, b2, w1, b1 = torch.zeros((2, 128, 3, 3)), torch.zeros(2), torch.zeros((1, 128, 3, 3)), torch.zeros(1)
    H = backends.UpdateHeads
    with pytest.raises(RuntimeError, match="UpdateHeads.*no CPU path"):
        H(w2, b2, w2, b2)
    with pytest.raises(RuntimeError, match="UpdateHeads.*no CPU path"):
        H(w2.half(), b2.half(), w2, b2, w1, b1)
    with pytest.raises(RuntimeError, match=r"UpdateHeads: delta_weight must be \[2,128,3,3\]"):
        H(w1, b2, w2, b2)
    with pytest.raises(RuntimeError, match=r"UpdateHeads: delta_weight must be \[2,128,3,3\]"):
        H(torch.zeros((2, 1152)), b2, w2, b2)
    with pytest.raises(RuntimeError, match=r"UpdateHeads: delta_bias must be \[2\]"):
        H(w2, b1, w2, b2)
    with pytest.raises(RuntimeError, match=r"UpdateHeads: weight_weight must be \[2,128,3,3\]"):
        H(w2, b2, torch.zeros((2, 64, 3, 3)), b2)
    with pytest.raises(RuntimeError, match=r"UpdateHeads: weight_bias must be \[2\]"):
        H(w2, b2, w2, torch.zeros(3))
    with pytest.raises(RuntimeError, match=r"UpdateHeads: eta_weight must be \[1,128,3,3\]"):
        H(w2, b2, w2, b2, w2, b1)
    with pytest.raises(RuntimeError, match=r"UpdateHeads: eta_bias must be \[1\]"):
        H(w2, b2, w2, b2, w1, b2)
    with pytest.raises(RuntimeError, match="UpdateHeads: eta_weight and eta_bias go together"):
        H(w2, b2, w2, b2, w1)
    with pytest.raises(RuntimeError, match="UpdateHeads: delta_weight must be float16 or float32"):
        H(w2.double(), b2, w2, b2)
    with pytest.raises(RuntimeError, match="UpdateHeads: eta_bias must be float16 or float32"):
        H(w2, b2, w2, b2, w1, b1.double())
    with pytest.raises(TypeError, match="UpdateHeads: weight_bias must be a tensor"):
        H(w2, b2, w2, None)


def _heads(backends, eta=True):
    """The checks of a call come before the packed buffers are looked at, so a CPU test can make them on an object that
    has none (the constructor needs a device)."""
    heads = backends.UpdateHeads.__new__(backends.UpdateHeads)
    heads.packed_delta = heads.packed_weight = torch.zeros(2308)
    heads.packed_eta = torch.zeros(1156) if eta else None
    return heads


def test_python_refusals_of_the_call(backends):
    heads = _heads(backends)
    x = torch.zeros((3, 128, 6, 8), dtype=torch.float16)
    with pytest.raises(RuntimeError, match="update_heads.*no CPU path"):           # CPU tensors are refused, not emulated
        heads(x, x.clone())
    with pytest.raises(RuntimeError, match="update_heads.*no CPU path"):           # the batched form
        heads(x[None], x.clone()[None])
    with pytest.raises(RuntimeError, match="update_heads: hd must be float16"):
        heads(x.float(), x)
    with pytest.raises(RuntimeError, match="update_heads: hw must be float16"):
        heads(x, x.to(torch.bfloat16))
    with pytest.raises(TypeError, match="update_heads: hw must be a tensor"):
        heads(x, None)
    with pytest.raises(RuntimeError, match=r"update_heads: hd must be \[B,128,h,w\] or \[1,B,128,h,w\]"):
        heads(torch.zeros((3, 64, 6, 8), dtype=torch.float16), x)
    with pytest.raises(RuntimeError, match=r"update_heads: hd must be \[B,128,h,w\] or \[1,B,128,h,w\]"):
        heads(torch.zeros((2, 3, 128, 6, 8), dtype=torch.float16), x)
    with pytest.raises(RuntimeError, match=r"update_heads: hd must be \[B,128,h,w\]"):
        heads(torch.zeros((3, 6, 8, 128), dtype=torch.float16), x)
    with pytest.raises(RuntimeError, match=r"update_heads: hw must have the shape of hd, \[3, 128, 6, 8\]"):
        heads(x, torch.zeros((2, 128, 6, 8), dtype=torch.float16))
    with pytest.raises(RuntimeError, match="update_heads: hw must be contiguous"):
        heads(x, torch.zeros((3, 6, 8, 128), dtype=torch.float16).permute(0, 3, 1, 2))
    with pytest.raises(RuntimeError, match="update_heads: hd must be contiguous"):
        heads(torch.zeros((3, 128, 6, 16), dtype=torch.float16)[..., ::2], x)
    with pytest.raises(RuntimeError, match="update_heads: hd requires grad.*inference"):
        heads(x.clone().requires_grad_(), x)


def test_python_refusals_of_eta(backends):
    heads = _heads(backends)
    net = torch.zeros((2, 128, 6, 8), dtype=torch.float16)
    with pytest.raises(RuntimeError, match=r"update_heads\.eta.*no CPU path"):
        heads.eta(net)
    with pytest.raises(RuntimeError, match=r"update_heads\.eta.*no CPU path"):
        heads.eta(net[None])
    with pytest.raises(RuntimeError, match=r"update_heads\.eta: net must be float16"):
        heads.eta(net.float())
    with pytest.raises(TypeError, match=r"update_heads\.eta: net must be a tensor"):
        heads.eta(None)
    with pytest.raises(RuntimeError, match=r"update_heads\.eta: net must be \[B,128,h,w\] or \[1,B,128,h,w\]"):
        heads.eta(torch.zeros((2, 6, 8, 128), dtype=torch.float16))
    with pytest.raises(RuntimeError, match=r"update_heads\.eta: net must be contiguous"):
        heads.eta(torch.zeros((2, 6, 8, 128), dtype=torch.float16).permute(0, 3, 1, 2))
    with pytest.raises(RuntimeError, match=r"update_heads\.eta: net requires grad.*inference"):
        heads.eta(net.clone().requires_grad_())
    with pytest.raises(RuntimeError, match=r"update_heads\.eta: this UpdateHeads was built without eta"):
        _heads(backends, eta=False).eta(net)
