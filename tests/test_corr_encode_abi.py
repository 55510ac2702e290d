"""CPU-side checks of droid_corr_encode: the symbols are exported and listed, the binding table matches the prototypes,
the ABI version is still 1, every host-side refusal answers DROID_E_ARG with the operator's name before any HIP call (so
none of this needs a GPU), and the Python wrappers refuse what the contract excludes."""
import ctypes
import os
import re

import pytest
import torch

F16, F32, F64 = 0, 1, 2
DROID_OK, DROID_E_ARG = 0, -1
FAKE = 0x1000   # a non-null, 16-byte aligned value for pointers the host never dereferences
BIG = 2 ** 31 - 1
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _levels(fill=FAKE, n=4):
    return (ctypes.c_void_p * n)(*([fill] * n))


def _call(lib, volumes="fake", slots=None, coords=FAKE, packed=FAKE, out=FAKE, B=2, cap=4, H1=6, W1=8, radius=3, levels=4,
          out_channels=128, dtype=F16, layout=0):
    if isinstance(volumes, str):
        volumes = _levels()
    return lib.droid_corr_encode(volumes, slots, coords, packed, out, B, cap, H1, W1, radius, levels, out_channels, dtype,
                                 layout, None)


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
    lib = ctypes.CDLL(backends._lib.LIB_PATH)
    for sym in ("droid_corr_encode", "droid_corr_encode_packed_bytes"):
        assert hasattr(lib, sym) and sym in backends._lib.SYMBOLS_CORR_ENCODE and sym in backends._lib.ABI_CORR_ENCODE
        assert sym not in backends._lib.SYMBOLS and sym not in backends._lib.SYMBOLS_UPDATE
    assert backends._lib.load().droid_abi_version() == 1   # adding a symbol keeps the ABI version
    assert "CorrEncoder" in backends.__all__ and callable(backends.CorrEncoder)
    from droid_backends.pyramid_store import PyramidStore
    assert callable(PyramidStore.encode)


def test_binding_table_matches_the_prototypes(backends):
    protos = _prototypes("droid_corr_encode_hip.h")
    assert sorted(protos) == sorted(backends._lib.ABI_CORR_ENCODE) == ["droid_corr_encode", "droid_corr_encode_packed_bytes"]
    of_ctype = {ctypes.c_int: "int", ctypes.c_int64: "int64_t", ctypes.c_size_t: "size_t", ctypes.c_float: "float",
                ctypes.c_void_p: "pointer", ctypes.POINTER(ctypes.c_void_p): "pointer"}
    lib = backends._lib.load()
    for name, (res, params) in protos.items():
        restype, argtypes = backends._lib.signature(name)
        assert of_ctype[restype] == res and [of_ctype[a] for a in argtypes] == params, name
        fn = getattr(lib, name)
        assert fn.restype == restype and list(fn.argtypes) == argtypes, name
    upd = open(os.path.join(ROOT, "include", "droid_update_hip.h")).read()
    assert '#include "droid_corr_encode_hip.h"' in upd and "droid_corr_encode" in upd   # the contract lives there


def test_packed_size_is_host_arithmetic(backends):
    from droid_backends import corr_encode as ce
    n = backends._lib.load().droid_corr_encode_packed_bytes()
    assert n == 4 * 64 * 128 * 2 + 128 * 2 == 2 * ce.packed_halves()
    hdr = open(os.path.join(ROOT, "include", "droid_update_hip.h")).read()
    assert "#define DROID_CORR_ENCODE_PACKED_BYTES (4 * 64 * 128 * 2 + 128 * 2)" in hdr


@pytest.mark.parametrize("kw,word", [
    (dict(B=-1), b"bad B"), (dict(B=65536, cap=BIG), b"bad B"),
    (dict(H1=0), b"map size"), (dict(W1=0), b"map size"), (dict(H1=-3), b"map size"), (dict(H1=BIG, W1=BIG), b"map size"),
    (dict(H1=1 << 16, W1=1 << 15), b"map size"),
    (dict(radius=4), b"radius"), (dict(radius=0), b"radius"),
    (dict(levels=3), b"levels"), (dict(levels=5), b"levels"),
    (dict(out_channels=64), b"out_channels"), (dict(out_channels=256), b"out_channels"),
    (dict(cap=0), b"cap"), (dict(cap=-1, slots=FAKE), b"cap"), (dict(cap=1, B=2), b"cap"),
    (dict(layout=2), b"coords_layout"), (dict(layout=-1), b"coords_layout"),
    (dict(dtype=F64), b"dtype"), (dict(dtype=-1), b"dtype"), (dict(dtype=3), b"dtype"),
    (dict(volumes=None), b"null pointer"), (dict(coords=None), b"null pointer"), (dict(packed=None), b"null pointer"),
    (dict(out=None), b"null pointer"),
    (dict(volumes=_levels(None)), b"null pyramid level"),
    (dict(packed=FAKE + 8), b"16-byte aligned"),
])
def test_refusals_need_no_gpu(backends, kw, word):
    lib = backends._lib.load()
    assert _call(lib, **kw) == DROID_E_ARG
    msg = lib.droid_last_error()
    assert b"corr_encode" in msg and word in msg, msg


def test_the_order_is_sizes_then_dtypes_then_pointers(backends):
    """All-NULL calls still name what is wrong with a size or the dtype."""
    lib = backends._lib.load()
    null = dict(volumes=None, coords=None, packed=None, out=None)
    assert _call(lib, H1=0, dtype=F64, **null) == DROID_E_ARG and b"map size" in lib.droid_last_error()
    assert _call(lib, radius=4, dtype=7, **null) == DROID_E_ARG and b"radius" in lib.droid_last_error()
    assert _call(lib, dtype=F64, **null) == DROID_E_ARG and b"dtype" in lib.droid_last_error()
    assert _call(lib, **null) == DROID_E_ARG and b"null pointer" in lib.droid_last_error()


def test_a_level_without_pixels_may_be_null(backends):
    """H1 = 4: level 3 is [.., 0, W1 >> 3]; the refusal names the first level WITH pixels that is null.  (Nothing is
    launched here: the call that passes every level is made with B = 0.)"""
    lib = backends._lib.load()
    lv = (ctypes.c_void_p * 4)(FAKE, FAKE, None, None)
    assert _call(lib, volumes=lv, H1=4, W1=8) == DROID_E_ARG and b"null pyramid level" in lib.droid_last_error()


def test_nothing_to_do_is_ok_and_launches_nothing(backends):
    lib = backends._lib.load()
    null = dict(volumes=None, coords=None, packed=None, out=None)
    assert _call(lib, B=0, **null) == DROID_OK
    assert _call(lib, B=0, dtype=F32, layout=1, slots=FAKE, **null) == DROID_OK
    assert _call(lib, B=0, levels=3, **null) == DROID_E_ARG          # the size checks still come first
    assert _call(lib, B=0, dtype=F64, **null) == DROID_E_ARG


def _pyr(cap=2, h=8, w=8, dtype=torch.float16):
    return [torch.zeros((cap, h, w, h >> l, w >> l), dtype=dtype) for l in range(4)]


def test_python_refusals_of_the_constructor(backends):
    w, b = torch.zeros((128, 196, 1, 1)), torch.zeros(128)
    with pytest.raises(RuntimeError, match="CorrEncoder.*no CPU path"):
        backends.CorrEncoder(w, b)
    with pytest.raises(RuntimeError, match=r"CorrEncoder: weight must be \[128,196,1,1\]"):
        backends.CorrEncoder(torch.zeros((128, 196, 3, 3)), b)
    with pytest.raises(RuntimeError, match=r"CorrEncoder: weight must be \[128,196,1,1\]"):
        backends.CorrEncoder(torch.zeros((64, 196)), b)
    with pytest.raises(RuntimeError, match=r"CorrEncoder: bias must be \[128\]"):
        backends.CorrEncoder(w, torch.zeros(64))
    with pytest.raises(RuntimeError, match="CorrEncoder: weight must be float16 or float32"):
        backends.CorrEncoder(w.double(), b)
    with pytest.raises(TypeError, match="CorrEncoder: bias must be a tensor"):
        backends.CorrEncoder(w, None)


def test_python_refusals_of_the_call(backends):
    """The checks of a call come before the packed buffer is looked at, so a CPU test can make them on an object that
    has none (the constructor needs a device)."""
    enc = backends.CorrEncoder.__new__(backends.CorrEncoder)
    enc.packed = torch.zeros(4 * 64 * 128 + 128, dtype=torch.float16)
    pyr, coords = _pyr(), torch.zeros((2, 2, 8, 8))
    with pytest.raises(RuntimeError, match="corr_encode.*no CPU path"):           # CPU tensors are refused, not emulated
        enc(pyr, coords)
    with pytest.raises(ValueError, match="corr_encode: layout"):
        enc(pyr, coords, layout="chw")
    with pytest.raises(RuntimeError, match=r"corr_encode: coords must be \[2, 8, 8, 2\] for layout 'hw2'"):
        enc(pyr, coords, layout="hw2")
    with pytest.raises(RuntimeError, match=r"corr_encode: coords must be \[2, 2, 8, 8\]"):
        enc(pyr, torch.zeros((2, 8, 8, 2)))
    with pytest.raises(RuntimeError, match="corr_encode: coords must be float32"):
        enc(pyr, coords.double())
    with pytest.raises(RuntimeError, match=r"corr_encode: pyramid\[0\] must be float16 or float32"):   # f64 is refused
        enc(_pyr(dtype=torch.float64), coords)
    with pytest.raises(RuntimeError, match="corr_encode: pyramid levels must share one dtype"):
        enc(pyr[:3] + [pyr[3].float()], coords)
    with pytest.raises(RuntimeError, match="corr_encode: the pyramid must have 4 levels"):
        enc(pyr[:3], coords)
    with pytest.raises(RuntimeError, match=r"corr_encode: pyramid\[2\] must be \[2,8,8,2,2\]"):
        enc(pyr[:2] + [torch.zeros((2, 8, 8, 2, 3), dtype=torch.float16), pyr[3]], coords)
    with pytest.raises(RuntimeError, match="corr_encode: slots must be int64"):
        enc(pyr, coords, slots=torch.zeros(2, dtype=torch.int32))
    with pytest.raises(RuntimeError, match=r"corr_encode: slots must be \[E\]"):
        enc(pyr, coords, slots=torch.zeros((2, 1), dtype=torch.int64))
    with pytest.raises(RuntimeError, match=r"corr_encode: coords must be \[3, 2, 8, 8\]"):   # E comes from the slots
        enc(pyr, coords, slots=torch.zeros(3, dtype=torch.int64))
    with pytest.raises(RuntimeError, match="corr_encode: coords must be contiguous"):
        enc(pyr, torch.zeros((2, 8, 8, 2)).permute(0, 3, 1, 2))
    with pytest.raises(RuntimeError, match=r"corr_encode: pyramid\[1\] must be contiguous"):
        enc([pyr[0], torch.zeros((2, 8, 8, 4, 8), dtype=torch.float16)[..., ::2], pyr[2], pyr[3]], coords)
    with pytest.raises(RuntimeError, match="corr_encode: coords requires grad.*inference"):
        enc(pyr, coords.clone().requires_grad_())
    with pytest.raises(RuntimeError, match=r"corr_encode: pyramid\[0\] requires grad"):
        enc([pyr[0].float().requires_grad_()] + [p.float() for p in pyr[1:]], coords)


def test_store_encode_refuses_other_shapes(backends):
    from droid_backends.pyramid_store import PyramidStore
    store = PyramidStore(torch.zeros((3, 1, 32, 8, 8), dtype=torch.float16), cap=2)
    with pytest.raises(RuntimeError, match=r"PyramidStore.encode: coords1 must be \[1, 0, h, w, 2\]"):
        store.encode(torch.zeros((1, 2, 8, 8, 2)), None)
    with pytest.raises(RuntimeError, match="PyramidStore.encode: coords1 must be"):
        store.encode(torch.zeros((0, 2, 8, 8)), None)
    assert store.encode(torch.zeros((1, 0, 8, 8, 2)), None).shape == (0, 128, 8, 8)
