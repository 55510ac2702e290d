"""CPU-side checks of droid_motion_encode (include/droid_motion_encode_hip.h): the symbols are exported and listed in
their own table, the binding table matches the prototypes, the ABI version is still 1, every host-side refusal answers
DROID_E_ARG with the operator's name before any HIP call (so none of this needs a GPU), and the Python wrappers refuse
what the contract excludes."""
import ctypes
import os
import re

import pytest
import torch

DROID_OK, DROID_E_ARG = 0, -1
FAKE = 0x1000   # a non-null, 16-byte aligned value for pointers the host never dereferences
BIG = 2 ** 31 - 1
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GEOMETRY = ("poses", "disps", "intrinsics", "ii", "jj", "target", "coords", "valid")
NO_GEOMETRY = {k: None for k in GEOMETRY}
ALL_NULL = dict(NO_GEOMETRY, motn_in=None, packed=None, out=None)


def _call(lib, poses=FAKE, disps=FAKE, intrinsics=FAKE, intr_stride=4, ii=FAKE, jj=FAKE, target=FAKE, motn_in=None,
          packed=FAKE, coords=FAKE, valid=FAKE, out=FAKE, E=2, nbuf=5, H=6, W=8, out_channels=128):
    return lib.droid_motion_encode(poses, disps, intrinsics, intr_stride, ii, jj, target, motn_in, packed, coords, valid,
                                   out, E, nbuf, H, W, out_channels, None)


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
    for sym in ("droid_motion_encode", "droid_motion_encode_packed_bytes"):
        assert hasattr(lib, sym) and sym in L.SYMBOLS_MOTION_ENCODE and sym in L.ABI_MOTION_ENCODE
        for other in (L.SYMBOLS, L.SYMBOLS_UPDATE, L.SYMBOLS_CORR_ENCODE, L.SYMBOLS_TEST):
            assert sym not in other
    assert L.load().droid_abi_version() == 1   # adding a symbol keeps the ABI version
    assert "FlowEncoder" in backends.__all__ and callable(backends.FlowEncoder)
    assert callable(backends.FlowEncoder.conv)
    assert "motion_features" in backends.__all__ and "reproject" in backends.__all__   # the unfused sequence stays


def test_binding_table_matches_the_prototypes(backends):
    protos = _prototypes("droid_motion_encode_hip.h")
    assert sorted(protos) == sorted(backends._lib.ABI_MOTION_ENCODE) == ["droid_motion_encode",
                                                                         "droid_motion_encode_packed_bytes"]
    of_ctype = {ctypes.c_int: "int", ctypes.c_int64: "int64_t", ctypes.c_size_t: "size_t", ctypes.c_float: "float",
                ctypes.c_void_p: "pointer", ctypes.POINTER(ctypes.c_void_p): "pointer"}
    lib = backends._lib.load()
    for name, (res, params) in protos.items():
        restype, argtypes = backends._lib.signature(name)
        assert of_ctype[restype] == res and [of_ctype[a] for a in argtypes] == params, name
        fn = getattr(lib, name)
        assert fn.restype == restype and list(fn.argtypes) == argtypes, name
    hdr = open(os.path.join(ROOT, "include", "droid_motion_encode_hip.h")).read()
    assert '#include "droid_update_hip.h"' in hdr and "Refusals" in hdr    # self-contained: contract and prototypes
    main = open(os.path.join(ROOT, "include", "droid_backends_hip.h")).read()
    upd = open(os.path.join(ROOT, "include", "droid_update_hip.h")).read()
    assert "motion_encode" not in main and "motion_encode" not in upd       # the other headers are as they were


def test_packed_size_is_the_corr_encoders(backends):
    from droid_backends import corr_encode as ce
    lib = backends._lib.load()
    n = lib.droid_motion_encode_packed_bytes()
    assert n == lib.droid_corr_encode_packed_bytes() == 4 * 64 * 128 * 2 + 128 * 2 == 2 * ce.packed_halves()


@pytest.mark.parametrize("kw,word", [
    (dict(E=-1), b"bad E"), (dict(E=65536), b"bad E"),
    (dict(H=0), b"map size"), (dict(W=0), b"map size"), (dict(H=-3), b"map size"), (dict(H=BIG, W=BIG), b"map size"),
    (dict(H=1 << 16, W=1 << 15), b"map size"),
    (dict(nbuf=0), b"nbuf"), (dict(nbuf=-2), b"nbuf"),
    (dict(out_channels=64), b"out_channels"), (dict(out_channels=256), b"out_channels"),
    (dict(intr_stride=1), b"intr_stride"), (dict(intr_stride=-4), b"intr_stride"), (dict(intr_stride=8), b"intr_stride"),
    (dict(packed=None), b"null pointer"), (dict(out=None), b"null pointer"),
    (dict(packed=None, motn_in=FAKE), b"null pointer"), (dict(out=None, motn_in=FAKE), b"null pointer"),
    (dict(packed=FAKE + 8), b"16-byte aligned"), (dict(packed=FAKE + 2, motn_in=FAKE), b"16-byte aligned"),
] + [({k: None}, b"null pointer") for k in GEOMETRY])
def test_refusals_need_no_gpu(backends, kw, word):
    lib = backends._lib.load()
    assert _call(lib, **kw) == DROID_E_ARG
    msg = lib.droid_last_error()
    assert b"motion_encode" in msg and word in msg, msg


def test_the_order_is_sizes_then_pointers(backends):
    """All-NULL calls still name what is wrong with a size, in the order of the contract."""
    lib = backends._lib.load()
    assert _call(lib, E=-1, H=0, **ALL_NULL) == DROID_E_ARG and b"bad E" in lib.droid_last_error()
    assert _call(lib, H=0, nbuf=0, **ALL_NULL) == DROID_E_ARG and b"map size" in lib.droid_last_error()
    assert _call(lib, nbuf=0, out_channels=3, **ALL_NULL) == DROID_E_ARG and b"nbuf" in lib.droid_last_error()
    assert _call(lib, out_channels=3, intr_stride=2, **ALL_NULL) == DROID_E_ARG and b"out_channels" in lib.droid_last_error()
    assert _call(lib, intr_stride=2, **ALL_NULL) == DROID_E_ARG and b"intr_stride" in lib.droid_last_error()
    assert _call(lib, **ALL_NULL) == DROID_E_ARG and b"null pointer" in lib.droid_last_error()
    # packed and out come before the geometry, and the alignment of packed before it too
    assert _call(lib, **dict(NO_GEOMETRY, packed=FAKE + 8)) == DROID_E_ARG and b"16-byte aligned" in lib.droid_last_error()


def test_nothing_to_do_is_ok_and_launches_nothing(backends):
    lib = backends._lib.load()
    assert _call(lib, E=0, **ALL_NULL) == DROID_OK
    assert _call(lib, E=0, intr_stride=0, **dict(ALL_NULL, motn_in=FAKE)) == DROID_OK
    assert _call(lib, E=0, out_channels=64, **ALL_NULL) == DROID_E_ARG          # the size checks still come first
    assert _call(lib, E=0, intr_stride=3, **ALL_NULL) == DROID_E_ARG
    assert _call(lib, E=0, nbuf=0, **ALL_NULL) == DROID_E_ARG


def test_python_refusals_of_the_constructor(backends):
    w, b = torch.zeros((128, 4, 7, 7)), torch.zeros(128)
    with pytest.raises(RuntimeError, match="FlowEncoder.*no CPU path"):
        backends.FlowEncoder(w, b)
    with pytest.raises(RuntimeError, match=r"FlowEncoder: weight must be \[128,4,7,7\]"):
        backends.FlowEncoder(torch.zeros((128, 196)), b)
    with pytest.raises(RuntimeError, match=r"FlowEncoder: weight must be \[128,4,7,7\]"):
        backends.FlowEncoder(torch.zeros((128, 4, 3, 3)), b)
    with pytest.raises(RuntimeError, match=r"FlowEncoder: weight must be \[128,4,7,7\]"):
        backends.FlowEncoder(torch.zeros((64, 4, 7, 7)), b)
    with pytest.raises(RuntimeError, match=r"FlowEncoder: bias must be \[128\]"):
        backends.FlowEncoder(w, torch.zeros(64))
    with pytest.raises(RuntimeError, match="FlowEncoder: weight must be float16 or float32"):
        backends.FlowEncoder(w.double(), b)
    with pytest.raises(TypeError, match="FlowEncoder: bias must be a tensor"):
        backends.FlowEncoder(w, None)


def _encoder(backends):
    """The checks of a call come before the packed buffer is looked at, so a CPU test can make them on an object that
    has none (the constructor needs a device)."""
    enc = backends.FlowEncoder.__new__(backends.FlowEncoder)
    enc.packed = torch.zeros(4 * 64 * 128 + 128, dtype=torch.float16)
    return enc


def _args(nbuf=5, E=3, h=6, w=8):
    return dict(poses=torch.zeros((nbuf, 7)), disps=torch.zeros((nbuf, h, w)), intrinsics=torch.zeros((nbuf, 4)),
                ii=torch.zeros(E, dtype=torch.int64), jj=torch.zeros(E, dtype=torch.int64),
                target=torch.zeros((1, E, h, w, 2)))


def test_python_refusals_of_the_call(backends):
    enc = _encoder(backends)
    ok = _args()
    with pytest.raises(RuntimeError, match="motion_encode.*no CPU path"):           # CPU tensors are refused, not emulated
        enc(**ok)
    with pytest.raises(RuntimeError, match="motion_encode.*no CPU path"):           # batched state, [4], [E,h,w,2]
        enc(**dict(ok, poses=ok["poses"][None], disps=ok["disps"][None], intrinsics=torch.zeros(4),
                   target=ok["target"][0]))
    with pytest.raises(RuntimeError, match="motion_encode: poses must be float32"):
        enc(**dict(ok, poses=ok["poses"].double()))
    with pytest.raises(RuntimeError, match=r"motion_encode: ii must be int64"):
        enc(**dict(ok, ii=ok["ii"].int()))
    with pytest.raises(RuntimeError, match="motion_encode: target must be float32"):
        enc(**dict(ok, target=ok["target"].half()))
    with pytest.raises(TypeError, match="motion_encode: target must be a tensor"):
        enc(**dict(ok, target=None))
    with pytest.raises(RuntimeError, match=r"motion_encode: poses must be \[nbuf,7\]"):
        enc(**dict(ok, poses=torch.zeros((5, 6))))
    with pytest.raises(RuntimeError, match=r"motion_encode: disps must be \[nbuf,h,w\]"):
        enc(**dict(ok, disps=torch.zeros((5, 48))))
    with pytest.raises(RuntimeError, match=r"motion_encode: intrinsics must be \[4\] or \[nbuf,4\]"):
        enc(**dict(ok, intrinsics=torch.zeros((5, 3))))
    with pytest.raises(RuntimeError, match=r"motion_encode: intrinsics must be \[4\] or \[nbuf,4\]"):   # fewer rows than frames
        enc(**dict(ok, intrinsics=torch.zeros((4, 4))))
    with pytest.raises(RuntimeError, match=r"motion_encode: ii and jj must be \[E\]"):
        enc(**dict(ok, jj=torch.zeros(4, dtype=torch.int64)))
    with pytest.raises(RuntimeError, match=r"motion_encode: target must be \[3, 6, 8, 2\] or \[1, 3, 6, 8, 2\]"):
        enc(**dict(ok, target=torch.zeros((3, 2, 6, 8))))
    with pytest.raises(RuntimeError, match="motion_encode: target must be contiguous"):
        enc(**dict(ok, target=torch.zeros((3, 2, 6, 8)).permute(0, 2, 3, 1)))
    with pytest.raises(RuntimeError, match="motion_encode: disps must be contiguous"):
        enc(**dict(ok, disps=torch.zeros((5, 6, 16))[..., ::2]))
    with pytest.raises(RuntimeError, match="motion_encode: target requires grad.*inference"):
        enc(**dict(ok, target=ok["target"].clone().requires_grad_()))
    with pytest.raises(RuntimeError, match="motion_encode: poses requires grad"):
        enc(**dict(ok, poses=ok["poses"].clone().requires_grad_()))


def test_python_refusals_of_conv(backends):
    enc = _encoder(backends)
    motn = torch.zeros((3, 4, 6, 8))
    with pytest.raises(RuntimeError, match=r"motion_encode\.conv.*no CPU path"):
        enc.conv(motn)
    with pytest.raises(RuntimeError, match=r"motion_encode\.conv.*no CPU path"):
        enc.conv(motn[None])
    with pytest.raises(RuntimeError, match=r"motion_encode\.conv: motn must be float32"):
        enc.conv(motn.half())
    with pytest.raises(TypeError, match=r"motion_encode\.conv: motn must be a tensor"):
        enc.conv(None)
    with pytest.raises(RuntimeError, match=r"motion_encode\.conv: motn must be \[E,4,h,w\] or \[1,E,4,h,w\]"):
        enc.conv(torch.zeros((3, 6, 8, 4)))
    with pytest.raises(RuntimeError, match=r"motion_encode\.conv: motn must be \[E,4,h,w\]"):
        enc.conv(torch.zeros((2, 3, 4, 6, 8)))
    with pytest.raises(RuntimeError, match=r"motion_encode\.conv: motn must be contiguous"):
        enc.conv(torch.zeros((3, 6, 8, 4)).permute(0, 3, 1, 2))
    with pytest.raises(RuntimeError, match=r"motion_encode\.conv: motn requires grad.*inference"):
        enc.conv(motn.clone().requires_grad_())
