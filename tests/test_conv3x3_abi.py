"""CPU-side checks of droid_conv3x3 (include/droid_conv3x3_hip.h): the symbols are exported and listed in their own
table, the binding table matches the prototypes, the ABI version is still 1, droid_conv3x3_packed_bytes is the header's
arithmetic, every host-side refusal answers DROID_E_ARG with the operator's name before any HIP call (so none of this
needs a GPU), and the Python wrapper refuses what the contract excludes."""
import ctypes
import os
import re

import pytest
import torch

DROID_OK, DROID_E_ARG = 0, -1
FAKE = 0x1000   # a non-null, 16-byte aligned value for pointers the host never dereferences
BIG = 2 ** 31 - 1
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ALL_NULL = dict(x=None, packed=None, y=None)


def _call(lib, x=FAKE, packed=FAKE, y=FAKE, B=2, c_in=128, c_out=128, H=6, W=8, xbs=None, ybs=None, ygs=0,
          group_channels=None, relu=1):
    g = c_out if group_channels is None else group_channels
    xbs = min(c_in * H * W, 2 ** 62) if xbs is None else xbs      # contiguous, inside an int64 for the absurd sizes
    ybs = min(g * H * W, 2 ** 62) if ybs is None else ybs
    return lib.droid_conv3x3(x, packed, y, B, c_in, c_out, H, W, xbs, ybs, ygs, g, relu, None)


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
    for sym in ("droid_conv3x3", "droid_conv3x3_packed_bytes"):
        assert hasattr(lib, sym) and sym in L.SYMBOLS_CONV3X3 and sym in L.ABI_CONV3X3
        for other in (L.SYMBOLS, L.SYMBOLS_UPDATE, L.SYMBOLS_CORR_ENCODE, L.SYMBOLS_MOTION_ENCODE, L.SYMBOLS_HEADS,
                      L.SYMBOLS_TEST):
            assert sym not in other
    assert L.load().droid_abi_version() == 1   # adding a symbol keeps the ABI version
    assert "Conv3x3" in backends.__all__ and callable(backends.Conv3x3)
    for stays in ("CorrEncoder", "FlowEncoder", "UpdateHeads"):
        assert stays in backends.__all__


def test_binding_table_matches_the_prototypes(backends):
    protos = _prototypes("droid_conv3x3_hip.h")
    assert sorted(protos) == sorted(backends._lib.ABI_CONV3X3) == ["droid_conv3x3", "droid_conv3x3_packed_bytes"]
    of_ctype = {ctypes.c_int: "int", ctypes.c_int64: "int64_t", ctypes.c_size_t: "size_t", ctypes.c_float: "float",
                ctypes.c_void_p: "pointer", ctypes.POINTER(ctypes.c_void_p): "pointer"}
    lib = backends._lib.load()
    for name, (res, params) in protos.items():
        restype, argtypes = backends._lib.signature(name)
        assert of_ctype[restype] == res and [of_ctype[a] for a in argtypes] == params, name
        fn = getattr(lib, name)
        assert fn.restype == restype and list(fn.argtypes) == argtypes, name
    hdr = open(os.path.join(ROOT, "include", "droid_conv3x3_hip.h")).read()
    assert '#include "droid_backends_hip.h"' in hdr and "Refusals" in hdr and "packed:" in hdr
    for other in ("droid_backends_hip.h", "droid_update_hip.h", "droid_heads_hip.h", "droid_motion_encode_hip.h"):
        assert "conv3x3" not in open(os.path.join(ROOT, "include", other)).read()      # the other headers are as they were


def test_packed_bytes_is_the_headers_arithmetic(backends):
    lib = backends._lib.load()
    for c_in in (32, 64, 128, 448, 512):
        for c_out in (64, 128, 192, 256):
            n = lib.droid_conv3x3_packed_bytes(c_in, c_out)
            assert n == (9 * c_in * c_out + c_out) * 2 and n % 16 == 0
    assert lib.droid_conv3x3_packed_bytes(128, 128) == 295168
    for c_in, c_out in [(0, 128), (16, 128), (48, 128), (544, 128), (-32, 128), (128, 0), (128, 32), (128, 96), (128, 320),
                        (128, -64)]:
        assert lib.droid_conv3x3_packed_bytes(c_in, c_out) == 0


@pytest.mark.parametrize("kw,word", [
    (dict(B=-1), b"bad B"), (dict(B=65536), b"bad B"),
    (dict(c_in=0), b"c_in"), (dict(c_in=16), b"c_in"), (dict(c_in=48), b"c_in"), (dict(c_in=544), b"c_in"), (dict(c_in=-32), b"c_in"),
    (dict(c_out=0), b"c_out"), (dict(c_out=32), b"c_out"), (dict(c_out=96), b"c_out"), (dict(c_out=320), b"c_out"),
    (dict(H=0), b"map size"), (dict(W=0), b"map size"), (dict(H=-3), b"map size"), (dict(H=BIG, W=BIG), b"map size"),
    (dict(H=1 << 16, W=1 << 15), b"map size"),
    (dict(group_channels=0), b"group_channels"), (dict(group_channels=32), b"group_channels"),
    (dict(group_channels=-64), b"group_channels"), (dict(group_channels=256), b"group_channels"),
    (dict(c_out=192, group_channels=128), b"group_channels"),
    (dict(relu=2), b"relu"), (dict(relu=-1), b"relu"),
    (dict(xbs=128 * 48 - 1), b"x_batch_stride"), (dict(xbs=0), b"x_batch_stride"), (dict(xbs=-(1 << 40)), b"x_batch_stride"),
    (dict(ybs=128 * 48 - 1), b"y_batch_stride"), (dict(ybs=0), b"y_batch_stride"),
    (dict(c_out=256, group_channels=128, ybs=128 * 48 - 1), b"y_batch_stride"),
    (dict(x=None), b"null pointer"), (dict(packed=None), b"null pointer"), (dict(y=None), b"null pointer"),
    (dict(packed=FAKE + 8), b"16-byte aligned"), (dict(packed=FAKE + 2), b"16-byte aligned"),
])
def test_refusals_need_no_gpu(backends, kw, word):
    lib = backends._lib.load()
    assert _call(lib, **kw) == DROID_E_ARG
    msg = lib.droid_last_error()
    assert b"conv3x3" in msg and word in msg, msg


def test_the_order_is_sizes_then_pointers(backends):
    """All-NULL calls still name what is wrong with a size, in the order of the contract."""
    lib = backends._lib.load()
    err = lib.droid_last_error
    assert _call(lib, B=-1, c_in=0, **ALL_NULL) == DROID_E_ARG and b"bad B" in err()
    assert _call(lib, c_in=0, c_out=0, **ALL_NULL) == DROID_E_ARG and b"c_in" in err()
    assert _call(lib, c_out=0, H=0, **ALL_NULL) == DROID_E_ARG and b"c_out" in err()
    assert _call(lib, H=0, group_channels=32, **ALL_NULL) == DROID_E_ARG and b"map size" in err()
    assert _call(lib, group_channels=32, relu=3, **ALL_NULL) == DROID_E_ARG and b"group_channels" in err()
    assert _call(lib, relu=3, xbs=1, **ALL_NULL) == DROID_E_ARG and b"relu" in err()
    assert _call(lib, xbs=1, ybs=1, **ALL_NULL) == DROID_E_ARG and b"x_batch_stride" in err()
    assert _call(lib, ybs=1, **ALL_NULL) == DROID_E_ARG and b"y_batch_stride" in err()
    assert _call(lib, **ALL_NULL) == DROID_E_ARG and b"null pointer" in err()
    assert _call(lib, x=None, packed=FAKE + 8) == DROID_E_ARG and b"null pointer" in err()   # null before alignment


def test_nothing_to_do_is_ok_and_launches_nothing(backends):
    lib = backends._lib.load()
    assert _call(lib, B=0, **ALL_NULL) == DROID_OK
    assert _call(lib, B=0, xbs=0, ybs=0, relu=0, **ALL_NULL) == DROID_OK        # the strides of an empty batch are free
    assert _call(lib, B=0, c_in=48, **ALL_NULL) == DROID_E_ARG                  # the size checks still come first
    assert _call(lib, B=0, c_out=96, **ALL_NULL) == DROID_E_ARG
    assert _call(lib, B=0, H=0, **ALL_NULL) == DROID_E_ARG
    assert _call(lib, B=0, group_channels=96, **ALL_NULL) == DROID_E_ARG
    # B = 1 has no batch stride to check: the pointers are next
    assert _call(lib, B=1, xbs=0, ybs=0, **ALL_NULL) == DROID_E_ARG and b"null pointer" in lib.droid_last_error()


def test_python_refusals_of_the_constructor(backends):
    C = backends.Conv3x3
    w, b = torch.zeros((128, 128, 3, 3)), torch.zeros(128)
    with pytest.raises(RuntimeError, match="Conv3x3.*no CPU path"):
        C(w, b)
    with pytest.raises(RuntimeError, match="Conv3x3.*no CPU path"):
        C([(w, b), (w.half(), b.half())], relu=False)
    with pytest.raises(RuntimeError, match=r"Conv3x3: weight must be \[C_out,C_in,3,3\]"):
        C(torch.zeros((128, 1152)), b)
    with pytest.raises(RuntimeError, match=r"Conv3x3: weight must be \[C_out,C_in,3,3\]"):
        C(torch.zeros((128, 128, 7, 7)), b)
    with pytest.raises(RuntimeError, match=r"Conv3x3: weight must be \[C_out,C_in,3,3\] with C_in a multiple of 32"):
        C(torch.zeros((128, 4, 3, 3)), b)
    with pytest.raises(RuntimeError, match=r"Conv3x3: weight must be \[C_out,C_in,3,3\]"):
        C(torch.zeros((2, 128, 3, 3)), torch.zeros(2))
    with pytest.raises(RuntimeError, match=r"Conv3x3: bias must be \[128\]"):
        C(w, torch.zeros(64))
    with pytest.raises(RuntimeError, match="Conv3x3: weight must be float16 or float32"):
        C(w.double(), b)
    with pytest.raises(TypeError, match="Conv3x3: bias must be a tensor"):
        C(w, None)
    with pytest.raises(RuntimeError, match=r"Conv3x3: weight\[1\] must have the shape of weight\[0\]"):
        C([(w, b), (torch.zeros((64, 128, 3, 3)), torch.zeros(64))])
    with pytest.raises(RuntimeError, match=r"Conv3x3: weight\[1\] must have the shape of weight\[0\]"):
        C([(w, b), (torch.zeros((128, 64, 3, 3)), b)])
    with pytest.raises(RuntimeError, match=r"Conv3x3: bias\[1\] must be \[128\]"):
        C([(w, b), (w, torch.zeros(2))])
    with pytest.raises(RuntimeError, match="Conv3x3: the layers stack to C_out = 384"):
        C([(w, b)] * 3)
    with pytest.raises(RuntimeError, match="Conv3x3: with a list of"):
        C([(w, b)], b)
    with pytest.raises(RuntimeError, match="Conv3x3: weight must be a tensor or a non-empty list"):
        C([])


def _conv(backends, c_in=128, c_out=128, groups=1):
    """The checks of a call come before the packed buffer is looked at, so a CPU test can make them on an object that
    has none (the constructor needs a device)."""
    conv = backends.Conv3x3.__new__(backends.Conv3x3)
    conv.c_in, conv.group_channels, conv.groups, conv.c_out, conv.relu = c_in, c_out, groups, groups * c_out, True
    conv.packed = torch.zeros(9 * c_in * groups * c_out + groups * c_out, dtype=torch.float16)
    return conv


def test_python_refusals_of_the_call(backends):
    conv = _conv(backends)
    x = torch.zeros((3, 128, 6, 8), dtype=torch.float16)
    wide = torch.zeros((3, 448, 6, 8), dtype=torch.float16)
    for ok in (x, x[None], wide[:, 128:256], wide[None][:, :, 320:]):     # CPU tensors are refused, not emulated
        with pytest.raises(RuntimeError, match="conv3x3: x must be a HIP.*no CPU path"):
            conv(ok)
    with pytest.raises(RuntimeError, match="conv3x3: x must be a HIP.*no CPU path"):
        conv(x, out=wide[:, 256:384])
    with pytest.raises(RuntimeError, match="conv3x3: x must be float16"):
        conv(x.float())
    with pytest.raises(RuntimeError, match="conv3x3: out must be float16"):
        conv(x, out=torch.zeros((3, 128, 6, 8)))
    with pytest.raises(TypeError, match="conv3x3: x must be a tensor"):
        conv(None)
    with pytest.raises(RuntimeError, match=r"conv3x3: x must be \[B,128,h,w\] or \[1,B,128,h,w\]"):
        conv(torch.zeros((3, 64, 6, 8), dtype=torch.float16))                # a wrong C_in
    with pytest.raises(RuntimeError, match=r"conv3x3: x must be \[B,128,h,w\]"):
        conv(torch.zeros((2, 3, 128, 6, 8), dtype=torch.float16))
    with pytest.raises(RuntimeError, match=r"conv3x3: x must be \[B,128,h,w\]"):
        conv(torch.zeros((128, 6, 8), dtype=torch.float16))
    with pytest.raises(RuntimeError, match="conv3x3: x must have the strides"):
        conv(torch.zeros((3, 6, 8, 128), dtype=torch.float16).permute(0, 3, 1, 2))
    with pytest.raises(RuntimeError, match="conv3x3: x must have the strides"):
        conv(torch.zeros((3, 128, 6, 16), dtype=torch.float16)[..., ::2])
    with pytest.raises(RuntimeError, match="conv3x3: x must have the strides"):
        conv(torch.zeros((3, 256, 6, 8), dtype=torch.float16)[:, ::2])
    with pytest.raises(RuntimeError, match="conv3x3: x must have the strides"):
        conv(torch.zeros((3, 128, 12, 8), dtype=torch.float16)[:, :, ::2])
    with pytest.raises(RuntimeError, match="conv3x3: x must have the strides"):
        conv(x[:1].expand(3, 128, 6, 8))                                     # a batch stride below C * h * w
    with pytest.raises(RuntimeError, match="conv3x3: out must have the strides"):
        conv(x, out=torch.zeros((3, 6, 8, 128), dtype=torch.float16).permute(0, 3, 1, 2))
    with pytest.raises(RuntimeError, match=r"conv3x3: out must be \[3, 128, 6, 8\]"):
        conv(x, out=torch.zeros((2, 128, 6, 8), dtype=torch.float16))
    with pytest.raises(RuntimeError, match=r"conv3x3: out must be \[B,128,h,w\]"):
        conv(x, out=torch.zeros((3, 64, 6, 8), dtype=torch.float16))
    with pytest.raises(RuntimeError, match=r"conv3x3: out must be \[1, 3, 128, 6, 8\]"):
        conv(x[None], out=torch.zeros((3, 128, 6, 8), dtype=torch.float16))
    with pytest.raises(RuntimeError, match="conv3x3: x requires grad.*inference"):
        conv(x.float().requires_grad_().half())
    with pytest.raises(RuntimeError, match="conv3x3: out requires grad"):
        conv(x, out=torch.zeros((3, 128, 6, 8), dtype=torch.float16).requires_grad_())
    with pytest.raises(RuntimeError, match="conv3x3: out is for a single layer"):
        _conv(backends, groups=2)(x, out=torch.zeros((3, 256, 6, 8), dtype=torch.float16))


def test_overlap_of_out_and_x_is_seen_exactly(backends):
    from droid_backends.conv3x3 import _overlap
    buf = torch.zeros((3, 448, 6, 8), dtype=torch.float16)
    other = torch.zeros((3, 128, 6, 8), dtype=torch.float16)
    assert _overlap(buf[:, :128], buf[:, :128]) and _overlap(buf[:, :128], buf[:, 64:192])
    assert _overlap(buf[:, 64:192], buf[:, :128]) and _overlap(buf[:, 320:], buf[:, 300:428])
    assert not _overlap(buf[:, :128], buf[:, 128:256]) and not _overlap(buf[:, 256:384], buf[:, :128])
    assert not _overlap(buf[:, :128], other) and not _overlap(other, buf[:, 320:])
    assert _overlap(buf[:1, :128], buf[:, 64:192]) and not _overlap(buf[1:2, :128], buf[:1, 64:192])
    flat = torch.zeros(3 * 448 * 48 + 128 * 48, dtype=torch.float16)
    a = flat[:3 * 448 * 48].view(3, 448, 6, 8)[:, :128]
    b = flat[128 * 48:128 * 48 + 3 * 128 * 48].view(3, 128, 6, 8)         # another batch stride: the ranges decide
    assert _overlap(a, b)
