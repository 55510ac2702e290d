"""CPU-side checks of the drop-in boundary: the C-ABI library loads without a GPU and exports every
symbol include/droid_backends_hip.h declares; the Python mirror exposes the reference's nine
operators (src/droid.cpp:237-250); the product never imports the oracle."""
import ctypes
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _header_symbols():
    txt = open(os.path.join(ROOT, "include", "droid_backends_hip.h")).read()
    txt = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    return sorted(set(re.findall(r"\b(droid_[a-z0-9_]+)\s*\(", txt)))


def test_library_exports_every_declared_symbol(backends):
    lib = ctypes.CDLL(backends._lib.LIB_PATH)
    syms = _header_symbols()
    assert len(syms) >= 18
    for s in syms:
        assert hasattr(lib, s), f"{s} declared in the header but not exported"
    assert sorted(backends._lib.SYMBOLS) == syms


def _header_prototypes():
    """{name: (result class, [parameter classes])} of every prototype in the header; classes are the words below."""
    txt = open(os.path.join(ROOT, "include", "droid_backends_hip.h")).read()
    txt = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    txt = re.sub(r"//[^\n]*", "", txt)

    def cls(decl, is_param):
        if "*" in decl:
            return "pointer"
        words = decl.replace("const", " ").split()
        words = words[:-1] if is_param else words   # a parameter ends with its name
        assert len(words) == 1 and words[0] in ("int", "int64_t", "size_t", "float", "double"), decl
        return words[0]

    protos = {}
    for res, name, params in re.findall(r"([A-Za-z_][\w \t\*]*?)\b(droid_[a-z0-9_]+)\s*\(([^()]*)\)\s*;", txt):
        assert name not in protos, name
        params = [p.strip() for p in params.split(",")]
        protos[name] = (cls(res, False), [] if params == ["void"] else [cls(p, True) for p in params])
    return protos


def test_binding_table_matches_the_header_prototypes(backends):
    """Arity, the class of every parameter and the class of the result of every function: a miscounted int or an
    int64_t bound as int truncates silently at sizes no test reaches."""
    protos = _header_prototypes()
    syms = _header_symbols()
    assert sorted(protos) == syms and len(protos) == len(syms) == 48   # a parser that skips a line must not pass
    of_ctype = {ctypes.c_int: "int", ctypes.c_int64: "int64_t", ctypes.c_size_t: "size_t", ctypes.c_float: "float",
                ctypes.c_double: "double", ctypes.c_void_p: "pointer", ctypes.c_char_p: "pointer"}
    assert len(of_ctype) == 7   # int64_t and size_t are distinct ctypes here

    def cls(t):
        return of_ctype.get(t) or ("pointer" if issubclass(t, ctypes._Pointer) else None)

    assert sorted(backends._lib.ABI) == syms
    lib = backends._lib.load()
    for name, (res, params) in protos.items():
        restype, argtypes = backends._lib.signature(name)
        assert res in ("int", "size_t", "pointer"), name
        assert cls(restype) == res, (name, restype, res)
        assert [cls(a) for a in argtypes] == params, (name, argtypes, params)
        fn = getattr(lib, name)   # and the loaded library carries exactly the table
        assert fn.restype == restype and list(fn.argtypes) == argtypes, name


def test_abi_version_and_workspace_query(backends):
    lib = backends._lib.load()
    assert lib.droid_abi_version() == 1
    small = lib.droid_ba_workspace_bytes(32, 8, 48, 64, 1, 8, 8)
    big = lib.droid_ba_workspace_bytes(2000, 256, 48, 64, 1, 256, 256)
    assert 0 < small < big
    assert lib.droid_ba_workspace_bytes(32, 8, 48, 64, 5, 5, 8) == 0  # empty window


def test_host_side_argument_checks_need_no_gpu(backends):
    lib = backends._lib.load()
    rc = lib.droid_corr_index_forward(None, None, None, 1, 8, 8, 8, 8, 3, 7, None)  # bad dtype
    assert rc == -1 and b"dtype" in lib.droid_last_error()
    rc = lib.droid_ba(None, None, None, None, None, None, None, None, None, 4, 8, 8, 8, 8, 5, 3, 1, 1e-4, 0.1, 0,
                      None, None, None, 0, None)  # t1 <= t0
    assert rc == -1 and b"window" in lib.droid_last_error()
    rc = lib.droid_reproject_motion(None, None, None, 3, None, None, None, 4, 8, 8, 8, None, None, None, None)  # bad stride
    assert rc == -1 and b"reproject_motion" in lib.droid_last_error()
    assert lib.droid_reproject_motion(None, None, None, 4, None, None, None, 0, 8, 8, 8, None, None, None, None) == 0  # E = 0
    assert lib.droid_chol_scratch_doubles(0) == 0
    n = 1530   # system rows of 128 bytes + diagonal / M tiles + one hand-over slot per lower-triangle tile + flags
    assert lib.droid_chol_scratch_doubles(n) >= (n + 1) * 1536 + (2 * 24 + 300) * 4096


def test_chol_scratch_grows_with_n(backends):
    """Over the sizes of the accuracy table (tests/chol_cases.py): strictly monotone, and never below the augmented
    system with 128-byte rows that opens the buffer.  The header's 128-byte claim is about the buffer's ADDRESS (the
    caller aligns it) and about the row pitch; the total is a count of doubles and need not be a multiple of 16."""
    import chol_cases
    lib = backends._lib.load()
    sizes = sorted({c.n for c in chol_cases.CASES})
    need = [lib.droid_chol_scratch_doubles(n) for n in sizes]
    assert all(a < b for a, b in zip(need, need[1:])), list(zip(sizes, need))
    for n, d in zip(sizes, need):
        assert d >= (n + 1) * ((n + 1 + 15) // 16 * 16), (n, d)


def test_python_mirror_has_the_reference_operators(backends):
    for name in ["ba", "frame_distance", "projmap", "depth_filter", "iproj", "altcorr_forward",
                 "altcorr_backward", "corr_index_forward", "corr_index_backward"]:
        assert callable(getattr(backends, name))
    for name in ["altcorr_pyramid_forward", "reproject", "motion_features", "frame_distance_matrix", "corr_pyramid_forward"]:   # additions
        assert callable(getattr(backends, name))
    from droid_backends import keyframes
    assert callable(keyframes.load) and callable(keyframes.save)


def test_cpu_tensors_are_refused_not_emulated(backends):
    import pytest
    import torch
    v = torch.zeros((1, 4, 4, 4, 4))
    c = torch.zeros((1, 2, 4, 4))
    with pytest.raises(RuntimeError, match="no CPU path"):
        backends.corr_index_forward(v, c, 3)


def test_product_does_not_reference_the_oracle():
    pkg = os.path.join(ROOT, "droid-slam_reserch_amd")
    for dp, _, fs in os.walk(pkg):
        for f in fs:
            if f.endswith((".py", ".hip", ".hpp", ".h", ".sh")):
                txt = open(os.path.join(dp, f), errors="replace").read()
                assert "import oracle" not in txt and "from oracle" not in txt, os.path.join(dp, f)
                assert "libdroid_oracle" not in txt, os.path.join(dp, f)


@pytest.mark.parametrize("op", ["corr_index_forward", "corr_index_backward", "corr_pyramid_forward", "corr_pyramid_forward_slots"])
def test_volume_operators_refuse_maps_their_32_bit_pixel_indices_cannot_hold(backends, op):
    """H1 * W1 and H2 * W2 above 2^27 are refused by name before any pointer is looked at (a query pixel index and the
    byte count of one plane are 32-bit; 46341^2 leaves int); 2^27 itself passes the size checks and fails on the null
    pointers.  Offsets into the volumes are 64-bit: tests/test_gpu_large_offsets.py."""
    lib = backends._lib.load()
    levels = (ctypes.c_void_p * 1)(None)

    def call(H1, W1, H2, W2):
        if op == "corr_index_forward":
            return lib.droid_corr_index_forward(None, None, None, 1, H1, W1, H2, W2, 3, 0, None)
        if op == "corr_index_backward":
            return lib.droid_corr_index_backward(None, None, None, 1, H1, W1, H2, W2, 3, 0, None)
        if op == "corr_pyramid_forward":
            return lib.droid_corr_pyramid_forward(levels, None, None, 1, H1, W1, 3, 1, 0, None)
        return lib.droid_corr_pyramid_forward_slots(levels, None, None, None, 1, 4, H1, W1, 3, 1, 0, None)

    shapes = [(46341, 46341, 1, 1), (1 << 14, (1 << 13) + 1, 1, 1)]
    if op.startswith("corr_index"):
        shapes += [(1, 1, 46341, 46341), (8, 8, (1 << 13) + 1, 1 << 14)]
    for shape in shapes:
        assert call(*shape) == -1
        msg = lib.droid_last_error()
        assert op.encode() in msg and b"map size" in msg, (shape, msg)
    assert call(1 << 14, 1 << 13, 1, 1) == -1 and b"null" in lib.droid_last_error()
