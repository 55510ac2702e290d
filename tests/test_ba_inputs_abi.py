"""CPU-side checks of droid_ba_inputs: the prototypes of include/droid_update_hip.h match the binding table ABI_UPDATE
class by class (as tests/test_abi.py holds the main header against ABI), the library exports both symbols, every refusal
of the contract answers its code and names ba_inputs and the argument before any HIP call (so none of this needs a GPU),
sizes come before pointers, and the workspace query grows with E + Ei and is 0 for refused sizes."""
import ctypes
import os
import re

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F16, F32, F64 = 0, 1, 2
DROID_OK, DROID_E_ARG, DROID_E_WORKSPACE = 0, -1, -2
MAX_NBUF = 16384   # DROID_BA_INPUTS_MAX_NBUF
BIG = 2 ** 31 - 1

# Pointers the host never dereferences (the checks return before any HIP call), 1 MiB apart so that none of the sizes
# below makes two of them share a byte.
NAMES = ("ii", "jj", "a", "delta", "w", "damping_net", "damping_buf", "ii_inac", "jj_inac", "target_inac", "weight_inac",
         "target_state", "weight_state", "ii_ba", "jj_ba", "target_ba", "weight_ba", "eta", "frames_active", "frames_eta",
         "info", "ws")
FAKE = {name: 0x10000000 + (k << 20) for k, name in enumerate(NAMES)}


def _call(lib, E=6, Ei=3, H=5, W=7, nbuf=16, n_damp=4, net_dtype=F16, damp_dtype=F16, t0=-1, ep=1e-7, cap_e=None,
          cap_m=None, ws_bytes=1 << 16, **ptr):
    p = dict(FAKE)
    p.update(ptr)
    cap_e = E + Ei if cap_e is None else cap_e
    cap_m = min(nbuf, E + Ei) if cap_m is None else cap_m
    return lib.droid_ba_inputs(p["ii"], p["jj"], p["a"], p["delta"], p["w"], p["damping_net"], p["damping_buf"],
                               p["ii_inac"], p["jj_inac"], p["target_inac"], p["weight_inac"], E, Ei, H, W, nbuf, n_damp,
                               net_dtype, damp_dtype, t0, ep, p["target_state"], p["weight_state"], p["ii_ba"],
                               p["jj_ba"], p["target_ba"], p["weight_ba"], cap_e, p["eta"], p["frames_active"],
                               p["frames_eta"], cap_m, p["info"], p["ws"], ws_bytes, None)


def _header(name):
    txt = open(os.path.join(ROOT, "include", name)).read()
    txt = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    return re.sub(r"//[^\n]*", "", txt)


def _prototypes(txt):
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


def test_binding_table_matches_the_second_header(backends):
    protos = _prototypes(_header("droid_update_hip.h"))
    assert sorted(protos) == sorted(backends._lib.ABI_UPDATE) == ["droid_ba_inputs", "droid_ba_inputs_workspace_bytes"]
    of_ctype = {ctypes.c_int: "int", ctypes.c_int64: "int64_t", ctypes.c_size_t: "size_t", ctypes.c_float: "float",
                ctypes.c_double: "double", ctypes.c_void_p: "pointer", ctypes.c_char_p: "pointer"}
    assert len(of_ctype) == 7
    lib = backends._lib.load()
    for name, (res, params) in protos.items():
        restype, argtypes = backends._lib.signature(name)
        assert of_ctype[restype] == res, (name, restype, res)
        assert [of_ctype[a] for a in argtypes] == params, (name, argtypes, params)
        fn = getattr(lib, name)
        assert fn.restype == restype and list(fn.argtypes) == argtypes, name
    assert len(protos["droid_ba_inputs"][1]) == 36 and protos["droid_ba_inputs"][1].count("float") == 1


def test_the_main_header_and_its_table_are_unchanged_in_size(backends):
    main = _prototypes(_header("droid_backends_hip.h"))
    assert len(main) == len(backends._lib.ABI) == 48 and not set(main) & set(backends._lib.ABI_UPDATE)
    assert "droid_update_hip.h" in open(os.path.join(ROOT, "include", "droid_backends_hip.h")).read()
    assert backends._lib.load().droid_abi_version() == 1
    with pytest.raises(KeyError):
        backends._lib.signature("droid_no_such_function")


def test_symbols_are_exported_and_public(backends):
    lib = ctypes.CDLL(backends._lib.LIB_PATH)
    for sym in ("droid_ba_inputs", "droid_ba_inputs_workspace_bytes"):
        assert hasattr(lib, sym) and sym in backends._lib.SYMBOLS_UPDATE and sym not in backends._lib.SYMBOLS
    assert "ba_inputs" in backends.__all__ and callable(backends.ba_inputs)


def test_load_names_a_missing_symbol(backends, monkeypatch):
    monkeypatch.setattr(backends._lib, "_lib", None)
    monkeypatch.setattr(backends._lib, "SYMBOLS_UPDATE", ["droid_ba_inputs", "droid_not_in_the_library"])
    with pytest.raises(backends._lib.DroidBackendError, match="does not export droid_not_in_the_library"):
        backends._lib.load()


@pytest.mark.parametrize("kw,word", [
    (dict(E=0), b"bad E"), (dict(E=-4), b"bad E"), (dict(Ei=-1), b"bad Ei"),
    (dict(E=65535, Ei=1), b"E + Ei"), (dict(E=BIG, Ei=BIG), b"E + Ei"), (dict(E=65536, Ei=0), b"E + Ei"),
    (dict(nbuf=0), b"nbuf"), (dict(nbuf=-2), b"nbuf"), (dict(nbuf=MAX_NBUF + 1), b"nbuf"),
    (dict(H=0), b"map size"), (dict(W=0), b"map size"), (dict(H=-5), b"map size"),
    (dict(E=65535, Ei=0, H=BIG, W=BIG), b"2^62"), (dict(E=3, Ei=0, H=BIG, W=BIG), b"2^62"),
    (dict(cap_e=8), b"cap_e"), (dict(cap_m=8), b"cap_m"), (dict(nbuf=4, cap_m=3), b"cap_m"),
    (dict(n_damp=-1), b"n_damp"), (dict(t0=-2), b"t0"),
    (dict(net_dtype=F64), b"net_dtype"), (dict(net_dtype=-1), b"net_dtype"), (dict(damp_dtype=F64), b"damp_dtype"),
    (dict(damp_dtype=3), b"damp_dtype"),
    (dict(ii=None), b"null pointer"), (dict(jj=None), b"null pointer"), (dict(a=None), b"null pointer"),
    (dict(w=None), b"null pointer"), (dict(damping_buf=None), b"null pointer"),
    (dict(ii_inac=None), b"Ei > 0"), (dict(jj_inac=None), b"Ei > 0"), (dict(target_inac=None), b"Ei > 0"),
    (dict(weight_inac=None), b"Ei > 0"),
    (dict(ii_ba=None), b"null pointer"), (dict(jj_ba=None), b"null pointer"), (dict(target_ba=None), b"null pointer"),
    (dict(weight_ba=None), b"null pointer"), (dict(eta=None), b"null pointer"), (dict(frames_active=None), b"null pointer"),
    (dict(frames_eta=None), b"null pointer"), (dict(info=None), b"null pointer"),
    (dict(delta=None), b"emit-only"), (dict(delta=None, target_state=None), b"emit-only"),
    (dict(ws=None), b"null workspace"), (dict(ws=FAKE["ws"] + 2), b"aligned"),
    # an output sharing a byte with an input or with another output
    (dict(target_ba=FAKE["a"]), b"target_ba overlaps a"), (dict(eta=FAKE["damping_buf"] + 4), b"eta overlaps damping_buf"),
    (dict(damping_buf=FAKE["damping_net"]), b"damping_buf overlaps damping_net"),
    (dict(ii_ba=FAKE["ii"] + 40), b"ii_ba overlaps ii"), (dict(jj_ba=FAKE["ii_ba"]), b"jj_ba overlaps ii_ba"),
    (dict(weight_state=FAKE["target_state"] + 8), b"weight_state overlaps target_state"),
    (dict(weight_ba=FAKE["weight_inac"]), b"weight_ba overlaps weight_inac"),
    (dict(frames_eta=FAKE["frames_active"]), b"frames_eta overlaps frames_active"),
    (dict(info=FAKE["jj_inac"] + 16), b"info overlaps jj_inac"), (dict(ws=FAKE["delta"]), b"workspace overlaps delta"),
    (dict(ws=FAKE["info"] + 28), b"workspace overlaps info"), (dict(target_state=FAKE["w"]), b"target_state overlaps w"),
    (dict(cap_e=1 << 20, ii_ba=FAKE["ii_ba"] - (1 << 22)), b"overlaps"),     # the capacity counts, not only E + Ei
])
def test_refusals_need_no_gpu(backends, kw, word):
    lib = backends._lib.load()
    assert _call(lib, **kw) == DROID_E_ARG
    msg = lib.droid_last_error()
    assert b"ba_inputs" in msg and word in msg, msg


def test_what_the_contract_allows_passes_the_checks_up_to_the_workspace(backends):
    """NULL where the contract allows it: the call gets as far as the workspace size (still no HIP call)."""
    lib = backends._lib.load()
    none_inac = dict(ii_inac=None, jj_inac=None, target_inac=None, weight_inac=None)
    for kw in (dict(), dict(damping_net=None), dict(damping_net=None, n_damp=-7), dict(Ei=0, **none_inac),
               dict(delta=None, target_state=None, weight_state=None, damping_net=None),
               dict(target_state=None, weight_state=None), dict(t0=0), dict(t0=BIG), dict(nbuf=MAX_NBUF),
               dict(E=65535, Ei=0, H=1, W=1), dict(cap_e=40, cap_m=33)):
        assert _call(lib, ws_bytes=0, **kw) == DROID_E_WORKSPACE, kw
        assert b"ba_inputs" in lib.droid_last_error() and b"workspace too small" in lib.droid_last_error()


def test_sizes_come_before_pointers_and_pointers_before_the_workspace(backends):
    lib = backends._lib.load()
    null = {name: None for name in NAMES}
    null["ws_bytes"] = 0
    for kw, word in ((dict(E=0), b"bad E"), (dict(Ei=-1), b"bad Ei"), (dict(E=40000, Ei=40000), b"E + Ei"),
                     (dict(nbuf=0), b"nbuf"), (dict(H=0), b"map size"), (dict(cap_e=1), b"cap_e"), (dict(cap_m=1), b"cap_m"),
                     (dict(t0=-9), b"t0"), (dict(net_dtype=7), b"net_dtype"), (dict(damp_dtype=7), b"damp_dtype"),
                     (dict(), b"null pointer")):
        assert _call(lib, **dict(null, **kw)) == DROID_E_ARG and word in lib.droid_last_error(), kw
    assert _call(lib, ws=None, ws_bytes=0) == DROID_E_ARG and b"null workspace" in lib.droid_last_error()
    assert _call(lib, ws_bytes=0, eta=None) == DROID_E_ARG and b"null pointer" in lib.droid_last_error()
    assert _call(lib, ws_bytes=0, eta=FAKE["a"]) == DROID_E_WORKSPACE      # the workspace size before the overlaps


def test_a_small_workspace_is_its_own_error(backends):
    lib = backends._lib.load()
    need = lib.droid_ba_inputs_workspace_bytes(6, 3, 16)
    assert need > 0
    assert _call(lib, ws_bytes=need - 1) == DROID_E_WORKSPACE
    msg = lib.droid_last_error()
    assert b"ba_inputs" in msg and b"workspace too small" in msg


def test_workspace_grows_with_the_edges_and_is_0_for_refused_sizes(backends):
    ws = backends._lib.load().droid_ba_inputs_workspace_bytes
    assert 0 < ws(1, 0, 16) < ws(2, 0, 16) < ws(2, 1, 16) < ws(48, 24, 16) < ws(2000, 0, 16) < ws(65535, 0, 16)
    assert ws(48, 24, 16) == ws(24, 48, 16) and ws(65534, 1, 16) == ws(65535, 0, 16)      # a function of E + Ei
    assert ws(48, 24, 16) < ws(48, 24, 64) < ws(48, 24, 72) == ws(48, 24, MAX_NBUF)        # min(nbuf, E + Ei) rows
    assert ws(65535, 0, MAX_NBUF) >= 4 * (65535 + 2 * MAX_NBUF)
    for bad in ((0, 3, 16), (-1, 3, 16), (6, -1, 16), (65535, 1, 16), (BIG, BIG, 16), (6, 3, 0), (6, 3, MAX_NBUF + 1)):
        assert ws(*bad) == 0, bad


def test_python_refusals(backends):
    E, h, w = 4, 5, 7
    coords1 = torch.zeros((1, E, h, w, 2))
    delta, weight = torch.zeros((1, E, h, w, 2), dtype=torch.float16), torch.zeros((1, E, h, w, 2), dtype=torch.float16)
    damping, buf = torch.zeros((1, 2, h, w), dtype=torch.float16), torch.zeros((9, h, w))
    ii = torch.zeros(E, dtype=torch.int64)
    args = (coords1, delta, weight, damping, buf, ii, ii)
    ba_inputs = backends.ba_inputs
    with pytest.raises(RuntimeError, match="ba_inputs: coords1 must be a HIP .*no CPU path"):
        ba_inputs(*args)
    with pytest.raises(RuntimeError, match="ba_inputs: coords1 must be float32"):
        ba_inputs(coords1.half(), *args[1:])
    with pytest.raises(RuntimeError, match="ba_inputs: delta must be float16 or float32"):
        ba_inputs(coords1, delta.double(), weight, damping, buf, ii, ii)
    with pytest.raises(RuntimeError, match="ba_inputs: weight must be float16"):   # one dtype for both network outputs
        ba_inputs(coords1, delta, weight.float(), damping, buf, ii, ii)
    with pytest.raises(RuntimeError, match="ba_inputs: weight must be float32"):   # emit-only mode holds fp32 state
        ba_inputs(coords1, None, weight, None, buf, ii, ii)
    with pytest.raises(RuntimeError, match="ba_inputs: damping_buf must be float32"):
        ba_inputs(coords1, delta, weight, damping, buf.half(), ii, ii)
    with pytest.raises(RuntimeError, match="ba_inputs: ii must be int64"):
        ba_inputs(coords1, delta, weight, damping, buf, ii.int(), ii)
    with pytest.raises(TypeError, match="ba_inputs: jj must be a tensor"):
        ba_inputs(coords1, delta, weight, damping, buf, ii, [0, 0, 0, 0])
    with pytest.raises(RuntimeError, match=r"ba_inputs: coords1 must be \[1, E, h, w, 2\] or \[E, h, w, 2\]"):
        ba_inputs(torch.zeros((2, E, h, w, 2)), delta, weight, damping, buf, ii, ii)
    with pytest.raises(RuntimeError, match=r"ba_inputs: delta must be \[4, 5, 7, 2\]"):
        ba_inputs(coords1, delta[:, :3].contiguous(), weight, damping, buf, ii, ii)
    with pytest.raises(RuntimeError, match=r"ba_inputs: ii and jj must be \[E\] = \[4\]"):
        ba_inputs(coords1, delta, weight, damping, buf, ii[:3], ii)
    with pytest.raises(RuntimeError, match=r"ba_inputs: damping_buf must be \[nbuf, 5, 7\]"):
        ba_inputs(coords1, delta, weight, damping, torch.zeros((9, 7, 5)), ii, ii)
    with pytest.raises(RuntimeError, match=r"ba_inputs: damping must be \[1, G, 5, 7\] or \[G, 5, 7\]"):
        ba_inputs(coords1, delta, weight, damping[..., :6].contiguous(), buf, ii, ii)
    with pytest.raises(RuntimeError, match="ba_inputs: inactive must be"):
        ba_inputs(*args, inactive=(ii, ii))
    with pytest.raises(RuntimeError, match=r"ba_inputs: target_inac must be \[4, 5, 7, 2\]"):
        ba_inputs(*args, inactive=(ii, ii, torch.zeros((1, 3, h, w, 2)), torch.zeros((1, E, h, w, 2))))
    with pytest.raises(RuntimeError, match="ba_inputs: t0 must not be negative"):
        ba_inputs(*args, t0=-1)
    with pytest.raises(RuntimeError, match="ba_inputs: coords1 must be contiguous"):
        ba_inputs(torch.zeros((1, E, h, 2, w)).transpose(3, 4), delta, weight, damping, buf, ii, ii)
