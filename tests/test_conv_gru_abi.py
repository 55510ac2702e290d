"""CPU-side checks of the ConvGRU's C ABI (include/droid_gru_hip.h): the symbols are exported and listed in a table of
their own, the binding table matches the prototypes, the ABI version is still 1, the two size functions are the header's
arithmetic, every host-side refusal answers DROID_E_ARG with the operator's name before any HIP call (none of this needs
a GPU), and the Python wrapper refuses what the contract excludes."""
import ctypes
import os

import pytest
import torch

from test_conv3x3_abi import _prototypes

DROID_OK, DROID_E_ARG = 0, -1
FAKE = 0x1000   # a non-null, 16-byte aligned value for pointers the host never dereferences
BIG = 2 ** 31 - 1
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ["droid_conv_gru", "droid_gru_context", "droid_gru_gates", "droid_gru_packed_bytes", "droid_gru_update",
         "droid_gru_workspace_bytes"]
H, W = 6, 8


def _table(seg, strides, channels):
    k = len(channels)
    return ((ctypes.c_void_p * k)(*seg), (ctypes.c_int64 * k)(*strides), (ctypes.c_int * k)(*channels))


def _segs(kw):
    """The segment table of a call from keyword overrides; None for an array leaves it out (a null array)."""
    channels = kw.pop("channels", [128, 128, 128, 64])
    h, w = kw.get("H", H), kw.get("W", W)
    strides = kw.pop("strides", [min(c * h * w, 2 ** 62) if c > 0 else 0 for c in channels])
    seg = (kw.pop("seg", [FAKE] * len(channels)) + [0] * len(channels))[:len(channels)]
    nseg = kw.pop("nseg", len(channels))
    s, b, c = _table(seg, strides, channels)
    null = kw.pop("null_array", None)
    return (None if null == "seg" else s, None if null == "strides" else b, None if null == "channels" else c, nseg)


def _ws_bytes(lib, kw):
    return lib.droid_gru_workspace_bytes(max(min(kw.get("B", 2), 65535), 0), kw.get("H", H), kw.get("W", W))


def _fused(lib, **kw):
    s, b, c, nseg = _segs(kw)
    a = dict(packed=FAKE, out=FAKE, obs=None, B=2, H=H, W=W, ws=FAKE, ws_bytes=None)
    a.update(kw)
    obs = min(128 * a["H"] * a["W"], 2 ** 62) if a["obs"] is None else a["obs"]
    wsb = _ws_bytes(lib, a) if a["ws_bytes"] is None else _ws_bytes(lib, a) - 1 if a["ws_bytes"] == "short" else a["ws_bytes"]
    return lib.droid_conv_gru(s, b, c, nseg, a["packed"], a["out"], obs, a["B"], a["H"], a["W"], a["ws"], wsb, None)


def _gates(lib, **kw):
    s, b, c, nseg = _segs(kw)
    a = dict(packed=FAKE, g=FAKE, z=FAKE, rnet=FAKE, B=2, H=H, W=W)
    a.update(kw)
    return lib.droid_gru_gates(s, b, c, nseg, a["packed"], a["g"], a["z"], a["rnet"], a["B"], a["H"], a["W"], None)


def _update(lib, **kw):
    s, b, c, nseg = _segs(kw)
    a = dict(packed=FAKE, g=FAKE, z=FAKE, net=FAKE, nbs=None, out=FAKE, obs=None, B=2, H=H, W=W)
    a.update(kw)
    hw = min(128 * a["H"] * a["W"], 2 ** 62)
    nbs, obs = (hw if a[k] is None else a[k] for k in ("nbs", "obs"))
    return lib.droid_gru_update(s, b, c, nseg, a["packed"], a["g"], a["z"], a["net"], nbs, a["out"], obs, a["B"], a["H"], a["W"], None)


def _context(lib, **kw):
    a = dict(net=FAKE, nbs=None, packed=FAKE, c_in=448, B=2, H=H, W=W, g=FAKE, ws=FAKE, ws_bytes=None)
    a.update(kw)
    nbs = min(128 * a["H"] * a["W"], 2 ** 62) if a["nbs"] is None else a["nbs"]
    wsb = _ws_bytes(lib, a) if a["ws_bytes"] is None else a["ws_bytes"]
    return lib.droid_gru_context(a["net"], nbs, a["packed"], a["c_in"], a["B"], a["H"], a["W"], a["g"], a["ws"], wsb, None)


SEG_CALLS = [_fused, _gates, _update]


def test_symbols_are_exported_listed_and_public(backends):
    L = backends._lib
    lib = ctypes.CDLL(L.LIB_PATH)
    assert sorted(L.SYMBOLS_GRU) == sorted(L.ABI_GRU) == NAMES
    for sym in NAMES:
        assert hasattr(lib, sym)
        for other in (L.SYMBOLS, L.SYMBOLS_UPDATE, L.SYMBOLS_CORR_ENCODE, L.SYMBOLS_MOTION_ENCODE, L.SYMBOLS_HEADS,
                      L.SYMBOLS_CONV3X3, L.SYMBOLS_TEST):
            assert sym not in other
    assert L.load().droid_abi_version() == 1   # adding symbols keeps the ABI version
    assert "ConvGRU" in backends.__all__ and callable(backends.ConvGRU)
    for stays in ("CorrEncoder", "FlowEncoder", "UpdateHeads", "Conv3x3"):
        assert stays in backends.__all__


def test_binding_table_matches_the_prototypes(backends):
    protos = _prototypes("droid_gru_hip.h")
    assert sorted(protos) == NAMES
    of_ctype = {ctypes.c_int: "int", ctypes.c_int64: "int64_t", ctypes.c_size_t: "size_t", ctypes.c_float: "float",
                ctypes.c_void_p: "pointer", ctypes.POINTER(ctypes.c_void_p): "pointer", ctypes.POINTER(ctypes.c_int64): "pointer",
                ctypes.POINTER(ctypes.c_int): "pointer"}
    lib = backends._lib.load()
    for name, (res, params) in protos.items():
        restype, argtypes = backends._lib.signature(name)
        assert of_ctype[restype] == res and [of_ctype[a] for a in argtypes] == params, name
        fn = getattr(lib, name)
        assert fn.restype == restype and list(fn.argtypes) == argtypes, name
    # the typed arrays sit where the header has them: pointers, int64 strides, int channels
    for name in ("droid_conv_gru", "droid_gru_gates", "droid_gru_update"):
        args = backends._lib.signature(name)[1]
        assert args[:4] == [ctypes.POINTER(ctypes.c_void_p), ctypes.POINTER(ctypes.c_int64), ctypes.POINTER(ctypes.c_int), ctypes.c_int]
    hdr = open(os.path.join(ROOT, "include", "droid_gru_hip.h")).read()
    assert '#include "droid_backends_hip.h"' in hdr and "Refusals" in hdr and "packed:" in hdr
    for other in ("droid_backends_hip.h", "droid_update_hip.h", "droid_heads_hip.h", "droid_motion_encode_hip.h",
                  "droid_conv3x3_hip.h", "droid_corr_encode_hip.h"):
        assert "gru" not in open(os.path.join(ROOT, "include", other)).read().lower()      # the other headers are as they were


def test_size_functions_are_the_headers_arithmetic(backends):
    lib = backends._lib.load()
    for c_in in (160, 192, 448, 512):
        n = lib.droid_gru_packed_bytes(c_in)
        assert n == (9 * c_in * 384 + 4 * 128 * 128 + 7 * 128) * 2 and n % 16 == 0
    for c_in in (0, 128, 144, 176, 544, -160):
        assert lib.droid_gru_packed_bytes(c_in) == 0
    for B, h, w in [(1, 1, 1), (3, 5, 9), (2, 9, 70), (24, 48, 64), (0, 4, 4)]:
        tiles = (h * w + 255) // 256
        plane = (B * 128 * h * w * 2 + 15) // 16 * 16
        assert lib.droid_gru_workspace_bytes(B, h, w) == B * tiles * 512 + B * 3 * 128 * 4 + 2 * plane
    for B, h, w in [(-1, 4, 4), (65536, 4, 4), (1, 0, 4), (1, 4, 0), (1, BIG, BIG), (1, 1 << 16, 1 << 15)]:
        assert lib.droid_gru_workspace_bytes(B, h, w) == 0


@pytest.mark.parametrize("call", SEG_CALLS, ids=lambda f: f.__name__)
@pytest.mark.parametrize("kw,word", [
    (dict(B=-1), b"bad B"), (dict(B=65536), b"bad B"),
    (dict(channels=[128], nseg=1), b"nseg"), (dict(channels=[128, 32, 32, 32, 32, 32]), b"nseg"), (dict(nseg=0), b"nseg"),
    (dict(null_array="seg"), b"null array"), (dict(null_array="strides"), b"null array"), (dict(null_array="channels"), b"null array"),
    (dict(channels=[64, 128, 128, 128]), b"seg_channels[0]"), (dict(channels=[128, 48, 128]), b"seg_channels[1]"),
    (dict(channels=[128, 128, 0]), b"seg_channels[2]"), (dict(channels=[128, 128, -32]), b"seg_channels[2]"),
    (dict(channels=[128, 128, 128, 64, 16]), b"seg_channels[4]"),
    (dict(channels=[128, 256, 160]), b"c_in"), (dict(channels=[128, 512]), b"c_in"),
    (dict(H=0), b"map size"), (dict(W=0), b"map size"), (dict(H=-3), b"map size"), (dict(H=BIG, W=BIG), b"map size"),
    (dict(H=1 << 16, W=1 << 15), b"map size"),
    (dict(strides=[128 * 48 - 1, 128 * 48, 128 * 48, 64 * 48]), b"seg_batch_stride[0]"),
    (dict(strides=[128 * 48, 128 * 48, 128 * 48, 0]), b"seg_batch_stride[3]"),
    (dict(strides=[128 * 48, -(1 << 40), 128 * 48, 64 * 48]), b"seg_batch_stride[1]"),
    (dict(seg=[FAKE, 0, FAKE, FAKE]), b"null pointer"), (dict(seg=[0, FAKE, FAKE, FAKE]), b"null pointer"),
    (dict(packed=None), b"null pointer"),
    (dict(packed=FAKE + 8), b"16-byte aligned"), (dict(packed=FAKE + 2), b"16-byte aligned"),
])
def test_refusals_of_the_segment_calls_need_no_gpu(backends, call, kw, word):
    lib = backends._lib.load()
    assert call(lib, **dict(kw)) == DROID_E_ARG
    msg = lib.droid_last_error()
    assert b"conv_gru" in msg and word in msg, msg


@pytest.mark.parametrize("call,kw,word", [
    (_fused, dict(obs=128 * 48 - 1), b"out_batch_stride"), (_fused, dict(obs=0), b"out_batch_stride"),
    (_fused, dict(ws_bytes=0), b"ws_bytes"), (_fused, dict(ws_bytes="short"), b"ws_bytes"),
    (_fused, dict(out=None), b"null pointer"), (_fused, dict(ws=None), b"null pointer"), (_fused, dict(ws=FAKE + 4), b"16-byte aligned"),
    (_gates, dict(g=None), b"null pointer"), (_gates, dict(z=None), b"null pointer"), (_gates, dict(rnet=None), b"null pointer"),
    (_update, dict(nbs=128 * 48 - 1), b"net_batch_stride"), (_update, dict(obs=128 * 48 - 1), b"out_batch_stride"),
    (_update, dict(g=None), b"null pointer"), (_update, dict(z=None), b"null pointer"), (_update, dict(net=None), b"null pointer"),
    (_update, dict(out=None), b"null pointer"),
    (_context, dict(B=-1), b"bad B"), (_context, dict(B=65536), b"bad B"),
    (_context, dict(c_in=128), b"c_in"), (_context, dict(c_in=176), b"c_in"), (_context, dict(c_in=544), b"c_in"),
    (_context, dict(H=0), b"map size"), (_context, dict(H=BIG, W=BIG), b"map size"),
    (_context, dict(nbs=128 * 48 - 1), b"net_batch_stride"), (_context, dict(ws_bytes=2 * 512 - 1), b"ws_bytes"),
    (_context, dict(net=None), b"null pointer"), (_context, dict(packed=None), b"null pointer"), (_context, dict(g=None), b"null pointer"),
    (_context, dict(ws=None), b"null pointer"), (_context, dict(packed=FAKE + 8), b"16-byte aligned"),
    (_context, dict(ws=FAKE + 8), b"16-byte aligned"),
])
def test_refusals_of_each_call_need_no_gpu(backends, call, kw, word):
    lib = backends._lib.load()
    assert call(lib, **dict(kw)) == DROID_E_ARG
    msg = lib.droid_last_error()
    assert b"conv_gru" in msg and word in msg, msg


def test_the_order_is_sizes_then_pointers(backends):
    """Calls whose pointers are all null still name what is wrong with a size, in the order of the contract."""
    lib = backends._lib.load()
    err = lib.droid_last_error
    null = dict(seg=[0, 0, 0, 0], packed=None, out=None, ws=None)
    assert _fused(lib, B=-1, nseg=0, **null) == DROID_E_ARG and b"bad B" in err()
    assert _fused(lib, nseg=0, null_array="seg", **null) == DROID_E_ARG and b"nseg" in err()
    assert _fused(lib, null_array="channels", H=0, **null) == DROID_E_ARG and b"null array" in err()
    assert _fused(lib, channels=[128, 48, 128, 64], H=0, **null) == DROID_E_ARG and b"seg_channels[1]" in err()
    assert _fused(lib, channels=[128, 512], H=0, **null) == DROID_E_ARG and b"c_in" in err()
    assert _fused(lib, H=0, strides=[1, 1, 1, 1], **null) == DROID_E_ARG and b"map size" in err()
    assert _fused(lib, strides=[1, 1, 1, 1], obs=1, **null) == DROID_E_ARG and b"seg_batch_stride[0]" in err()
    assert _fused(lib, obs=1, ws_bytes=0, **null) == DROID_E_ARG and b"out_batch_stride" in err()
    assert _fused(lib, ws_bytes=0, **null) == DROID_E_ARG and b"ws_bytes" in err()
    assert _fused(lib, **null) == DROID_E_ARG and b"null pointer" in err()
    assert _fused(lib, out=None, packed=FAKE + 8) == DROID_E_ARG and b"null pointer" in err()   # null before alignment
    assert _update(lib, nbs=1, obs=1) == DROID_E_ARG and b"net_batch_stride" in err()


def test_nothing_to_do_is_ok_and_launches_nothing(backends):
    lib = backends._lib.load()
    null = dict(seg=[0, 0, 0, 0], packed=None)
    assert _fused(lib, B=0, out=None, ws=None, **null) == DROID_OK
    assert _fused(lib, B=0, out=None, ws=None, strides=[0, 0, 0, 0], obs=0, **null) == DROID_OK   # the strides of an empty batch are free
    assert _gates(lib, B=0, g=None, z=None, rnet=None, **null) == DROID_OK
    assert _update(lib, B=0, g=None, z=None, net=None, out=None, **null) == DROID_OK
    assert _context(lib, B=0, net=None, packed=None, g=None, ws=None) == DROID_OK
    assert _fused(lib, B=0, channels=[128, 48, 128], **null) == DROID_E_ARG      # the size checks still come first
    assert _fused(lib, B=0, H=0, **null) == DROID_E_ARG
    # B = 1 has no batch stride to check: the pointers are next
    assert _fused(lib, B=1, strides=[0, 0, 0, 0], obs=0, out=None, ws=None, **null) == DROID_E_ARG and b"null pointer" in lib.droid_last_error()


# ---------------------------------------------------------------------------------------------------- the Python side
def _params(c_in=448, dtype=torch.float32):
    p = {k: (torch.zeros((128, c_in, 3, 3), dtype=dtype), torch.zeros(128, dtype=dtype)) for k in ("convz", "convr", "convq")}
    p.update({k: (torch.zeros((128, 128, 1, 1), dtype=dtype), torch.zeros(128, dtype=dtype))
              for k in ("w", "convz_glo", "convr_glo", "convq_glo")})
    return p


def test_python_refusals_of_the_constructor(backends):
    G = backends.ConvGRU
    with pytest.raises(RuntimeError, match="ConvGRU.*no CPU path"):
        G(**_params())
    with pytest.raises(RuntimeError, match="ConvGRU.*no CPU path"):
        G(**_params(160, torch.float16))
    p = _params()
    p["convr"] = (torch.zeros((128, 416, 3, 3)), torch.zeros(128))
    with pytest.raises(RuntimeError, match=r"ConvGRU: convr.weight must have the 448 input channels"):
        G(**p)
    for bad in (torch.zeros((128, 448, 1, 1)), torch.zeros((64, 448, 3, 3)), torch.zeros((128, 128, 3, 3)), torch.zeros((128, 440, 3, 3))):
        p = _params()
        p["convz"] = (bad, torch.zeros(128))
        with pytest.raises(RuntimeError, match=r"ConvGRU: convz.weight must be \[128,C,3,3\]"):
            G(**p)
    p = _params()
    p["convq_glo"] = (torch.zeros((128, 64, 1, 1)), torch.zeros(128))
    with pytest.raises(RuntimeError, match=r"ConvGRU: convq_glo.weight must be \[128,128,1,1\]"):
        G(**p)
    p = _params()
    p["w"] = (p["w"][0], torch.zeros(64))
    with pytest.raises(RuntimeError, match=r"ConvGRU: w.bias must be \[128\]"):
        G(**p)
    p = _params()
    p["convz"] = (p["convz"][0].double(), p["convz"][1])
    with pytest.raises(RuntimeError, match="ConvGRU: convz.weight must be float16 or float32"):
        G(**p)
    p = _params()
    p["convr_glo"] = (p["convr_glo"][0], None)
    with pytest.raises(TypeError, match="ConvGRU: convr_glo.bias must be a tensor"):
        G(**p)
    p = _params()
    p["convq"] = p["convq"][0]
    with pytest.raises(RuntimeError, match=r"ConvGRU: convq must be a \(weight, bias\) pair"):
        G(**p)

    class Module:
        pass
    m = Module()
    with pytest.raises(RuntimeError, match="ConvGRU: the module has no layer convz"):
        G.from_module(m)
    for k in ("convz", "convr", "convq"):
        setattr(m, k, torch.nn.Conv2d(448, 128, 3, padding=1))
    for k in ("w", "convz_glo", "convr_glo", "convq_glo"):
        setattr(m, k, torch.nn.Conv2d(128, 128, 1))
    with pytest.raises(RuntimeError, match="ConvGRU.*no CPU path"):          # every layer was found and has the right shape
        G.from_module(m)


def _gru(backends, c_in=448):
    """The checks of a call come before the packed buffer is looked at, so a CPU test can make them on an object that
    has none (the constructor needs a device)."""
    gru = backends.ConvGRU.__new__(backends.ConvGRU)
    gru.c_in = c_in
    gru.packed = torch.zeros(8, dtype=torch.float16)
    return gru


def test_python_refusals_of_the_calls(backends):
    gru = _gru(backends)
    h = lambda *s: torch.zeros(s, dtype=torch.float16)
    net, inp, corr, flow = h(3, 128, 6, 8), h(3, 128, 6, 8), h(3, 128, 6, 8), h(3, 64, 6, 8)
    wide = h(3, 448, 6, 8)
    cpu = "must be a HIP.*no CPU path"
    for args in ((net, inp, corr, flow), (net[None], inp[None], corr[None], flow[None]), (net, wide[:, 128:]),
                 (wide[:, :128], wide[:, 128:256], wide[:, 256:384], wide[:, 384:])):
        with pytest.raises(RuntimeError, match="conv_gru: net " + cpu):        # CPU tensors are refused, not emulated
            gru(*args)
    with pytest.raises(RuntimeError, match="conv_gru: takes 1 to 4 inputs"):
        gru(net)
    with pytest.raises(RuntimeError, match="conv_gru: takes 1 to 4 inputs"):
        gru(net, flow, flow, flow, flow, flow)
    with pytest.raises(RuntimeError, match="conv_gru: net must be float16"):
        gru(net.float(), inp, corr, flow)
    with pytest.raises(RuntimeError, match=r"conv_gru: inputs\[1\] must be float16"):
        gru(net, inp, corr.float(), flow)
    with pytest.raises(TypeError, match=r"conv_gru: inputs\[2\] must be a tensor"):
        gru(net, inp, corr, None)
    with pytest.raises(RuntimeError, match=r"conv_gru: net must be \[B,128,h,w\]"):
        gru(h(3, 64, 6, 8), inp, corr, flow)
    with pytest.raises(RuntimeError, match=r"conv_gru: inputs\[0\] must be \[B,C,h,w\] or \[1,B,C,h,w\] with C a positive multiple of 32"):
        gru(net, h(3, 48, 6, 8), corr, flow)
    with pytest.raises(RuntimeError, match=r"conv_gru: inputs\[2\] must be \[3, 64, 6, 8\] like net"):
        gru(net, inp, corr, h(2, 64, 6, 8))
    with pytest.raises(RuntimeError, match=r"conv_gru: inputs\[1\] must be \[3, 128, 6, 8\] like net"):
        gru(net, inp, h(3, 128, 8, 6), flow)
    with pytest.raises(RuntimeError, match=r"conv_gru: inputs\[0\] must be \[3, 128, 6, 8\] like net"):
        gru(net, inp[None], corr, flow)
    with pytest.raises(RuntimeError, match="conv_gru: net and the inputs have 384 channels in all, the module was built for 448"):
        gru(net, inp, corr)
    with pytest.raises(RuntimeError, match=r"conv_gru: inputs\[1\] must have the strides"):
        gru(net, inp, h(3, 6, 8, 128).permute(0, 3, 1, 2), flow)
    with pytest.raises(RuntimeError, match="conv_gru: net must have the strides"):
        gru(h(3, 256, 6, 8)[:, ::2], inp, corr, flow)
    with pytest.raises(RuntimeError, match="conv_gru: net requires grad.*inference"):
        gru(net.float().requires_grad_().half(), inp, corr, flow)
    with pytest.raises(RuntimeError, match="conv_gru: out must be float16"):
        gru(net, inp, corr, flow, out=net.float())
    with pytest.raises(RuntimeError, match=r"conv_gru: out must be \[3, 128, 6, 8\]"):
        gru(net, inp, corr, flow, out=h(2, 128, 6, 8))
    # the overlap rules are checked before a launch: out may be net itself, nothing else
    with pytest.raises(RuntimeError, match="conv_gru: net " + cpu):
        gru(net, inp, corr, flow, out=net)
    assert gru._out("conv_gru", net, net, False, [inp, corr, flow]) is net
    with pytest.raises(RuntimeError, match="conv_gru: out must be net itself or must not overlap net"):
        gru._out("conv_gru", wide[:, 64:192], wide[:, :128], False, [])
    with pytest.raises(RuntimeError, match=r"conv_gru: out must not overlap inputs\[1\]"):
        gru._out("conv_gru", wide[:, 256:384], net, False, [inp, wide[:, 320:]])
    # the phases
    g = torch.zeros((3, 3, 128))
    with pytest.raises(RuntimeError, match="conv_gru.context: net " + cpu):
        gru.context(net)
    with pytest.raises(RuntimeError, match="conv_gru.gates: g must be float32"):
        gru.gates(g.half(), net, inp, corr, flow)
    with pytest.raises(RuntimeError, match=r"conv_gru.gates: g must be a contiguous \[3, 3, 128\]"):
        gru.gates(torch.zeros((3, 128)), net, inp, corr, flow)
    with pytest.raises(RuntimeError, match="conv_gru.gates: net " + cpu):
        gru.gates(g, net, inp, corr, flow)
    with pytest.raises(RuntimeError, match="conv_gru.update: z must be float16"):
        gru.update(g, net.float(), net, net, inp, corr, flow)
    with pytest.raises(RuntimeError, match="conv_gru.update: rnet must be contiguous and of net's shape"):
        gru.update(g, net, wide[:, :128], net, inp, corr, flow)
    with pytest.raises(RuntimeError, match="conv_gru.update: net " + cpu):
        gru.update(g, h(3, 128, 6, 8), h(3, 128, 6, 8), net, inp, corr, flow)
