"""CPU-side checks of the pose-algebra entry points: the symbols are exported and listed, the Python names are public,
every host-side refusal answers DROID_E_ARG with the function's name and the offending argument before any HIP call (so
none of this needs a GPU: the pointers are fake and never dereferenced), empty calls return 0, and the Python wrappers
refuse what the contract excludes."""
import ctypes

import pytest
import torch

DROID_OK, DROID_E_ARG = 0, -1
INV, LOG, EXP, MATRIX = 0, 1, 2, 3
A, B, OUT, K0, K1, TS, Q = (0x10000000 * k for k in range(1, 8))   # fake, non-null, 256 MiB apart
BIG = 2 ** 31 - 1


def _unary(lib, in_=A, out=OUT, n=9, op=INV):
    return lib.droid_se3_unary(in_, out, n, op, None)


def _mul(lib, a=A, sa=7, b=B, sb=7, out=OUT, n=9):
    return lib.droid_se3_mul(a, sa, b, sb, out, n, None)


def _interp(lib, poses=A, ts=TS, N=5, query=Q, M=8, out=OUT, k0=K0, k1=K1):
    return lib.droid_pose_interpolate(poses, ts, N, query, M, out, k0, k1, None)


def test_symbols_are_exported_and_listed(backends):
    lib = ctypes.CDLL(backends._lib.LIB_PATH)
    for sym in ("droid_se3_unary", "droid_se3_mul", "droid_pose_interpolate"):
        assert hasattr(lib, sym) and sym in backends._lib.SYMBOLS
    assert backends._lib.load().droid_abi_version() == 1   # adding symbols keeps the ABI version
    for name in ("SE3", "pose_interpolate"):
        assert name in backends.__all__ and callable(getattr(backends, name))
    from droid_backends import se3
    for name in ("SE3", "cat", "interpolate"):
        assert name in se3.__all__ and callable(getattr(se3, name))
    assert backends.pose_interpolate is se3.interpolate and backends.SE3 is se3.SE3


@pytest.mark.parametrize("kw,word", [
    (dict(op=-1), b"bad op"), (dict(op=4), b"bad op"), (dict(op=BIG), b"bad op"),
    (dict(n=-1), b"bad n"), (dict(n=-2 ** 62), b"bad n"),
    (dict(n=2 ** 58 + 1), b"n * 16"), (dict(n=2 ** 63 - 1, op=MATRIX), b"n * 16"),
    (dict(in_=None), b"null pointer"), (dict(out=None), b"null pointer"), (dict(in_=None, out=None, n=1), b"null pointer"),
    (dict(out=A, op=LOG), b"out overlaps in"), (dict(out=A, op=EXP), b"out overlaps in"),
    (dict(out=A, op=MATRIX), b"out overlaps in"),
    (dict(out=A + 28, op=INV), b"out overlaps in"), (dict(out=A - 28, op=INV), b"out overlaps in"),
    (dict(out=A + 4 * 7 * 9 - 4, op=INV), b"out overlaps in"),       # the last float of in
    (dict(out=A - 4 * 16 * 9 + 4, op=MATRIX), b"out overlaps in"),   # the last float of out on the first of in
])
def test_unary_refusals_need_no_gpu(backends, kw, word):
    lib = backends._lib.load()
    assert _unary(lib, **kw) == DROID_E_ARG
    msg = lib.droid_last_error()
    assert b"se3_unary" in msg and word in msg, msg


@pytest.mark.parametrize("kw,word", [
    (dict(sa=1), b"stride_a"), (dict(sa=-7), b"stride_a"), (dict(sa=6), b"stride_a"), (dict(sa=14), b"stride_a"),
    (dict(sb=1), b"stride_b"), (dict(sb=8), b"stride_b"),
    (dict(n=-1), b"bad n"), (dict(n=2 ** 58 + 1), b"n * 16"),
    (dict(a=None), b"null pointer"), (dict(b=None), b"null pointer"), (dict(out=None), b"null pointer"),
    (dict(out=A, sa=0), b"out overlaps a"), (dict(out=B, sb=0), b"out overlaps b"),     # a broadcast record is read by all
    (dict(out=A + 28), b"out overlaps a"), (dict(out=B - 28), b"out overlaps b"),
    (dict(out=A - 4 * 7 * 9 + 4, sa=0), b"out overlaps a"),
])
def test_mul_refusals_need_no_gpu(backends, kw, word):
    lib = backends._lib.load()
    assert _mul(lib, **kw) == DROID_E_ARG
    msg = lib.droid_last_error()
    assert b"se3_mul" in msg and word in msg, msg


@pytest.mark.parametrize("kw,word", [
    (dict(N=0), b"bad N"), (dict(N=-1), b"bad N"), (dict(N=0, M=0), b"bad N"),
    (dict(M=-1), b"bad M"),
    (dict(poses=None), b"null pointer"), (dict(ts=None), b"null pointer"), (dict(query=None), b"null pointer"),
    (dict(out=None), b"null pointer"),
    (dict(out=A), b"out overlaps"), (dict(out=TS), b"out overlaps"), (dict(out=Q), b"out overlaps"),
    (dict(out=A + 4 * 7 * 5 - 4), b"out overlaps"), (dict(out=Q - 4 * 7 * 8 + 4), b"out overlaps"),
    (dict(k0=A), b"k0_out overlaps"), (dict(k0=Q + 28), b"k0_out overlaps"), (dict(k1=TS), b"k1_out overlaps"),
    (dict(k1=TS - 8 * 8 + 4), b"k1_out overlaps"),
])
def test_interpolate_refusals_need_no_gpu(backends, kw, word):
    lib = backends._lib.load()
    assert _interp(lib, **kw) == DROID_E_ARG
    msg = lib.droid_last_error()
    assert b"pose_interpolate" in msg and word in msg, msg


def test_sizes_come_before_pointers(backends):
    lib = backends._lib.load()
    assert _unary(lib, in_=None, out=None, op=9) == DROID_E_ARG and b"bad op" in lib.droid_last_error()
    assert _unary(lib, in_=None, out=None, n=-3) == DROID_E_ARG and b"bad n" in lib.droid_last_error()
    assert _mul(lib, a=None, b=None, out=None, sa=3) == DROID_E_ARG and b"stride_a" in lib.droid_last_error()
    assert _interp(lib, poses=None, ts=None, query=None, out=None, N=0) == DROID_E_ARG and b"bad N" in lib.droid_last_error()


def test_empty_calls_return_ok_without_pointers(backends):
    lib = backends._lib.load()
    for op in (INV, LOG, EXP, MATRIX):
        assert _unary(lib, in_=None, out=None, n=0, op=op) == DROID_OK
    assert _mul(lib, a=None, b=None, out=None, n=0) == DROID_OK
    assert _mul(lib, a=None, sa=0, b=None, sb=0, out=None, n=0) == DROID_OK
    assert _interp(lib, poses=None, ts=None, query=None, out=None, k0=None, k1=None, M=0) == DROID_OK


def test_python_refusals(backends):
    from droid_backends import se3
    SE3 = backends.SE3
    rec = torch.zeros((4, 7))
    rec[:, 6] = 1
    for call, name in ((lambda: SE3(rec).inv(), "SE3.inv"), (lambda: SE3(rec).log(), "SE3.log"),
                       (lambda: SE3(rec).matrix(), "SE3.matrix"), (lambda: SE3(rec) * SE3(rec), "SE3.__mul__"),
                       (lambda: SE3.exp(torch.zeros((4, 6))), "SE3.exp"),
                       (lambda: backends.pose_interpolate(rec, torch.arange(4.0), 4, [1.5]), "pose_interpolate"),
                       (lambda: se3.interpolate(SE3(rec), torch.arange(4.0), 4, [1.5]), "pose_interpolate")):
        with pytest.raises(RuntimeError, match=name + ": .*no CPU path"):   # CPU tensors are refused, not emulated
            call()
    with pytest.raises(RuntimeError, match="SE3: data must be float32"):
        SE3(rec.double())
    with pytest.raises(RuntimeError, match="SE3: data must be float32"):
        SE3(rec.half())
    with pytest.raises(RuntimeError, match=r"SE3: data must be \[\.\.\., 7\]"):
        SE3(torch.zeros((4, 6)))
    with pytest.raises(TypeError, match="SE3: data must be a tensor"):
        SE3([0, 0, 0, 0, 0, 0, 1])
    with pytest.raises(RuntimeError, match="SE3.exp: xi must be float32"):
        SE3.exp(torch.zeros((4, 6), dtype=torch.float64))
    with pytest.raises(RuntimeError, match=r"SE3.exp: xi must be \[\.\.\., 6\]"):
        SE3.exp(rec)
    for other in (torch.zeros((4, 3)), torch.zeros((4, 4)), 2.0):
        with pytest.raises(TypeError, match="droid_backends.reproject and droid_backends.iproj"):
            SE3(rec) * other
    with pytest.raises(TypeError):
        torch.zeros((4, 7)) * SE3(rec)
    with pytest.raises(RuntimeError, match="pose_interpolate: poses must be float32"):
        backends.pose_interpolate(rec.double(), torch.arange(4.0), 4, [1.5])
    with pytest.raises(RuntimeError, match="pose_interpolate: tstamp must be a float32 tensor"):
        backends.pose_interpolate(rec, torch.arange(4.0).double(), 4, [1.5])
    with pytest.raises(TypeError, match="cat: a non-empty list of SE3"):
        se3.cat([])
    with pytest.raises(TypeError, match="cat: a non-empty list of SE3"):
        se3.cat([rec])


def test_host_side_conveniences(backends):
    """Pure torch, no device: Identity (motion_filter.py:55 builds it on the host), wrapping, indexing, cat, len."""
    from droid_backends import se3
    SE3 = backends.SE3
    Id = SE3.Identity(1,)
    assert Id.data.device.type == "cpu" and Id.data.dtype == torch.float32
    assert Id.data.squeeze().tolist() == [0, 0, 0, 0, 0, 0, 1] and tuple(Id.shape) == (1,) and len(Id) == 1
    assert tuple(SE3.Identity(2, 3).shape) == (2, 3) and tuple(SE3.Identity((2, 3)).data.shape) == (2, 3, 7)
    assert SE3.Identity(1, dtype=torch.float64).data.dtype == torch.float64
    data = torch.arange(6 * 7, dtype=torch.float32).view(2, 3, 7)
    P = SE3(data)
    assert P.data.data_ptr() == data.data_ptr()                 # contiguous: wrapped, not copied
    assert SE3(data.transpose(0, 1)).data.is_contiguous()       # otherwise made contiguous
    assert tuple(P.shape) == (2, 3) and P.device == data.device and len(P) == 2
    assert torch.equal(P[1].data, data[1]) and torch.equal(P[:, 2].data, data[:, 2])
    assert torch.equal(P[..., 0].data, data[:, 0]) and torch.equal(P[1, 2].data, data[1, 2])
    assert torch.equal(P[torch.tensor([1, 0])].data, data[[1, 0]])
    assert torch.equal(P[torch.tensor([[True, False, True], [False, False, True]])].data, data[[0, 0, 1], [0, 2, 2]])
    with pytest.raises(IndexError):
        P[0, 0, 0]                                              # the record dimension is not indexed
    assert torch.equal(se3.cat([P, P], 0).data, torch.cat([data, data], 0))
    assert torch.equal(se3.cat([P, P], 1).data, torch.cat([data, data], 1))
    assert torch.equal(se3.cat([P, P], -1).data, torch.cat([data, data], 1))
    with pytest.raises(IndexError):
        se3.cat([P, P], 2)
