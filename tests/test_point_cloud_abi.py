"""CPU-side checks of the point-cloud entry points: the symbols are exported and listed, the Python name is public,
every host-side refusal answers DROID_E_ARG with the function's name and the offending argument before any HIP call (so
none of this needs a GPU: the pointers are fake and never dereferenced), sizes are checked before pointers, an empty call
returns 0 without pointers, and the Python wrapper refuses what the contract excludes."""
import ctypes

import pytest
import torch

DROID_OK, DROID_E_ARG = 0, -1
# fake, non-null, 1 GiB apart: the largest array of the default call (images, 9 * 3 * 64 * 48 * 64 bytes) is 5 MiB
POSES, DISPS, INTR, INDEX, THRESH, IMAGES, POINTS, COLORS, SRC, OFFSETS, MATRICES, WS = (0x40000000 * k for k in range(1, 13))
N, NBUF, H, W = 13, 9, 48, 64
HW = H * W


def _ws_bytes(lib, n=N, h=H, w=W):
    return lib.droid_point_cloud_workspace_bytes(n, h, w)


def _call(lib, poses=POSES, disps=DISPS, intr=INTR, index=INDEX, thresh=THRESH, images=IMAGES, n=N, nbuf=NBUF, h=H, w=W,
          min_count=2, ratio=0.5, points=POINTS, colors=COLORS, src=SRC, offsets=OFFSETS, matrices=MATRICES, ws=WS,
          ws_bytes=None):
    if ws_bytes is None:
        ws_bytes = 1 << 40
    return lib.droid_point_cloud(poses, disps, intr, index, thresh, images, n, nbuf, h, w, min_count, ratio, points, colors,
                                 src, offsets, matrices, ws, ws_bytes, None)


def test_symbols_are_exported_and_listed(backends):
    lib = ctypes.CDLL(backends._lib.LIB_PATH)
    for sym in ("droid_point_cloud", "droid_point_cloud_workspace_bytes"):
        assert hasattr(lib, sym) and sym in backends._lib.SYMBOLS
    assert backends._lib.load().droid_abi_version() == 1   # adding symbols keeps the ABI version
    assert "point_cloud" in backends.__all__ and callable(backends.point_cloud)


def test_workspace_query(backends):
    lib = backends._lib.load()
    assert _ws_bytes(lib) == N * 12 * 36                      # 36 bytes per 256-pixel tile
    assert _ws_bytes(lib, 1, 1, 1) == 36 and _ws_bytes(lib, 2, 9, 19) == 72 and _ws_bytes(lib, 1, 31, 41) == 5 * 36
    assert _ws_bytes(lib, 0, 8, 8) == 0
    for bad in ((-1, 8, 8), (4, 0, 8), (4, 8, -2), (2 ** 31 - 1, 2, 1), (65536, 256, 128)):
        assert _ws_bytes(lib, *bad) == 0 and b"point_cloud" in lib.droid_last_error()


@pytest.mark.parametrize("kw,word", [
    (dict(n=-1), b"bad n"), (dict(n=-2 ** 31), b"bad n"),
    (dict(h=0), b"map size"), (dict(w=0), b"map size"), (dict(h=-3), b"map size"),
    (dict(n=2 ** 31 // HW + 1), b"n * H * W"), (dict(n=1, h=2 ** 16, w=2 ** 15), b"n * H * W"),
    (dict(n=2 ** 20, h=2 ** 6, w=2 ** 5), b"n * H * W"), (dict(n=2 ** 31 - 1, h=2 ** 31 - 1, w=2 ** 31 - 1), b"n * H * W"),
    (dict(nbuf=0), b"bad nbuf"), (dict(nbuf=-1), b"bad nbuf"),
    (dict(poses=None), b"null pointer"), (dict(disps=None), b"null pointer"), (dict(intr=None), b"null pointer"),
    (dict(index=None), b"null pointer"), (dict(thresh=None), b"null pointer"),
    (dict(points=None), b"null pointer"), (dict(src=None), b"null pointer"), (dict(offsets=None), b"null pointer"),
    (dict(matrices=None), b"null pointer"),
    (dict(images=None), b"images and colors"), (dict(colors=None), b"images and colors"),
    (dict(ws=None), b"null workspace"), (dict(ws_bytes=0), b"workspace too small"),
    (dict(ws_bytes=N * 12 * 36 - 1), b"workspace too small"), (dict(ws=WS + 4), b"8-byte aligned"),
    # outputs on inputs: first and last byte
    (dict(points=POSES), b"points overlaps poses"), (dict(points=POSES + NBUF * 28 - 4), b"points overlaps poses"),
    (dict(points=DISPS - N * HW * 12 + 4), b"points overlaps disps"), (dict(colors=DISPS + NBUF * HW * 4 - 4), b"colors overlaps disps"),
    (dict(src=INTR + 12), b"src overlaps intrinsics"), (dict(offsets=INDEX + N * 8 - 4), b"offsets overlaps index"),
    (dict(offsets=INDEX - (N + 1) * 4 + 4), b"offsets overlaps index"), (dict(matrices=THRESH), b"matrices overlaps thresh"),
    (dict(colors=IMAGES + NBUF * 192 * HW - 1), b"colors overlaps images"), (dict(ws=DISPS + 8), b"workspace overlaps disps"),
    # outputs on each other
    (dict(colors=POINTS), b"colors overlaps points"), (dict(colors=POINTS + N * HW * 12 - 4), b"colors overlaps points"),
    (dict(src=POINTS + 4), b"src overlaps points"), (dict(offsets=SRC + N * HW * 4 - 4), b"offsets overlaps src"),
    (dict(matrices=OFFSETS + N * 4), b"matrices overlaps offsets"), (dict(ws=MATRICES + N * 64 - 8), b"workspace overlaps matrices"),
    (dict(ws=POINTS - N * 12 * 36 + 8), b"workspace overlaps points"),
])
def test_refusals_need_no_gpu(backends, kw, word):
    lib = backends._lib.load()
    assert _call(lib, **kw) == DROID_E_ARG
    msg = lib.droid_last_error()
    assert b"point_cloud" in msg and word in msg, msg


def test_sizes_come_before_pointers(backends):
    lib = backends._lib.load()
    nothing = dict(poses=None, disps=None, intr=None, index=None, thresh=None, images=None, points=None, colors=None, src=None,
                   offsets=None, matrices=None, ws=None, ws_bytes=0)
    assert _call(lib, n=-1, **nothing) == DROID_E_ARG and b"bad n" in lib.droid_last_error()
    assert _call(lib, h=0, **nothing) == DROID_E_ARG and b"map size" in lib.droid_last_error()
    assert _call(lib, n=2 ** 20, **nothing) == DROID_E_ARG and b"n * H * W" in lib.droid_last_error()
    assert _call(lib, nbuf=0, **nothing) == DROID_E_ARG and b"bad nbuf" in lib.droid_last_error()
    assert _call(lib, **nothing) == DROID_E_ARG and b"null pointer" in lib.droid_last_error()
    # pointers before the workspace, the workspace before overlaps
    assert _call(lib, ws=None, points=POSES) == DROID_E_ARG and b"null workspace" in lib.droid_last_error()


def test_empty_call_returns_ok_without_pointers(backends):
    lib = backends._lib.load()
    nothing = dict(poses=None, disps=None, intr=None, index=None, thresh=None, images=None, points=None, colors=None, src=None,
                   offsets=None, matrices=None, ws=None, ws_bytes=0)
    assert _call(lib, n=0, **nothing) == DROID_OK
    assert _call(lib, n=0, h=1, w=1, **nothing) == DROID_OK


def test_python_refusals(backends):
    pc = backends.point_cloud
    poses = torch.zeros((9, 7))
    poses[:, 6] = 1
    disps, K = torch.ones((9, 6, 8)), torch.tensor([8.0, 8.0, 3.5, 2.5])
    index, images = torch.tensor([0, 3, 5]), torch.zeros((9, 3, 48, 64), dtype=torch.uint8)
    with pytest.raises(RuntimeError, match="point_cloud: poses must be a HIP .*no CPU path"):   # refused, not emulated
        pc(poses, disps, K, index, 0.1, images)
    with pytest.raises(RuntimeError, match="point_cloud: poses must be float32"):
        pc(poses.double(), disps, K, index, 0.1)
    with pytest.raises(RuntimeError, match="point_cloud: disps must be float32"):
        pc(poses, disps.half(), K, index, 0.1)
    with pytest.raises(RuntimeError, match="point_cloud: intrinsics must be float32"):
        pc(poses, disps, K.double(), index, 0.1)
    with pytest.raises(RuntimeError, match="point_cloud: index must be int64"):
        pc(poses, disps, K, index.int(), 0.1)
    with pytest.raises(RuntimeError, match="point_cloud: thresh must be float32"):
        pc(poses, disps, K, index, torch.full((3,), 0.1, dtype=torch.float64))
    with pytest.raises(RuntimeError, match="point_cloud: images must be uint8"):
        pc(poses, disps, K, index, 0.1, images.float())
    with pytest.raises(TypeError, match="point_cloud: index must be a tensor"):
        pc(poses, disps, K, [0, 3, 5], 0.1)
    with pytest.raises(RuntimeError, match=r"point_cloud: poses must be \[nbuf, 7\]"):
        pc(poses[:, :6].contiguous(), disps, K, index, 0.1)
    with pytest.raises(RuntimeError, match=r"point_cloud: poses must be \[nbuf, 7\]"):
        pc(poses, disps[0], K, index, 0.1)
    with pytest.raises(RuntimeError, match=r"point_cloud: poses must be \[nbuf, 7\]"):
        pc(poses, disps, torch.ones((9, 4)), index, 0.1)
    with pytest.raises(RuntimeError, match=r"point_cloud: index must be \[n\]"):
        pc(poses, disps, K, index[None], 0.1)
    with pytest.raises(RuntimeError, match=r"point_cloud: thresh must be a number or \[n\] = \[3\]"):
        pc(poses, disps, K, index, torch.full((4,), 0.1))
    for bad in (images[:8], images[:, :2], images[:, :, :47], torch.zeros((9, 3, 64, 48), dtype=torch.uint8),
                torch.zeros((9, 3, 6, 8), dtype=torch.uint8), images[0]):
        with pytest.raises(RuntimeError, match=r"point_cloud: images must be \[9, 3, 48, 64\]"):
            pc(poses, disps, K, index, 0.1, bad.contiguous())
    with pytest.raises(RuntimeError, match="point_cloud: disps must be contiguous"):
        pc(poses, torch.ones((9, 8, 6)).transpose(1, 2), K, index, 0.1)
    with pytest.raises(RuntimeError, match="point_cloud: poses must be contiguous"):
        pc(torch.zeros((7, 9)).t(), disps, K, index, 0.1)
    with pytest.raises(RuntimeError, match="point_cloud: index must be contiguous"):
        pc(poses, disps, K, torch.arange(6)[::2], 0.1)
    with pytest.raises(RuntimeError, match="point_cloud: images must be contiguous"):
        pc(poses, disps, K, index, 0.1, torch.zeros((9, 3, 64, 48), dtype=torch.uint8).transpose(2, 3))
