"""numpy restatement of droid_motion_encode (include/droid_motion_encode_hip.h): from the motion planes m [E,4,H,W] and
the fp32 parameters of flow_encoder[0] ([128,4,7,7], [128]),

    a = half(m), zero outside the image                                   (autocast's cast, padding=3)
    s = sum_{c,ky,kx} a[e,c,v+ky-3,u+kx-3] * w16[n,c,ky,kx] + b16[n]      in float64 -- exact products, 2^-53 per addition
    S = sum |a * w16| + |b16[n]|

and the bound the device is held to around relu(s), the one of tests/corr_encode_ref.py: fp32 accumulation of the 196
exact products and the bias in ANY order ((196 + 2) * 2^-24 * S), the one rounding to half (2^-11 * |relu(s)|) and 2^-25
for results in the subnormal range of half.  The packed layout of the header is restated here (`pack`, `unpack`),
independent of the package's packer.  The geometry is oracle/geom.py's motion_features, imported; `scene` builds the
inputs of the shapes the tests share."""
import functools

import numpy as np

import geom_cases as gc
from oracle import geom

CHANNELS, KS, K, KP, N = 4, 7, 49, 64, 128
KTOT = CHANNELS * K          # 196
PACKED_HALVES = CHANNELS * KP * N + N
# (H, W, E): every tap but the centre is padding | the map is smaller than the halo | one wave, a window crosses all four
# borders | ragged, a wave's pixels wrap over rows, element-wise stores | W > 64: a wave boundary inside a row | a tail
# workgroup | the real plane, all 16-byte stores
SHAPES = [(1, 1, 1), (3, 5, 2), (8, 8, 3), (11, 13, 3), (9, 70, 2), (30, 40, 3), (48, 64, 5)]
NBUF = 6
BAD_INDEX = (-1, 2 ** 32 + 3)


def half(x):
    """autocast's cast: fp32 -> half, round to nearest even, overflow to inf."""
    with np.errstate(over="ignore"):
        return np.asarray(x, dtype=np.float32).astype(np.float16)


def operand(m):
    """a [E,4,H+6,W+6] float64: the half values of m inside a frame of three zeros (padding=3)."""
    a = half(m).astype(np.float64)
    return np.pad(a, [(0, 0), (0, 0), (3, 3), (3, 3)])


def windows(m):
    """[E,196,H,W] float64: column k = 49 c + 7 ky + kx holds a[e, c, v + ky - 3, u + kx - 3]."""
    ap = operand(m)
    E, _, Hp, Wp = ap.shape
    H, W = Hp - 6, Wp - 6
    out = np.empty((E, KTOT, H, W))
    for c in range(CHANNELS):
        for ky in range(KS):
            for kx in range(KS):
                out[:, K * c + KS * ky + kx] = ap[:, c, ky:ky + H, kx:kx + W]
    return out


def sums(m, weight, bias):
    """m [E,4,H,W] fp32 values; weight [128,4,7,7], bias [128] fp32.  Returns (s, S) as float64 [E,128,H,W]."""
    win = windows(m)
    E, _, H, W = win.shape
    flat = win.reshape(E, KTOT, H * W)
    w64 = half(np.asarray(weight).reshape(N, KTOT)).astype(np.float64)
    b64 = half(bias).astype(np.float64)
    s = np.matmul(w64, flat) + b64[None, :, None]
    S = np.matmul(np.abs(w64), np.abs(flat)) + np.abs(b64)[None, :, None]
    return s.reshape(E, N, H, W), S.reshape(E, N, H, W)


def relu(s):
    return np.where(s > 0, s, 0.0)


def bound(s, S):
    return (KTOT + 2) * 2.0 ** -24 * S + 2.0 ** -11 * np.abs(relu(s)) + 2.0 ** -25


def pack(weight, bias):
    """The packed buffer of the header as a flat float16 array: [4 channels][2 K steps][8 channel tiles][64 lanes][8]
    then b16 [128]; element (c, s, nt, lane, j) = w16[16 nt + (lane & 15)][c][kk // 7][kk % 7],
    kk = 32 s + 8 (lane >> 4) + j, zero where kk >= 49."""
    w16 = half(np.asarray(weight).reshape(N, CHANNELS, KS, KS))
    out = np.zeros((CHANNELS, 2, 8, 64, 8), np.float16)
    for c in range(CHANNELS):
        for s in range(2):
            for lane in range(64):
                for j in range(8):
                    kk = 32 * s + 8 * (lane >> 4) + j
                    if kk < K:
                        out[c, s, :, lane, j] = w16[16 * np.arange(8) + (lane & 15), c, kk // KS, kk % KS]
    return np.concatenate([out.reshape(-1), half(bias)])


def padding_mask():
    """bool [PACKED_HALVES]: True at the padded K entries of the packed weights."""
    kk = (32 * np.arange(2)[:, None, None, None] + 8 * (np.arange(64) >> 4)[None, None, :, None]
          + np.arange(8)[None, None, None, :])
    m = np.broadcast_to(kk >= K, (CHANNELS, 2, 8, 64, 8)).reshape(-1)
    return np.concatenate([m, np.zeros(N, bool)])


def unpack(packed):
    """(w16 [128,4,7,7], b16 [128]) read back from a packed buffer."""
    packed = np.asarray(packed)
    body = packed[:CHANNELS * KP * N].reshape(CHANNELS, 2, 8, 64, 8)
    w16 = np.zeros((N, CHANNELS, KS, KS), np.float16)
    for c in range(CHANNELS):
        for kk in range(K):
            s, g, j = kk // 32, (kk % 32) // 8, kk % 8
            for c16 in range(16):
                w16[16 * np.arange(8) + c16, c, kk // KS, kk % KS] = body[c, s, :, 16 * g + c16, j]
    return w16, packed[CHANNELS * KP * N:]


def params(seed):
    """nn.Conv2d(4, 128, 7)'s default init: uniform in +-1/sqrt(fan_in) = 1/sqrt(196) for weight and bias (fp32)."""
    rng = np.random.default_rng(seed)
    k = 1.0 / np.sqrt(KTOT)
    w = rng.uniform(-k, k, (N, CHANNELS, KS, KS)).astype(np.float32)
    b = rng.uniform(-k, k, (N,)).astype(np.float32)
    return w, b


@functools.lru_cache(maxsize=None)
def scene(H, W, E):
    """The inputs of shape (H, W, E), float32 / int64, shared and never modified: six frames on a gentle trajectory,
    per-frame anisotropic intrinsics, edges (0 -> 1), one stereo edge, from E = 3 on one edge with an index outside the
    buffer, then (3 -> 4), (5 -> 0); target = the oracle's coords + noise, so that all four planes are non-zero.
    Returns a dict with poses, disps, intrinsics, ii, jj, target and `bad`, the list of edges outside the buffer."""
    rng = np.random.default_rng(1000 * H + 10 * W + E)
    poses = np.zeros((NBUF, 7))
    poses[:, :3] = rng.normal(0, 0.04, (NBUF, 3)) + 0.03 * np.arange(NBUF)[:, None] * np.array([1.0, 0.2, 0.1])
    q = np.concatenate([rng.normal(0, np.deg2rad(1.5), (NBUF, 3)), np.ones((NBUF, 1))], axis=1)
    poses[:, 3:] = q / np.linalg.norm(q, axis=1, keepdims=True)
    poses = poses.astype(np.float32)
    disps = rng.uniform(0.3, 2.0, (NBUF, H, W)).astype(np.float32)
    Ks = gc.aniso_K_frames(H, W, NBUF)
    bad_value = BAD_INDEX[(H + W) % 2]
    edges = [(0, 1), (2, 2), (bad_value, 3) if H % 2 else (4, bad_value), (3, 4), (5, 0)]
    if E == 1:
        edges = [(2, 2)]
    assert E <= len(edges)
    ii = np.array([e[0] for e in edges[:E]], np.int64)
    jj = np.array([e[1] for e in edges[:E]], np.int64)
    bad = [e for e in range(E) if not (0 <= ii[e] < NBUF and 0 <= jj[e] < NBUF)]
    live = [e for e in range(E) if e not in bad]
    coords = np.zeros((E, H, W, 2))
    coords[live], _ = geom.reproject(poses, disps, Ks, ii[live], jj[live])
    target = (coords + rng.normal(0, 2.0, coords.shape)).astype(np.float32)
    out = dict(poses=poses, disps=disps, intrinsics=Ks, ii=ii, jj=jj, target=target, bad=bad)
    for v in out.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def oracle_motion(H, W, E):
    """(motn [E,4,H,W], coords [E,H,W,2], valid [E,H,W,1]) of scene(H, W, E) in float64 from oracle/geom.py; zeros for
    an edge outside the buffer, as the operators write them."""
    sc = scene(H, W, E)
    live = [e for e in range(E) if e not in sc["bad"]]
    motn, coords, valid = np.zeros((E, 4, H, W)), np.zeros((E, H, W, 2)), np.zeros((E, H, W, 1))
    motn[live], coords[live], valid[live] = geom.motion_features(sc["poses"], sc["disps"], sc["intrinsics"], sc["ii"][live],
                                                                 sc["jj"][live], sc["target"][live])
    return motn, coords, valid
