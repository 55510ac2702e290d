"""numpy restatement of droid_corr_encode (include/droid_update_hip.h): from the lookup values `a` (half values, any
float array that holds them) and the fp32 parameters of corr_encoder[0],

    s = sum_k a[e,k,p] * w16[n,k] + b16[n]          in float64 -- exact products, one rounding per addition at 2^-53
    S = sum_k |a[e,k,p] * w16[n,k]| + |b16[n]|

and the bound the device is held to around relu(s): fp32 accumulation of the 196 exact products and the bias in ANY
order (the project's form, corr_cases.forward_bound: (terms + 2) * 2^-24 * S), the one rounding to half
(2^-11 * |relu(s)|, relative half-ulp) and 2^-25 for results in the subnormal range of half (half an ulp there).
The packed weight layout of the header is restated here too (`pack`, `unpack`), independent of the package's packer."""
import numpy as np

LEVELS, K, KP, N = 4, 49, 64, 128
KTOT = LEVELS * K          # 196
PACKED_HALVES = LEVELS * KP * N + N


def half(x):
    """autocast's cast: fp32 -> half, round to nearest even, overflow to inf."""
    with np.errstate(over="ignore"):
        return np.asarray(x, dtype=np.float32).astype(np.float16)


def sums(a, weight, bias):
    """a [E,196,...] half values; weight [128,196] fp32, bias [128] fp32.  Returns (s, S) as float64 [E,128,...]."""
    a64 = np.asarray(a).astype(np.float64)
    flat = a64.reshape(a64.shape[0], KTOT, -1)
    w64 = half(np.asarray(weight).reshape(N, KTOT)).astype(np.float64)
    b64 = half(bias).astype(np.float64)
    with np.errstate(invalid="ignore", over="ignore"):
        s = np.matmul(w64, flat) + b64[None, :, None]
        S = np.matmul(np.abs(w64), np.abs(flat)) + np.abs(b64)[None, :, None]
    shape = (a64.shape[0], N) + a64.shape[2:]
    return s.reshape(shape), S.reshape(shape)


def relu(s):
    return np.where(s > 0, s, 0.0)


def bound(s, S):
    return (KTOT + 2) * 2.0 ** -24 * S + 2.0 ** -11 * np.abs(relu(s)) + 2.0 ** -25


def finite_mask(a):
    """[E,1,...] bool: True where every one of the 196 values of a pixel is finite (the only exclusion of the product
    test: an fp32 lookup value that overflowed to inf in half)."""
    return np.isfinite(np.asarray(a).astype(np.float64)).all(axis=1, keepdims=True)


def pack(weight, bias):
    """The packed buffer of the header as a flat float16 array: [4 levels][2 K steps][8 channel tiles][64 lanes][8]
    then b16 [128]; element (l, s, nt, lane, j) = w16[16 nt + (lane & 15)][49 l + 32 s + 8 (lane >> 4) + j], zero where
    32 s + 8 (lane >> 4) + j >= 49."""
    w16 = half(np.asarray(weight).reshape(N, KTOT))
    out = np.zeros((LEVELS, 2, 8, 64, 8), np.float16)
    for l in range(LEVELS):
        for s in range(2):
            for lane in range(64):
                for j in range(8):
                    kk = 32 * s + 8 * (lane >> 4) + j
                    if kk < K:
                        out[l, s, :, lane, j] = w16[16 * np.arange(8) + (lane & 15), K * l + kk]
    return np.concatenate([out.reshape(-1), half(bias)])


def padding_mask():
    """bool [PACKED_HALVES]: True at the padded K entries of the packed weights."""
    kk = (32 * np.arange(2)[:, None, None, None] + 8 * (np.arange(64) >> 4)[None, None, :, None]
          + np.arange(8)[None, None, None, :])
    m = np.broadcast_to(kk >= K, (LEVELS, 2, 8, 64, 8)).reshape(-1)
    return np.concatenate([m, np.zeros(N, bool)])


def unpack(packed):
    """(w16 [128,196], b16 [128]) read back from a packed buffer."""
    packed = np.asarray(packed)
    body = packed[:LEVELS * KP * N].reshape(LEVELS, 2, 8, 64, 8)
    w16 = np.zeros((N, KTOT), np.float16)
    for l in range(LEVELS):
        for kk in range(K):
            s, g, j = kk // 32, (kk % 32) // 8, kk % 8
            for c in range(16):
                w16[16 * np.arange(8) + c, K * l + kk] = body[l, s, :, 16 * g + c, j]
    return w16, packed[LEVELS * KP * N:]
