"""The contract of droid_conv3x3 (include/droid_conv3x3_hip.h) restated in numpy for the tests: the convolution with an
fp64 sum, the one rounding to half and the activation; the packed layout; the case tables.  Restated from the header:
nothing here imports the package."""
import numpy as np

# (h, w, B): the smallest maps at which the kernel can go wrong (tests/test_gpu_conv3x3.py says what each one catches)
MAPS = [(1, 1, 1), (1, 2, 2), (3, 3, 3), (8, 8, 5), (2, 64, 2), (5, 9, 2), (11, 13, 3), (9, 70, 1), (30, 40, 1), (48, 64, 1)]
# (C_in, C_out of a layer, layers of one launch)
CHANNELS = [(32, 64, 1), (64, 128, 1), (128, 128, 1), (128, 64, 1), (128, 128, 2)]
GRU_CHANNELS = (448, 128, 1)          # the ConvGRU's input width, on the maps up to 11 x 13
PACK_SIZES = [(32, 64), (128, 128), (128, 64), (128, 256), (448, 128)]
BOUND_SEED = 20240


def cases():
    """Every (C_in, C_out, layers, h, w, B) of the tables."""
    out = [(ci, co, k, h, w, B) for ci, co, k in CHANNELS for h, w, B in MAPS]
    return out + [GRU_CHANNELS + (h, w, B) for h, w, B in MAPS if h * w <= 11 * 13]


def case_id(c):
    return "%dto%dx%d-%dx%d-B%d" % (c[0], c[2], c[1], c[3], c[4], c[5])


def window(x):
    """[B,C,H,W] -> [B,H,W,9 C]: the zero-padded 3 x 3 window of every pixel, ordered k = 9 c + 3 ky + kx."""
    B, C, H, W = x.shape
    p = np.zeros((B, C, H + 2, W + 2), dtype=x.dtype)
    p[:, :, 1:-1, 1:-1] = x
    taps = [p[:, :, ky:ky + H, kx:kx + W] for ky in range(3) for kx in range(3)]       # 9 x [B,C,H,W]
    return np.stack(taps, axis=2).transpose(0, 3, 4, 1, 2).reshape(B, H, W, 9 * C)


def act(y16, relu):
    """max(., 0) that keeps a NaN and gives +0 for everything not above zero; the identity without relu."""
    if not relu:
        return y16
    return np.where((y16 > 0) | np.isnan(y16), y16, np.float16(0)).astype(np.float16)


def exact(x16, w16, b16):
    """(s, mag): the fp64 value sum x * w16 + b16 before the rounding, and sum |x * w16|, both [B,N,H,W]."""
    n = w16.shape[0]
    a = window(x16.astype(np.float64))
    wm = w16.astype(np.float64).reshape(n, -1).T
    s = a @ wm + b16.astype(np.float64)
    mag = np.abs(a) @ np.abs(wm)
    return s.transpose(0, 3, 1, 2), mag.transpose(0, 3, 1, 2)


def conv(x16, w16, b16, relu=True):
    """The contract: half in, half out."""
    with np.errstate(over="ignore", invalid="ignore"):
        return act(exact(x16, w16, b16)[0].astype(np.float16), relu)


def bound(c_in, s, mag):
    """The accumulation bound of the contract's arithmetic around the fp64 value s: 9 C_in exact products and the bias
    summed in fp32 in any order, gamma_K <= (K + 2) u for K <= 4608, then one rounding to half (2^-11 relative) and half
    of half's smallest subnormal step."""
    return (9 * c_in + 2) * 2.0 ** -24 * mag + 2.0 ** -11 * np.abs(s) + 2.0 ** -25


def packed_halves(c_in, c_out):
    return 9 * c_in * c_out + c_out


def pack(w16, b16):
    """halves [C_in / 32][9][C_out / 16][64][8] + b16 [C_out]; element (s, t, nt, lane, j) is
    w16[16 nt + (lane & 15)][32 s + 8 (lane >> 4) + j][t / 3][t % 3]."""
    n, c = w16.shape[:2]
    out = np.empty((c // 32, 9, n // 16, 64, 8), dtype=np.float16)
    lane = np.arange(64)
    for s in range(c // 32):
        for t in range(9):
            for nt in range(n // 16):
                for j in range(8):
                    out[s, t, nt, :, j] = w16[16 * nt + (lane & 15), 32 * s + 8 * (lane >> 4) + j, t // 3, t % 3]
    return np.concatenate([out.reshape(-1), b16.astype(np.float16)])


def unpack(packed, c_in, c_out):
    """The inverse of `pack`: (w16 [C_out,C_in,3,3], b16 [C_out])."""
    body = packed[:9 * c_in * c_out].reshape(c_in // 32, 9, c_out // 16, 4, 16, 8)      # (s, t, nt, g, c16, j)
    w = body.transpose(2, 4, 0, 3, 5, 1).reshape(c_out, c_in, 3, 3)                        # (nt, c16, s, g, j, t)
    return np.ascontiguousarray(w), packed[9 * c_in * c_out:]


def operands(seed, c_in, c_out, h, w, B, scale=1.0):
    """Random half operands of a layer: x ~ N(0, 1), w ~ N(0, 1 / sqrt(9 C_in)), b ~ N(0, 0.5): outputs of order one,
    on both sides of zero."""
    rng = np.random.default_rng(seed)
    x = rng.normal(0, scale, (B, c_in, h, w)).astype(np.float16)
    wt = rng.normal(0, 1 / np.sqrt(9 * c_in), (c_out, c_in, 3, 3)).astype(np.float16)
    b = rng.normal(0, 0.5, (c_out,)).astype(np.float16)
    return x, wt, b
