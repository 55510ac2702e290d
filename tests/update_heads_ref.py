"""numpy restatement of droid_update_heads (include/droid_heads_hip.h): for one head, from x [B,128,H,W] half values
and the fp32 parameters of the layer ([n,128,3,3], [n], n in {1, 2}),

    t = sum_{c,ky,kx} x[b,c,v+ky-1,u+kx-1] * w16[n,c,ky,kx] + b16[n]      in float64, x = 0 outside the image
    S = sum |x * w16| + |b16[n]|
    y = act(t)                                                            in float64

and the bound the device is held to around y:
    L * (1152 + 2) * 2^-24 * S    fp32 accumulation of the 1152 exact products and the bias in ANY order, carried through
                                  the activation by its Lipschitz constant L (identity 1, sigmoid 1/4, softplus-centi 0.01)
  + 8 * 2^-24 * |y|               expf / log1pf / the division in fp32 (zero for the identity)
  + 2^-11 * |y|                   the ONE rounding to half
  + 2^-25                         results in the subnormal range of half.
The packed layout of the header is restated here (`pack`, `unpack`), independent of the package's packer.  Results are in
the layout of the device: [B,H,W,n]."""
import functools

import numpy as np

C, KS, TAPS = 128, 3, 9
KTOT = C * TAPS          # 1152
IDENTITY, SIGMOID, SOFTPLUS_CENTI = 0, 1, 2
LIPSCHITZ = {IDENTITY: 1.0, SIGMOID: 0.25, SOFTPLUS_CENTI: 0.01}
# (H, W, B): only the centre tap is inside the image | a map smaller than the halo | one tile touching all four borders |
# ragged, rows wrapping inside a wave | W > 64 | a tail workgroup | the real plane
SHAPES = [(1, 1, 1), (3, 5, 2), (8, 8, 3), (11, 13, 3), (9, 70, 2), (30, 40, 3), (48, 64, 5)]


def half(x):
    """autocast's cast: fp32 -> half, round to nearest even, overflow to inf."""
    with np.errstate(over="ignore"):
        return np.asarray(x, dtype=np.float32).astype(np.float16)


def packed_floats(n):
    return (KTOT * n + n + 3) // 4 * 4


def windows(x, mode="constant"):
    """[B,1152,H,W] float64: column k = 9 c + 3 ky + kx holds x[b, c, v + ky - 1, u + kx - 1] (zero outside)."""
    xp = np.pad(np.asarray(x).astype(np.float64), [(0, 0), (0, 0), (1, 1), (1, 1)], mode=mode)
    B, _, Hp, Wp = xp.shape
    H, W = Hp - 2, Wp - 2
    out = np.empty((B, KTOT, H, W))
    for c in range(C):
        for ky in range(KS):
            for kx in range(KS):
                out[:, TAPS * c + KS * ky + kx] = xp[:, c, ky:ky + H, kx:kx + W]
    return out


def sums(x, weight, bias, mode="constant", transpose_taps=False):
    """x [B,128,H,W] half values; weight [n,128,3,3], bias [n] fp32.  Returns (t, S) as float64 [B,H,W,n].  `mode` and
    `transpose_taps` build the WRONG restatements the CPU tests hold the bound against (edge replication instead of the
    zero padding; ky and kx exchanged)."""
    win = windows(x, mode)
    B, _, H, W = win.shape
    flat = win.reshape(B, KTOT, H * W)
    w16 = half(weight).astype(np.float64)
    if transpose_taps:
        w16 = w16.transpose(0, 1, 3, 2)
    n = w16.shape[0]
    w64 = w16.reshape(n, KTOT)
    b64 = half(bias).astype(np.float64)
    t = np.matmul(w64, flat) + b64[None, :, None]
    S = np.matmul(np.abs(w64), np.abs(flat)) + np.abs(b64)[None, :, None]
    to_device = lambda a: np.ascontiguousarray(a.reshape(B, n, H, W).transpose(0, 2, 3, 1))
    return to_device(t), to_device(S)


def act(kind, t):
    t = np.asarray(t, dtype=np.float64)
    if kind == IDENTITY:
        return t
    with np.errstate(over="ignore"):
        if kind == SIGMOID:
            return 1.0 / (1.0 + np.exp(-t))
        return 0.01 * np.where(t > 20.0, t, np.log1p(np.exp(np.minimum(t, 20.0))))


def bound(kind, t, S):
    y = np.abs(act(kind, t))
    return (LIPSCHITZ[kind] * (KTOT + 2) * 2.0 ** -24 * S + (0.0 if kind == IDENTITY else 8 * 2.0 ** -24) * y
            + 2.0 ** -11 * y + 2.0 ** -25)


def pack(weight, bias):
    """The packed buffer of the header as a flat float32 array: element ((c * 3 + ky) * 3 + kx) * n + j is
    float(w16[j][c][ky][kx]), element 1152 n + j is float(b16[j]), the rest (up to a multiple of four floats) zero."""
    w16, b16 = half(weight), half(bias)
    n = w16.shape[0]
    out = np.zeros(packed_floats(n), np.float32)
    for j in range(n):
        for c in range(C):
            for ky in range(KS):
                for kx in range(KS):
                    out[((c * 3 + ky) * 3 + kx) * n + j] = np.float32(w16[j, c, ky, kx])
        out[KTOT * n + j] = np.float32(b16[j])
    return out


def padding_mask(n):
    m = np.zeros(packed_floats(n), bool)
    m[(KTOT + 1) * n:] = True
    return m


def unpack(packed, n):
    """(w16 [n,128,3,3], b16 [n]) read back from a packed buffer of a head with n outputs."""
    packed = np.asarray(packed)
    w = packed[:KTOT * n].reshape(C, KS, KS, n).transpose(3, 0, 1, 2)
    return w.astype(np.float16), packed[KTOT * n:KTOT * n + n].astype(np.float16)


N_OUT = {IDENTITY: 2, SIGMOID: 2, SOFTPLUS_CENTI: 1}


def params(kind, seed):
    """nn.Conv2d(128, n, 3)'s default init: uniform in +-1/sqrt(fan_in) = 1/sqrt(1152) for weight and bias (fp32);
    n = 2 for the identity (delta) and the sigmoid (weight) head, 1 for softplus-centi (eta)."""
    rng = np.random.default_rng(1000 + 10 * seed + kind)
    k = 1.0 / np.sqrt(KTOT)
    n = N_OUT[kind]
    w = rng.uniform(-k, k, (n, C, KS, KS)).astype(np.float32)
    b = rng.uniform(-k, k, (n,)).astype(np.float32)
    return w, b


@functools.lru_cache(maxsize=None)
def hidden(B, H, W, seed):
    """x [B,128,H,W] float16, shared and never modified: half of a rectified normal, about half zeros, like a ReLU output."""
    rng = np.random.default_rng(7919 * seed + 1000 * H + 10 * W + B)
    x = half(np.maximum(rng.normal(0, 1, (B, C, H, W)), 0))
    x.setflags(write=False)
    return x


def shuffled_fp32(x, weight, bias, kind, seeds):
    """What a device may compute: the 1152 exact products and the bias summed in fp32 in a random order (one per seed),
    the activation in fp32, one rounding to half.  Returns one float64 array [B,H,W,n] of the halves' values per seed."""
    win = windows(x)
    B, _, H, W = win.shape
    w16 = half(weight).astype(np.float64).reshape(-1, KTOT)
    b16 = half(bias)
    outs = [np.empty((B, H, W, w16.shape[0])) for _ in seeds]
    for j in range(w16.shape[0]):
        exact = win * w16[j][None, :, None, None]
        prod = exact.astype(np.float32)    # exact: 11 x 11 bits
        assert np.array_equal(prod.astype(np.float64), exact)
        terms = np.concatenate([prod, np.broadcast_to(np.float32(b16[j]), (B, 1, H, W))], axis=1)
        for out, seed in zip(outs, seeds):
            acc = np.zeros((B, H, W), np.float32)
            for k in np.random.default_rng(seed).permutation(KTOT + 1):
                acc = acc + terms[:, k]
            with np.errstate(over="ignore"):
                if kind == SIGMOID:
                    acc = np.float32(1) / (np.float32(1) + np.exp(-acc))
                elif kind == SOFTPLUS_CENTI:
                    acc = np.float32(0.01) * np.where(acc > 20, acc, np.log1p(np.exp(np.minimum(acc, np.float32(20)))))
            assert acc.dtype == np.float32
            out[..., j] = half(acc).astype(np.float64)
    return outs
