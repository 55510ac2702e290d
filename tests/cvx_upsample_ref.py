"""Reference side of the convex-upsampling tests (droid_cvx_upsample, include/droid_backends_hip.h).

  ref(data, mask, dtype)   numpy restatement of the contract, written from its indexing formula with explicit padding and
                           slicing: dtype = np.float64 is THE reference, np.float32 the algorithm class of the kernel
  nb(data)                 per output pixel, the maximum of |P| over the 3x3 neighbourhood: the scale of the error bar
  stock(...)               the caller-shaped torch sequence `DepthVideo.upsample` runs (droid_slam/depth_video.py:134-138
                           -> droid_net.py:21-35): gather, softmax over 9, F.unfold, multiply, sum, pixel shuffle, indexed
                           write -- in the spirit of tests/callers.py: the call sequence, not the reference's module

The error bar ("Convex upsampling"): u = 2^-24; per weight expf <= 2u, the rounding of x = m - max <= u (it
enters as |x| u and w |x| <= 1/e), the 9-term denominator <= 8u + 3u, the division <= u; per output each product <= u
and the 9-term accumulation <= 8u of partial sums bounded by nb: about 24 u nb.  BAR = 32 u nb at every output pixel.
"""
import functools

import numpy as np

U = 2.0 ** -24
BAR = 32.0 * U                 # times nb, at every output pixel, none excluded
STOCK_F32_BAR = 64.0 * U       # device vs the stock chain with fp32 masks: two fp32 evaluations, each within 32 u nb
STOCK_F16_CPU_BAR = 2.0 * 2.0 ** -12   # the stock chain rounds its weights to half: measured 1.2 .. 1.5 x 2^-12 nb from fp64
STOCK_F16_DEV_BAR = 2.0 ** -10         # device vs the stock chain with half masks: 4x the stock chain's own distance

CASES = [(3, 5, 7), (2, 9, 8), (1, 1, 1), (2, 1, 9), (2, 6, 130), (2, 48, 64)]   # (n, H, W)
SIGMAS = [1.0, 4.0, 16.0]


def _taps(data, dtype):
    """P(y + ky - 1, x + kx - 1) for the 9 taps k = ky * 3 + kx: [9, n, H, W], zero outside the image."""
    n, H, W = data.shape
    pad = np.zeros((n, H + 2, W + 2), dtype)
    pad[:, 1:H + 1, 1:W + 1] = data
    return np.stack([pad[:, ky:ky + H, kx:kx + W] for ky in range(3) for kx in range(3)])


def ref(data, mask, dtype=np.float64):
    """data [n, H, W], mask [n, 576, H, W] (any float dtype, widened exactly) -> [n, 8H, 8W] of `dtype`.
    out[e, 8y+a, 8x+b] = sum_k w_k P_k(y, x), w = softmax_k(mask[e, (k*8+a)*8+b, y, x]): the maximum subtracted first,
    exp, the sum in ascending k, one division per weight, the products accumulated in ascending k."""
    n, H, W = data.shape
    m = np.asarray(mask).astype(dtype).reshape(n, 9, 8, 8, H, W)        # [e, k, a, b, y, x]
    P = _taps(np.asarray(data).astype(dtype), dtype)                    # [k, e, y, x]
    ex = np.exp(m - m.max(axis=1, keepdims=True))
    s = ex[:, 0].copy()
    for k in range(1, 9):
        s = s + ex[:, k]
    acc = (ex[:, 0] / s) * P[0][:, None, None]
    for k in range(1, 9):
        acc = acc + (ex[:, k] / s) * P[k][:, None, None]                # [e, a, b, y, x]
    assert acc.dtype == dtype
    return np.ascontiguousarray(acc.transpose(0, 3, 1, 4, 2)).reshape(n, 8 * H, 8 * W)


def nb(data):
    """[n, 8H, 8W] float64: max |P| over the 3x3 neighbourhood of the coarse pixel an output pixel belongs to."""
    m = np.abs(_taps(np.asarray(data, np.float64), np.float64)).max(axis=0)
    return np.repeat(np.repeat(m, 8, axis=1), 8, axis=2)


def err_nb(got, want64, scale):
    """max over ALL output pixels of |got - want| / nb (compare with BAR and the STOCK_* bars)."""
    got = np.asarray(got, np.float64)
    assert got.shape == want64.shape == scale.shape and np.isfinite(got).all()
    return float((np.abs(got - want64) / scale).max())


def stock(data, mask, ix=None, out=None):
    """The stock torch sequence.  data [buffer, h, w] f32, mask [n, 576, h, w] (half: the softmax returns half, so the
    weights are rounded to half, as in the reference with autocast off).  With ix / out: `disps_up[ix] = ...` of
    DepthVideo.upsample; without: the upsampled frames [n, 8h, 8w]."""
    import torch
    import torch.nn.functional as F
    d = data if ix is None else data[ix]                                  # the gather
    n, h, w = d.shape
    m = torch.softmax(mask.view(n, 1, 9, 8, 8, h, w), dim=2)
    up = F.unfold(d[:, None], [3, 3], padding=1).view(n, 1, 9, 1, 1, h, w)
    up = torch.sum(m * up, dim=2)                                         # materialises [n, 1, 9, 8, 8, h, w] in fp32
    up = up.permute(0, 4, 2, 5, 3, 1).reshape(n, 8 * h, 8 * w)            # pixel shuffle: a copy
    if out is None:
        return up
    out[ix] = up                                                          # index_put
    return out


@functools.lru_cache(maxsize=None)
def problem(case, sigma):
    """Seeded inputs and the shared references of one (case, sigma): data f32 U(0.001, 10), logits N(0, sigma^2) generated
    as half (mask32 is the same values widened, so one fp64 reference serves both).  The arrays are read-only."""
    n, H, W = CASES[case]
    rng = np.random.default_rng(1000 * case + int(sigma))
    data = rng.uniform(0.001, 10.0, (n, H, W)).astype(np.float32)
    mask16 = rng.normal(0.0, sigma, (n, 576, H, W)).astype(np.float16)
    p = dict(data=data, mask16=mask16, mask32=mask16.astype(np.float32), ref64=ref(data, mask16, np.float64), nb=nb(data))
    for v in p.values():
        v.setflags(write=False)
    return p


@functools.lru_cache(maxsize=None)
def onehot(case):
    """Masks that select ONE tap per output pixel: its logit is +60000, the other eight -60000 (both exact in half; the
    difference of 120000 underflows exp to 0 and the selected weight is exactly 1).  The selected tap cycles over all 9
    with (a, b), the pixel and the entry.  Expected: exactly the selected neighbour, +0.0 where it is padding -- this
    pins the (k, a, b) channel order and the borders without a tolerance.  Returns data, mask16, expected [n, 8H, 8W]."""
    n, H, W = CASES[case]
    rng = np.random.default_rng(77 + case)
    data = rng.uniform(0.001, 10.0, (n, H, W)).astype(np.float32)
    e, a, b, y, x = np.meshgrid(np.arange(n), np.arange(8), np.arange(8), np.arange(H), np.arange(W), indexing="ij")
    sel = (e + a * 8 + b + 5 * (y * W + x)) % 9                           # [e, a, b, y, x]
    m = np.full((n, 9, 8, 8, H, W), -60000.0, np.float16)
    np.put_along_axis(m, sel[:, None], np.float16(60000.0), axis=1)
    yy, xx = y + sel // 3 - 1, x + sel % 3 - 1
    inside = (yy >= 0) & (yy < H) & (xx >= 0) & (xx < W)
    want = np.where(inside, data[e, yy.clip(0, H - 1), xx.clip(0, W - 1)], np.float32(0.0)).astype(np.float32)
    want = np.ascontiguousarray(want.transpose(0, 3, 1, 4, 2)).reshape(n, 8 * H, 8 * W)
    mask16 = m.reshape(n, 576, H, W)
    for v in (data, mask16, want):
        v.setflags(write=False)
    return data, mask16, want


def same_bits(a, b):
    a, b = np.ascontiguousarray(a, np.float32), np.ascontiguousarray(b, np.float32)
    return a.shape == b.shape and np.array_equal(a.view(np.uint32), b.view(np.uint32))
