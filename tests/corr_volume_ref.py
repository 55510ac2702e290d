"""Host restatement of `corr_volume_pyramid` (the all-pairs correlation pyramid CorrBlock.__init__ builds, reference
droid_slam/modules/corr.py:24-38, 63-71), written from the contract in include/droid_backends_hip.h.  Test code only:
the product never imports it.

  operands(fmaps, ii, jj, dtype)   a, b = T(f / 4) per edge, [E, C, hw] (zeros for an edge with an index out of range)
  level0_exact(a, b)               fp64 dot products of those operands, [E, hw, hw]
  abs_products(a, b)               sum_c |a_c| |b_c| in fp64, [E, hw, hw]
  level0_interval(a, b, dtype)     [T(x - beta), T(x + beta)], beta = (C + 2) 2^-24 sum|a||b|: every fp32 evaluation of
                                   the sum, in any order, rounds into it (first-order bound, rounding is monotone)
  pool(level, dtype)               level l+1 from the rounded level l: T(fp32(((v00 + v01) + v10) + v11) * 0.25f)
"""
import numpy as np


def operands(fmaps, ii, jj, dtype):
    """fmaps [nbuf, ncam, C, h, w] (or [nbuf, C, h, w]) -> a, b [E, C, h*w] of `dtype`, divided by 4 and ROUNDED to dtype."""
    fmaps = np.asarray(fmaps)
    if fmaps.ndim == 4:
        fmaps = fmaps[:, None]
    nbuf, ncam, C, h, w = fmaps.shape
    E = len(ii)
    a = np.zeros((E, C, h * w), dtype)
    b = np.zeros((E, C, h * w), dtype)
    for e, (i, j) in enumerate(zip(ii, jj)):
        if not (0 <= i < nbuf and 0 <= j < nbuf):
            continue
        cam = 1 if (ncam == 2 and i == j) else 0
        # numpy divides a half array in half precision (correctly rounded, subnormals kept), like torch
        a[e] = (fmaps[i, 0].astype(dtype) / dtype(4)).reshape(C, h * w)
        b[e] = (fmaps[j, cam].astype(dtype) / dtype(4)).reshape(C, h * w)
    return a, b


def level0_exact(a, b):
    return np.matmul(a.astype(np.float64).transpose(0, 2, 1), b.astype(np.float64))


def abs_products(a, b):
    return np.matmul(np.abs(a.astype(np.float64)).transpose(0, 2, 1), np.abs(b.astype(np.float64)))


def level0_interval(a, b, dtype):
    x = level0_exact(a, b)
    beta = (a.shape[1] + 2) * 2.0 ** -24 * abs_products(a, b)
    with np.errstate(over="ignore"):
        return (x - beta).astype(dtype), (x + beta).astype(dtype), x.astype(dtype)


def pool(level, dtype):
    """[..., H2, W2] of dtype -> [..., H2 // 2, W2 // 2]; odd sizes drop the last row / column."""
    v = np.asarray(level)
    assert v.dtype == dtype
    H2, W2 = v.shape[-2] // 2, v.shape[-1] // 2
    f = v[..., :2 * H2, :2 * W2].astype(np.float32)
    s = ((f[..., 0::2, 0::2] + f[..., 0::2, 1::2]) + f[..., 1::2, 0::2]) + f[..., 1::2, 1::2]
    return (s * np.float32(0.25)).astype(dtype)
