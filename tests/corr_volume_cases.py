"""Case table for corr_volume_pyramid_kernel (csrc/corr_volume.hip) and the classifier that says which of the kernel's
regimes a case reaches.  Host only, test code only: the product never imports it.

The classifier restates the kernel's host code (launch_corr_volume_pyramid) and its tile walk; the constants it uses
are compared with the ones parsed out of the sources in test_corr_volume_cases.py, so an edit of the kernel fails there
instead of silently un-covering a regime.  `write_counts` restates the kernel's WRITE MAPS (level-0 store and the
level 1/2/3 stores as functions of (tid, tile, p-tile)): address arithmetic only, no MFMA.
"""
from collections import namedtuple

import numpy as np

# ------------------------------------------------------------------------------------------ the kernel's constants
P = {np.float16: 32, np.float32: 16}     # query pixels per workgroup (CvCfg<T>::P)
KC = {np.float16: 32, np.float32: 16}    # channels per staged chunk (CvCfg<T>::KC)
TILE_W = 64                              # columns of a plane tile, at most
BAND = 8                                 # rows of a plane tile
XCD = 8                                  # the block order is changed iff E * nptiles % 8 == 0
THREADS = 256
C_STEP, C_MAX, HW_MAX, MIN_SIDE, W_STEP, HW_STEP, MAX_LEVELS = 32, 256, 1 << 24, 8, 8, 16, 4

Regime = namedtuple("Regime", "P nptiles ragged_ptile nbands last_band_rows odd_h nxc last_wc wc_changes reorder chunks")


def legal(E, H, W, C, levels, ncam=1):
    """The shape rules of corr_volume_pyramid_any (csrc/api.hip)."""
    return (E >= 0 and 1 <= ncam <= 2 and C > 0 and C % C_STEP == 0 and C <= C_MAX and H >= MIN_SIDE and W >= MIN_SIDE
            and W % W_STEP == 0 and (H * W) % HW_STEP == 0 and H * W <= HW_MAX and 1 <= levels <= MAX_LEVELS)


def classify(dtype, E, H, W, C, levels):
    hw = H * W
    p = P[dtype]
    nptiles = (hw + p - 1) // p
    nbands = (H + BAND - 1) // BAND
    nxc = (W + TILE_W - 1) // TILE_W
    last_wc = min(TILE_W, W - (nxc - 1) * TILE_W)
    return Regime(P=p, nptiles=nptiles, ragged_ptile=hw % p != 0, nbands=nbands, last_band_rows=H - BAND * (nbands - 1),
                  odd_h=H % 2 == 1, nxc=nxc, last_wc=last_wc, wc_changes=nxc > 1 and last_wc != TILE_W,
                  reorder=(E * nptiles) % XCD == 0, chunks=C // KC[dtype])


def describe(r):
    return (f"P={r.P} nptiles={r.nptiles}{'(ragged)' if r.ragged_ptile else ''} nbands={r.nbands}(last {r.last_band_rows})"
            f"{' oddH' if r.odd_h else ''} nxc={r.nxc}(last wc {r.last_wc}{', wc changes' if r.wc_changes else ''})"
            f" reorder={'on' if r.reorder else 'off'} chunks={r.chunks}")


# ------------------------------------------------------------------------------------------------- the case table
Case = namedtuple("Case", "name dtype H W C levels ncam nbuf ii jj seed")

SHAPES = [(8, 8), (9, 16), (10, 72), (12, 80), (8, 136), (11, 128), (16, 64)]
WIDE = [(10, 72), (12, 80), (8, 136), (11, 128)]          # nxc > 1
# 11x128 in fp32 has 88 p-tiles: E * 88 % 8 == 0 for every E, the reordering cannot be switched off there
ALWAYS_REORDERED = {(np.float32, 11, 128)}

# (H, W, C, levels, ncam, ii, jj); nbuf = 4.  ii == jj with ncam == 2 is a stereo edge (reads camera 1).
_ROWS = [
    (8, 8, 32, 4, 1, [0], [1]),                                                   # minimum: reordering off
    (8, 8, 256, 1, 1, [0, 1, 2, 3], [1, 2, 3, 0]),                                # reordering on at nxc == 1
    (9, 16, 96, 4, 2, [0, 2], [3, 2]),                                            # stereo
    (9, 16, 32, 2, 1, [1], [0]),                                                  # the levels > 2 guard not taken
    (10, 72, 32, 4, 1, [0, 1, 2, 3, 0, 1, 2, 3], [1, 2, 3, 0, 2, 3, 0, 1]),       # E = 8: reordering on (23 / 45 p-tiles)
    (10, 72, 96, 3, 2, [3, 1], [0, 1]),                                           # off; stereo; levels > 3 not taken
    (12, 80, 256, 4, 1, [2], [1]),                                                # off; the most chunks
    (12, 80, 32, 1, 1, [0, 1, 2, 3], [3, 0, 1, 2]),                               # on; level 0 only
    (8, 136, 96, 4, 1, [1], [3]),                                                 # off; three x-tiles
    (8, 136, 32, 4, 2, [0, 2, 2, 3], [2, 2, 1, 0]),                               # on; stereo
    (11, 128, 32, 4, 1, [3], [0]),                                                # half: off; fp32: on
    (11, 128, 96, 4, 1, [0, 1], [2, 3]),                                          # on for both types
    (16, 64, 32, 4, 1, [1], [2]),                                                 # control: what the older tests cover
]


def _cases():
    out = []
    for dt in (np.float16, np.float32):
        for n, (H, W, C, levels, ncam, ii, jj) in enumerate(_ROWS):
            name = f"{H}x{W}-{'f16' if dt is np.float16 else 'f32'}-C{C}-L{levels}-cam{ncam}-E{len(ii)}"
            out.append(Case(name, dt, H, W, C, levels, ncam, 4, ii, jj, 100 + n))
    return out


CASES = _cases()


def regime_of(case):
    return classify(case.dtype, len(case.ii), case.H, case.W, case.C, case.levels)


def make_fmaps(case):
    rng = np.random.default_rng(case.seed)
    return rng.normal(0, 1, (case.nbuf, case.ncam, case.C, case.H, case.W)).astype(case.dtype)


# ------------------------------------------------------------------------------------------------- special values
OVERFLOW_SHAPE = (10, 72, 32)   # H, W, C: nxc = 2, half only


def overflow_fmaps():
    """Half features [2, 1, 32, 10, 72] whose level 0 (edge 0 -> 1) rounds to +inf, to -inf and to finite values.

    Pixel p has the value s_p * m_p * (1 + noise) in every channel, m_p in {1, 400}, s_p = +-1: the sum over 32 channels
    of (m_p / 4)(m_q / 4) is 2 m_p m_q = 3.2e5 for two large pixels (beyond half's 65504, far from fp32's 3.4e38), 800
    or 2 otherwise."""
    H, W, C = OVERFLOW_SHAPE
    rng = np.random.default_rng(77)
    m = np.where(rng.random((2, 1, 1, H, W)) < 0.5, 400.0, 1.0)
    s = np.where(rng.random((2, 1, 1, H, W)) < 0.5, -1.0, 1.0)
    return (s * m * (1 + 0.05 * rng.normal(0, 1, (2, 1, C, H, W)))).astype(np.float16)


NAN_SHAPE = (10, 72, 64)        # H, W, C


def nan_fmaps(dtype):
    """Features [4, 1, 64, 10, 72] for the edges 0 -> 1 and 2 -> 3: one NaN in frame 0 at (channel 5, pixel p*), one in
    frame 1 at (channel 41, pixel q*).  p* lies in the last p-tile of either type (the ragged one of half), q* in the last
    row of the partial band and in the last (8-column) x-tile.  Returns fmaps, p*, q*."""
    H, W, C = NAN_SHAPE
    rng = np.random.default_rng(78)
    f = rng.normal(0, 1, (4, 1, C, H, W)).astype(dtype)
    pstar, qstar = H * W - 3, (H - 1) * W + (W - 2)
    f[0, 0, 5].reshape(-1)[pstar] = np.nan
    f[1, 0, 41].reshape(-1)[qstar] = np.nan
    return f, pstar, qstar


def bad_indices(nbuf):
    """Frame indices outside [0, nbuf); 2^32 and 2^32 + 1 are the frames 0 and 1 when cut to 32 bits."""
    return [-1, nbuf, 2 ** 32, 2 ** 32 + 1, 2 ** 63 - 1]


# -------------------------------------------------------------------------------------- the kernel's write maps
def write_counts(dtype, H, W, levels):
    """How often each element of each level of ONE slot is written by the workgroups of one edge, from the kernel's
    address arithmetic.  Returns (counts, outside): counts[l] is an int array of the level's size (H*W * (H>>l)*(W>>l)),
    outside the number of element writes that fall before or behind the slot at any level."""
    hw = H * W
    p = P[dtype]
    V = 16 // np.dtype(dtype).itemsize            # elements of a 16-byte piece
    PXB = TILE_W // V                             # lanes per plane row
    KPI = THREADS // (BAND * PXB)                 # query pixels per pass of the level-0 store
    nptiles, nbands, nxc = (hw + p - 1) // p, (H + BAND - 1) // BAND, (W + TILE_W - 1) // TILE_W
    sizes = [hw * (H >> l) * (W >> l) for l in range(levels)]
    counts = [np.zeros(n, np.int64) for n in sizes]
    outside = 0

    def put(l, off, run):
        """`run` consecutive elements from each offset in `off` (relative to the slot's first element of level l)."""
        nonlocal outside
        idx = (off[:, None] + np.arange(run)[None, :]).reshape(-1)
        ok = (idx >= 0) & (idx < sizes[l])
        outside += int(np.sum(~ok))
        np.add.at(counts[l], idx[ok], 1)

    tid = np.arange(THREADS)
    s_px, s_r, s_k = (tid % PXB) * V, (tid // PXB) & 7, tid // (BAND * PXB)
    for pt in range(nptiles):
        p0 = pt * p
        for t in range(nbands * nxc):
            band, x0 = t // nxc, (t % nxc) * TILE_W
            wc = min(TILE_W, W - x0)
            # level 0: thread (s_k, s_r, s_px), eight passes of KPI query pixels
            y = BAND * band + s_r
            live = (s_px < wc) & (y < H)
            for it in range(8):
                q = p0 + s_k + it * KPI
                sel = live & (q < hw)
                put(0, (q * hw + y * W + x0 + s_px)[sel], V)
            if levels < 2:
                continue
            # levels 1-3: thread (pp, bx) owns the 8x8 block at columns 8 bx of query pixel pp
            pp, bx = tid >> 3, tid & 7
            sel = (pp < p) & (8 * bx < wc) & (p0 + pp < hw)
            pix, xg = (p0 + pp)[sel], (x0 + 8 * bx)[sel]
            H1, W1, H2, W2, H3, W3 = H >> 1, W >> 1, H >> 2, W >> 2, H >> 3, W >> 3
            for r in range(4):
                if 4 * band + r < H1:
                    put(1, pix * (H1 * W1) + (xg >> 1) + (4 * band + r) * W1, 4)
            if levels > 2:
                for r in range(2):
                    if 2 * band + r < H2:
                        put(2, pix * (H2 * W2) + (xg >> 2) + (2 * band + r) * W2, 2)
                if levels > 3 and band < H3:
                    put(3, pix * (H3 * W3) + band * W3 + (xg >> 3), 1)
    return counts, outside
