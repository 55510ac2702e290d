"""Cases of the correlation parity tests (tests/test_gpu_corr_paths.py) and a host restatement of the dispatch of
csrc/corr.hip.  Plain helpers, no fixtures: tests/test_corr_cases.py proves on the CPU that the tables below reach every
path the dispatch can take and every per-tile branch of the tiled kernels; the GPU tests then hold the same cases to
oracle/corr.py.

The restatement is by hand on purpose (like stage_graphs.predicted_classes): a kernel whose threshold is retuned must
fail tests/test_corr_cases.py, which reads the constants from the source, instead of silently losing its test.
"""
import numpy as np

# ---- constants of csrc/corr.hip (compared with the source by test_constants_match_the_source) -----------------------
CS_MAXPLANE = 192
ALT_TQ, ALT_MAXPOS, ALT_CH = 8, 448, 32
AM_TX, AM_TY, AM_MAXBLK, AM_MAXPOS = 16, 4, 15, 640
AM_XBLK = {3: 12, 4: 15}                 # AmCfg<R>::XBLK
AM_CH = {"f32": 16}                      # AM_CH: the workgroup matrix-core path takes fp32 maps only
AM_MAXSTAGE = {"f32": 8}                 # AM_MAXSTAGE
AW_MAXBLK = {3: 15, 4: 20}               # AwCfg<R>::MAXBLK
ABT, AB_CH, AB_MAXPOS = 8, 16, 448
G1MAX = 16                               # altcorr_backward_kernel keeps 16 * G1MAX channels in registers
SETUP_LIM, SETUP_EMPTY = 1.0e6, -2000000  # bilin_setup: clamp of far coordinates, origin of a non-finite query

DTYPES = {"f16": np.float16, "f32": np.float32, "f64": np.float64}
SIZE = {"f16": 2, "f32": 4, "f64": 8}


# ---- dispatch ------------------------------------------------------------------------------------------------------
def volume_path(dtype, r, HW, H2, W2, base_align, slotted, entry="index"):
    """Kernel that serves one level of a volume lookup: launch_corr_small, launch_corr_coop, corr_index_forward_t /
    corr_pyramid_forward_t.  base_align: the volume's base address modulo 16.  entry "pyramid" (with or without
    slots) refuses every radius but 3 and 4 (corr_pyramid_shape_ok): None."""
    sz = SIZE[dtype]
    if entry != "index" and r not in (3, 4):
        return None
    assert entry != "index" or not slotted
    if r in (3, 4):
        pb = H2 * W2 * sz
        if pb <= CS_MAXPLANE and pb % 16 == 0 and base_align % 16 == 0:
            return "small"
        if r == 3 and sz <= 4 and W2 * sz <= 64 and HW % 64 == 0:
            return "coop"
        return "row"
    return "generic"


def alt_forward_path(dtype, r, C, H1, W1, H2, W2):
    """launch_altcorr_forward, in its order."""
    lim = 1 << 30
    if dtype == "f32" and C % AM_CH["f32"] == 0 and C <= AM_CH["f32"] * AM_MAXSTAGE["f32"] and r in (3, 4) and H2 * W2 * C < lim:
        return "mfma_f32"
    if dtype == "f16" and C % 32 == 0 and C <= 128 and r in (3, 4) and H2 * W2 * C < lim and H1 * W1 * C < lim:
        return "wave_f16"
    if dtype == "f32" and C % ALT_CH == 0 and r in (3, 4):
        return "tiled"
    return "generic"


def alt_backward_path(r, C):
    """launch_altcorr_backward and the g1_regs switch of altcorr_backward_kernel."""
    if C % AB_CH == 0 and r in (3, 4):
        return "tiled"
    return "per_tap_regs" if C <= 16 * G1MAX else "per_tap_atomics"


# ---- bilin_setup and the per-tile branches -------------------------------------------------------------------------
def bilin_origin(x, y, r):
    """Top-left integer tap (x1, y1) of every query, as bilin_setup forms it: floor, clamp to +-1e6, minus r; a NaN or
    infinite coordinate in either component sends both to -2000000."""
    x = np.asarray(x, np.float32)
    y = np.asarray(y, np.float32)
    fin = np.isfinite(x) & np.isfinite(y)
    with np.errstate(invalid="ignore"):
        fx = np.clip(np.floor(np.where(fin, x, 0)), -SETUP_LIM, SETUP_LIM).astype(np.int64) - r
        fy = np.clip(np.floor(np.where(fin, y, 0)), -SETUP_LIM, SETUP_LIM).astype(np.int64) - r
    return np.where(fin, fx, SETUP_EMPTY), np.where(fin, fy, SETUP_EMPTY)


def _tiles(a, th, tw, fill):
    """[..., H, W] -> [..., tiles_y, tiles_x, th * tw], ragged edges padded with `fill` (masked queries)."""
    H, W = a.shape[-2:]
    ty, tx = -(-H // th), -(-W // tw)
    p = np.full(a.shape[:-2] + (ty * th, tx * tw), fill, a.dtype)
    p[..., :H, :W] = a
    p = p.reshape(a.shape[:-2] + (ty, th, tx, tw))
    return np.moveaxis(p, -3, -2).reshape(a.shape[:-2] + (ty, tx, th * tw))


def _boxes(coords, r, H2, W2, th, tw):
    """Clipped bounding box of the windows of every th x tw query tile: (width, height, x0, y0, any hit), each
    [B, N, tiles_y, tiles_x].  coords [B, N, H1, W1, 2].  Queries whose window misses the map do not stretch the box."""
    nt = 2 * r + 2
    x1, y1 = bilin_origin(coords[..., 0], coords[..., 1], r)
    hit = (x1 + nt > 0) & (x1 < W2) & (y1 + nt > 0) & (y1 < H2)
    big = 1 << 40
    tx1, ty1, thit = _tiles(x1, th, tw, 0), _tiles(y1, th, tw, 0), _tiles(hit, th, tw, False)
    x0 = np.maximum(np.where(thit, tx1, big).min(-1), 0)
    y0 = np.maximum(np.where(thit, ty1, big).min(-1), 0)
    xe = np.minimum(np.where(thit, tx1 + nt, -big).max(-1), W2)
    ye = np.minimum(np.where(thit, ty1 + nt, -big).max(-1), H2)
    return np.maximum(xe - x0, 0), np.maximum(ye - y0, 0), x0, y0, thit.any(-1)


def backward_tile_classes(coords, r, H2, W2):
    """altcorr_backward_tiled per 8x8 tile: "empty" (npos == 0: early return), "hit_lists", "incoherent"
    (npos > AB_MAXPOS: per-tap atomics)."""
    bw, bh, _, _, _ = _boxes(coords, r, H2, W2, ABT, ABT)
    npos = bw * bh
    return np.where(npos == 0, "empty", np.where(npos > AB_MAXPOS, "incoherent", "hit_lists"))


def tiled_forward_tile_classes(coords, r, H2, W2):
    """altcorr_forward_tiled per 8x8 tile: "staged" or "per_query" (npos > ALT_MAXPOS)."""
    bw, bh, _, _, _ = _boxes(coords, r, H2, W2, ALT_TQ, ALT_TQ)
    return np.where(bw * bh > ALT_MAXPOS, "per_query", "staged")


def mfma_tile_classes(coords, r, H2, W2):
    """altcorr_mfma_body per 16x4 tile.  Each of its four waves boxes a 4x4 sub-tile; the workgroup stages the union.
    "per_query" (!fits: a wave box over 16 AM_MAXBLK positions or a union over AM_MAXPOS), "two_rounds" (a wave box
    over 16 XBLK positions where XBLK < AM_MAXBLK, that is radius 3), else "one_round"."""
    sw, sh, sx, sy, _ = _boxes(coords, r, H2, W2, 4, 4)          # [B, N, ty4, tx4]
    live = (sw > 0) & (sh > 0)
    nposw = sw * sh
    big = 1 << 40
    grp = lambda a, fill: _tiles(a, 1, 4, fill)                    # four sub-tiles in x make one workgroup tile
    glive = grp(live, False)
    bx0 = np.where(glive, grp(sx, 0), big).min(-1)
    by0 = np.where(glive, grp(sy, 0), big).min(-1)
    bx1 = np.where(glive, grp(sx + sw, 0), -big).max(-1)
    by1 = np.where(glive, grp(sy + sh, 0), -big).max(-1)
    npos = np.maximum(bx1 - bx0, 0) * np.maximum(by1 - by0, 0)
    gn = np.where(glive, grp(nposw, 0), 0)
    fits = (gn <= 16 * AM_MAXBLK).all(-1) & (npos <= AM_MAXPOS)
    two = (gn > 16 * AM_XBLK[r]).any(-1) & (AM_XBLK[r] < AM_MAXBLK)
    return np.where(~fits, "per_query", np.where(two, "two_rounds", "one_round"))


def wave_tile_classes(coords, r, H2, W2):
    """altcorr_wave_f16 per 4x4 sub-tile (one wave): "per_query" when the box exceeds 16 AwCfg<R>::MAXBLK positions,
    else "box_gemm"."""
    sw, sh, _, _, _ = _boxes(coords, r, H2, W2, 4, 4)
    return np.where(sw * sh > 16 * AW_MAXBLK[r], "per_query", "box_gemm")


def nonfinite_tiles(coords, th, tw):
    """[B, N, tiles_y, tiles_x]: does the th x tw query tile hold a NaN or infinite coordinate?"""
    return _tiles(~np.isfinite(coords).all(-1), th, tw, False).any(-1)


def class_shares(classes):
    names, counts = np.unique(classes, return_counts=True)
    return {str(n): c / classes.size for n, c in zip(names, counts)}


# ---- coordinates ---------------------------------------------------------------------------------------------------
NONFINITE = ((np.nan, 2.25), (1.5, np.nan), (np.inf, 2.0), (-np.inf, 2.0), (3.0, np.inf), (np.nan, np.inf))
KINDS = ("integer", "half", "near_one", "near_zero", "random", "border", "empty", "nonfinite")


def edge_coords(rng, n, r, H2, W2):
    """n query coordinates (x [n], y [n], kind [n]) for a plane of H2 x W2 and radius r, the kinds dealt round-robin:
    integer (dx = 0), k + .5, k + 0.99999 and k + 1e-5 (a half weight that rounds to 1 or to 0), uniform over the
    plane and r + 2 beyond it, windows hanging over each of the four borders by 1 .. 2r+1 taps, wholly empty windows
    (just outside, and 1e9 / 1e30 away), and NaN in x only, in y only, +inf, -inf."""
    nt = 2 * r + 2
    x = rng.integers(0, W2, n).astype(np.float64)
    y = rng.integers(0, H2, n).astype(np.float64)
    kind = np.arange(n) % len(KINDS)
    order = np.arange(n)
    for k, name in enumerate(KINDS):
        m = order[kind == k]
        if name == "half":
            x[m] += 0.5
            y[m] += np.where(np.arange(len(m)) % 2 == 0, 0.5, 0.0)
        elif name == "near_one":
            x[m] += 0.99999
            y[m] += np.where(np.arange(len(m)) % 2 == 0, 0.99999, 0.25)
        elif name == "near_zero":
            x[m] += 1e-5
            y[m] += np.where(np.arange(len(m)) % 2 == 0, 1e-5, 0.75)
        elif name == "random":
            x[m] = rng.uniform(-r - 2, W2 + r + 2, len(m))
            y[m] = rng.uniform(-r - 2, H2 + r + 2, len(m))
        elif name == "border":
            for t, q in enumerate(m):
                over, side = 1 + (t // 4) % (nt - 1), t % 4       # taps outside the plane, which border
                f = rng.uniform(0, 1)
                if side == 0:
                    x[q] = r - over + f                             # x1 = -over
                elif side == 1:
                    x[q] = W2 + over - nt + r + f                   # x1 + nt = W2 + over
                elif side == 2:
                    y[q] = r - over + f
                else:
                    y[q] = H2 + over - nt + r + f
        elif name == "empty":
            for t, q in enumerate(m):
                size = W2 if t % 2 == 0 else H2                     # even t: x leaves the plane, odd t: y
                far = (-r - 2.5, size + r + 0.5, -1e9, 1e9, -1e30, 1e30)[(t // 2) % 6]
                if t % 2 == 0:
                    x[q] = far
                else:
                    y[q] = far
        elif name == "nonfinite":
            for t, q in enumerate(m):
                x[q], y[q] = NONFINITE[t % len(NONFINITE)]
    p = rng.permutation(n)
    return x[p].astype(np.float32), y[p].astype(np.float32), kind[p]


# ---- volume lookups ------------------------------------------------------------------------------------------------
QMAPS = ((8, 8), (7, 9), (9, 8), (16, 20))
PLANES = {"f16": ((8, 8), (3, 4), (24, 32), (12, 17)), "f32": ((4, 8), (12, 16), (12, 17)), "f64": ((4, 6), (12, 17))}


class VolumeCase:
    """One call of corr_index_forward ("index"), corr_pyramid_forward ("pyramid") or corr_pyramid_forward with slots
    ("slots").  levels: the planes (H2, W2) per level; offset: the volume is a contiguous view one element into its
    storage (base 2 mod 4 for halves, off 16 for every type)."""

    def __init__(self, dtype, r, qmap, levels, entry="index", values="normal", offset=False, seed=0):
        self.dtype, self.r, self.qmap, self.levels = dtype, r, tuple(qmap), tuple(levels)
        self.entry, self.values, self.offset, self.seed = entry, values, offset, seed
        self.B = 2 if entry == "index" else 4
        self.cap = 5
        self.slots = np.array([3, 0, 3, 7], np.int64) if entry == "slots" else None   # permuted, repeated, out of range
        lv = "+".join(f"{h}x{w}" for h, w in self.levels)
        self.id = f"{entry}-{dtype}-r{r}-q{qmap[0]}x{qmap[1]}-p{lv}-{values}" + ("-offset" if offset else "")

    @property
    def slotted(self):
        return self.entry == "slots"

    def paths(self):
        hw = self.qmap[0] * self.qmap[1]
        al = SIZE[self.dtype] if self.offset else 0
        return [volume_path(self.dtype, self.r, hw, h, w, al, self.slotted, self.entry) for h, w in self.levels]

    def tuples(self):
        return {(p, self.dtype, self.r, self.slotted, self.entry) for p in self.paths()}

    def build(self):
        """(volumes per level [nb, H1, W1, H2, W2], coords [B, 2, H1, W1] at level-0 scale, kinds [B, H1, W1]);
        nb = cap for the slotted entry, else B."""
        rng = np.random.default_rng(1000 + self.seed)
        dt = DTYPES[self.dtype]
        H1, W1 = self.qmap
        nb = self.cap if self.slotted else self.B
        vols = []
        for h, w in self.levels:
            shape = (nb, H1, W1, h, w)
            if self.values == "normal":
                v = rng.normal(0, 1, shape)
            else:   # magnitudes 2^U(-24, 12), random signs: subnormal halves, products below the half range, and
                    # partial sums whose exponents differ by more than 13 (at most 4 * 2^12 per output: finite)
                v = np.exp2(rng.uniform(-24, 12, shape)) * rng.choice([-1.0, 1.0], shape)
            vols.append(v.astype(dt))
        # coordinates are drawn for the plane of level 0 and handed over at level-0 scale; level l sees them * 2^-l
        h0, w0 = self.levels[0]
        n = self.B * H1 * W1
        x, y, kind = edge_coords(rng, n, self.r, h0, w0)
        coords = np.stack([x.reshape(self.B, H1, W1), y.reshape(self.B, H1, W1)], 1)
        kind = kind.reshape(self.B, H1, W1)
        if self.offset:
            # windows on the first rows of the first plane and the last rows of the last plane of the tensor: the row
            # loads there would leave the tensor (and, for a base at 2 mod 4, start before it)
            coords[0, :, 0, 0] = (self.r + 0.25, self.r + 0.5)                       # x1 = 0, y1 = 0
            coords[-1, :, -1, -1] = (w0 - self.r - 2 + 0.75, h0 - self.r - 2 + 0.5)  # x1 + nt = W2, y1 + nt = H2
            kind[0, 0, 0] = kind[-1, -1, -1] = KINDS.index("random")
        return vols, np.ascontiguousarray(coords, np.float32), kind


def _volume_cases():
    out, k = [], 0
    for dtype in ("f16", "f32", "f64"):
        for r in (1, 2, 3, 4, 5):
            for plane in PLANES[dtype]:
                for qmap in (QMAPS if r in (3, 4) else ((7, 9), (16, 20))):
                    out.append(VolumeCase(dtype, r, qmap, [plane], values=("normal", "wide")[k % 2], seed=k))
                    k += 1
    # a storage offset of one element: `small` refuses the base, coop and the row kernel meet both ends of the tensor
    for dtype, plane, qmap in (("f16", (8, 8), (8, 8)), ("f16", (24, 32), (16, 20)), ("f32", (4, 8), (8, 8)),
                               ("f32", (12, 17), (7, 9)), ("f64", (4, 6), (7, 9))):
        for r in (3, 4):
            out.append(VolumeCase(dtype, r, qmap, [plane], values=("wide", "normal")[k % 2], offset=True, seed=k))
            k += 1
    for dtype in ("f16", "f32", "f64"):
        out.append(VolumeCase(dtype, 2, (7, 9), [PLANES[dtype][0]], offset=True, seed=k))
        k += 1
    for entry in ("pyramid", "slots"):
        for dtype in ("f16", "f32", "f64"):
            for r in (3, 4):
                for qmap, nl in (((8, 8), 4), ((16, 20), 3), ((9, 8), 2), ((12, 17), 2)):
                    levels = [(qmap[0] >> l, qmap[1] >> l) for l in range(nl)]
                    out.append(VolumeCase(dtype, r, qmap, levels, entry=entry, values=("normal", "wide")[k % 2], seed=k))
                    k += 1
    return out


VOLUME_CASES = _volume_cases()


def reachable_volume_tuples():
    """Every (path, dtype, radius, slotted, entry) the dispatch can pick over a grid of shapes that is wider than the
    table: all query maps and planes below, aligned and unaligned bases."""
    qmaps = QMAPS + ((12, 16), (24, 32), (48, 64), (5, 5), (1, 64))
    planes = sorted({p for ps in PLANES.values() for p in ps} | {(1, 1), (2, 2), (6, 8), (48, 64), (1, 24), (16, 20)})
    found = set()
    for dtype in DTYPES:
        for r in (1, 2, 3, 4, 5):
            for qh, qw in qmaps:
                for al in (0, SIZE[dtype]):
                    for h, w in planes:
                        found.add((volume_path(dtype, r, qh * qw, h, w, al, False), dtype, r, False, "index"))
                    for entry in ("pyramid", "slots"):
                        for l in range(4):
                            if (qh >> l) < 1 or (qw >> l) < 1:
                                break
                            p = volume_path(dtype, r, qh * qw, qh >> l, qw >> l, al, entry == "slots", entry)
                            if p is not None:
                                found.add((p, dtype, r, entry == "slots", entry))
    return found


# ---- corr_index_backward -------------------------------------------------------------------------------------------
class IndexBackwardCase:
    def __init__(self, dtype, r, qmap, plane, seed):
        self.dtype, self.r, self.qmap, self.plane, self.seed = dtype, r, qmap, plane, seed
        self.id = f"{dtype}-r{r}-q{qmap[0]}x{qmap[1]}-p{plane[0]}x{plane[1]}"

    def build(self):
        rng = np.random.default_rng(2000 + self.seed)
        (H1, W1), (H2, W2), B, rd = self.qmap, self.plane, 2, 2 * self.r + 1
        x, y, kind = edge_coords(rng, B * H1 * W1, self.r, H2, W2)
        coords = np.ascontiguousarray(np.stack([x.reshape(B, H1, W1), y.reshape(B, H1, W1)], 1), np.float32)
        cg = rng.normal(0, 1, (B, rd, rd, H1, W1)).astype(DTYPES[self.dtype])
        return (B, H1, W1, H2, W2), coords, cg, kind.reshape(B, H1, W1)


INDEX_BACKWARD_CASES = [IndexBackwardCase(d, r, q, p, i) for i, (d, r, q, p) in enumerate(
    (d, r, q, p) for d in ("f16", "f32", "f64") for r in (1, 3, 4) for q in ((7, 9), (16, 20)) for p in ((4, 6), (12, 17)))]


# ---- alt-corr ------------------------------------------------------------------------------------------------------
class AltCase:
    """Feature maps fmap1 [B, H1, W1, C], fmap2 [B, H2, W2, C] and N coordinate sets: the identity grid scaled to
    fmap2 plus a per-tile jitter (`jitter` px, or `jitter_mixed` = (small, large) alternating by 8x8 tile), with
    border, empty and non-finite queries spliced in at fixed places."""

    def __init__(self, name, dtype, r, C, qmap, fmap2, jitter, N=1, B=2, mixed=None, seed=0, empty_tile=False):
        self.empty_tile = empty_tile
        self.id, self.dtype, self.r, self.C, self.qmap, self.fmap2 = name, dtype, r, C, qmap, fmap2
        self.jitter, self.N, self.B, self.mixed, self.seed = jitter, N, B, mixed, seed

    def forward_path(self):
        return alt_forward_path(self.dtype, self.r, self.C, *self.qmap, *self.fmap2)

    def backward_path(self):
        return alt_backward_path(self.r, self.C)

    def build(self):
        """(fmap1, fmap2, coords [B, N, H1, W1, 2]); the maps are halves / 4 widened to the case's type, so that the
        same values serve every element type."""
        rng = np.random.default_rng(3000 + self.seed)
        (H1, W1), (H2, W2), B, N, C = self.qmap, self.fmap2, self.B, self.N, self.C
        dt = DTYPES[self.dtype]
        f1 = (rng.normal(0, 1, (B, H1, W1, C)).astype(np.float16) / np.float16(4)).astype(dt)
        f2 = (rng.normal(0, 1, (B, H2, W2, C)).astype(np.float16) / np.float16(4)).astype(dt)
        yy, xx = np.meshgrid(np.arange(H1, dtype=np.float64), np.arange(W1, dtype=np.float64), indexing="ij")
        gx = (xx + 0.5) * W2 / W1 - 0.5
        gy = (yy + 0.5) * H2 / H1 - 0.5
        j = np.full((H1, W1), float(self.jitter or 0))
        if self.mixed is not None:
            tile = (np.arange(H1)[:, None] // 8 + np.arange(W1)[None, :] // 8) % 2
            j = np.where(tile == 0, float(self.mixed[0]), float(self.mixed[1]))
        cx = gx[None, None] + rng.uniform(-1, 1, (B, N, H1, W1)) * j
        cy = gy[None, None] + rng.uniform(-1, 1, (B, N, H1, W1)) * j
        coords = np.stack([cx, cy], -1).astype(np.float32)
        # spliced queries.  Every entry of NONFINITE (NaN in x only, in y only, +inf, -inf, inf in y, NaN with inf) goes
        # into every (b, n) at places spread evenly over the map, so that they fall into different tiles; then border,
        # empty and near-integer queries at random places, a tenth of the map
        x, y, kind = edge_coords(rng, 3 * len(KINDS), self.r, H2, W2)
        keep = np.isin(kind, [KINDS.index(k) for k in ("border", "empty", "near_one")])
        sx, sy = x[keep], y[keep]
        flat = coords.reshape(B, N, H1 * W1, 2)
        HW, nn = H1 * W1, len(NONFINITE)
        m = min(len(sx), max(HW // 10, 3))
        for b in range(B):
            for n in range(N):
                at = rng.choice(HW, m, replace=False)
                o = rng.permutation(len(sx))[:m]
                flat[b, n, at, 0], flat[b, n, at, 1] = sx[o], sy[o]
        if self.empty_tile:   # the first 8x8 tile of (0, 0): far away, NaN and inf only -- no window touches the map
            coords[0, 0, :8, :8] = np.float32(-1e9)
            coords[0, 0, 0:8:2, 0:8:3, 0] = np.nan
            coords[0, 0, 1:8:2, 1:8:3, 1] = np.inf
        for b in range(B):
            for n in range(N):
                nf_at = ((2 * np.arange(nn) + 1) * HW // (2 * nn) + 3 * (b + n)) % HW
                flat[b, n, nf_at] = np.array(NONFINITE, np.float32)
        return f1, f2, coords


ALT_BACKWARD_CASES = [
    AltCase("incoherent-r3-C16", "f32", 3, 16, (8, 8), (24, 24), 12.0, N=2, seed=1),
    AltCase("incoherent-r4-C32", "f32", 4, 32, (9, 11), (24, 24), 12.0, N=2, seed=2),
    AltCase("mixed-r3-C16", "f32", 3, 16, (16, 24), (24, 24), None, N=2, mixed=(1.0, 12.0), seed=3, empty_tile=True),
    AltCase("tiled-r3-C272", "f32", 3, 272, (5, 6), (6, 7), 1.5, seed=4),
    AltCase("per-tap-regs-r3-C40", "f32", 3, 40, (5, 6), (6, 7), 1.5, N=2, seed=5),
    AltCase("per-tap-regs-r2-C32", "f32", 2, 32, (5, 6), (6, 7), 1.5, N=2, seed=6),
    AltCase("per-tap-atomics-r3-C264", "f32", 3, 264, (5, 6), (6, 7), 1.5, N=2, seed=7),
]
# the class meant to dominate each tiled backward case (at least a quarter of its tiles; test_corr_cases.py)
ALT_BACKWARD_DOMINANT = {"incoherent-r3-C16": ("incoherent",), "incoherent-r4-C32": ("incoherent",),
                         "mixed-r3-C16": ("incoherent", "hit_lists")}

ALT_FORWARD_CASES = [
    AltCase("generic-f64-r2-C24", "f64", 2, 24, (7, 9), (9, 10), 2.0, N=2, seed=11),
    AltCase("generic-f64-r3-C40", "f64", 3, 40, (7, 9), (9, 10), 2.0, seed=12),
    AltCase("generic-f64-r2-C40", "f64", 2, 40, (5, 6), (6, 7), 2.0, seed=13),
    AltCase("generic-f64-r3-C24", "f64", 3, 24, (5, 6), (6, 7), 2.0, seed=14),
    AltCase("generic-f16-r3-C40", "f16", 3, 40, (7, 9), (9, 10), 2.0, seed=15),
    AltCase("generic-f32-r5-C32", "f32", 5, 32, (5, 6), (6, 7), 2.0, seed=16),
    # non-finite, border and empty queries on each of the fast paths, and the per-tile branches no earlier test reaches
    AltCase("mfma-f32-r3-C32", "f32", 3, 32, (8, 16), (8, 16), 1.0, seed=17),
    AltCase("mfma-f32-r4-C16", "f32", 4, 16, (7, 18), (8, 16), 1.0, seed=18),
    AltCase("mfma-f32-r3-C16-two-rounds", "f32", 3, 16, (16, 32), (16, 32), 2.4, B=1, seed=19),
    AltCase("mfma-f32-r3-C16-per-query", "f32", 3, 16, (8, 16), (20, 24), 12.0, seed=20),
    AltCase("mfma-f32-r4-C16-per-query", "f32", 4, 16, (6, 18), (20, 24), 12.0, seed=21),
    AltCase("wave-f16-r3-C32", "f16", 3, 32, (7, 9), (9, 10), 1.0, seed=22),
    AltCase("wave-f16-r4-C64", "f16", 4, 64, (7, 9), (9, 10), 1.0, seed=23),
    AltCase("wave-f16-r3-C32-per-query", "f16", 3, 32, (6, 7), (20, 24), 12.0, seed=24),
    AltCase("wave-f16-r4-C32-per-query", "f16", 4, 32, (6, 7), (20, 24), 12.0, seed=25),
    AltCase("tiled-f32-r3-C160", "f32", 3, 160, (9, 10), (9, 10), 1.0, seed=26),
    AltCase("tiled-f32-r4-C160-per-query", "f32", 4, 160, (8, 8), (24, 24), 12.0, seed=27),
]
ALT_FORWARD_DOMINANT = {"mfma-f32-r3-C16-two-rounds": ("mfma", "two_rounds"), "mfma-f32-r3-C16-per-query": ("mfma", "per_query"),
                        "mfma-f32-r4-C16-per-query": ("mfma", "per_query"), "wave-f16-r3-C32-per-query": ("wave", "per_query"),
                        "wave-f16-r4-C32-per-query": ("wave", "per_query"), "tiled-f32-r4-C160-per-query": ("tiled", "per_query")}


FORWARD_TILE = {"mfma_f32": (AM_TY, AM_TX), "wave_f16": (4, 4), "tiled": (ALT_TQ, ALT_TQ)}   # query tile (rows, columns)


def forward_tile_classes(case, coords):
    """Per-tile classes of the kernel that serves an alt-corr forward case, or None for the generic kernel."""
    path = case.forward_path()
    fn = {"mfma_f32": mfma_tile_classes, "wave_f16": wave_tile_classes, "tiled": tiled_forward_tile_classes}.get(path)
    return None if fn is None else fn(coords, case.r, *case.fmap2)


# ---- the inputs of three older tests, rebuilt: which per-tile branches do their jitters reach? ------------------------
def legacy_mfma_coords(jitter, C, H, W):
    """Coordinates of tests/test_gpu_corr.py::test_altcorr_diverging_windows_and_channel_counts (same generator calls)."""
    rng = np.random.default_rng(int(jitter * 10) + C)
    rng.normal(0, 1, (2, H, W, C)), rng.normal(0, 1, (2, H, W, C))
    yy, xx = np.meshgrid(np.arange(H, dtype=np.float32), np.arange(W, dtype=np.float32), indexing="ij")
    cx = xx[None] + rng.uniform(-jitter, jitter, (2, H, W))
    cy = yy[None] + rng.uniform(-jitter, jitter, (2, H, W))
    coords = np.stack([cx, cy], -1)[:, None].astype(np.float32)
    coords[0, 0, 0, 0] = [-1e9, 3.0]
    coords[1, 0, H - 1, W - 1] = [1e9, -1e9]
    return coords


def legacy_wave_coords(C, r, jitter):
    """Coordinates of tests/test_gpu_baseline_shapes.py::test_altcorr_half_wave_kernel_channel_counts_edges_and_
    diverging_windows (same generator calls): [E, 1, 10, 13, 2]."""
    rng = np.random.default_rng(7 * C + r)
    F, H, W = 3, 10, 13
    rng.normal(0, 1, (F, H, W, C))
    yy, xx = np.meshgrid(np.arange(H, dtype=np.float32), np.arange(W, dtype=np.float32), indexing="ij")
    coords = np.stack([xx[None] + rng.uniform(-jitter, jitter, (4, H, W)), yy[None] + rng.uniform(-jitter, jitter, (4, H, W))],
                      -1).astype(np.float32)
    return coords[:, None]


# ---- componentwise bars --------------------------------------------------------------------------------------------
U32, U64, U16 = 2.0 ** -24, 2.0 ** -53, 2.0 ** -11
COMBINE_OPS = 8   # four products and three adds that form a bilinear combine, and the product with the feature / the
                  # rounding of the tap sum it combines


def forward_bound(case, abs_sum, ref):
    """|got - ref| allowed per element of an alt-corr forward output.  A dot product of C terms summed in any order
    in a type with unit roundoff u is within C u sum|terms| of the truth (first order; the tests' C u < 1e-4), and the
    combine adds COMBINE_OPS more roundings of quantities bounded by the same sum: (C + 8) u sum|terms|.
    abs_sum = the oracle on |fmap1|, |fmap2| (the weights are non-negative).  f64: u = 2^-53.  f32 and the f16 wave
    kernel: u = 2^-24 (fp32 accumulation and combine); the wave kernel stores a half: half an ulp of the result more.
    The generic kernel on f16 accumulates the dot product in fp32 but, like the reference's scalar_t = half, rounds the
    tap sum, each weighted product and each partial sum of the combine to half: C 2^-24 + 8 2^-11, and its store is
    exact."""
    C = case.C
    if case.dtype == "f64":
        return (C + COMBINE_OPS) * U64 * abs_sum
    if case.dtype == "f32":
        return (C + COMBINE_OPS) * U32 * abs_sum
    if case.forward_path() == "generic":
        return (C * U32 + COMBINE_OPS * U16) * abs_sum
    return (C + COMBINE_OPS) * U32 * abs_sum + U16 * np.abs(ref) + 2.0 ** -25


def backward_bound(count, abs_sum):
    """|got - ref| allowed per element of an alt-corr gradient: an fp32 sum of n terms in any order is within
    (n + c) 2^-24 sum|terms|, c = COMBINE_OPS.  n = the oracle on all-ones inputs: every (query, tap) pair that reaches
    the element counts with the sum of its bilinear weights, which is at most one, so n is at most the number of
    contributions and the bar is no wider than the textbook one.  abs_sum = the oracle on |fmap1|, |fmap2|,
    |corr_grad|.  Forces exact zeros where nothing contributes."""
    return (count + COMBINE_OPS) * U32 * abs_sum
