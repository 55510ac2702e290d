"""Cases of the large-tensor parity tests (tests/test_gpu_large_offsets.py): shapes at which an element offset passes
2^31 and 2^32 (half) or a byte offset passes 2^32 and 2^33 (fp32), and the entries on which the device is compared.
Plain data and integer helpers, no fixtures: tests/test_large_offsets.py proves on the CPU, with integers only, that the
named entries of every case lie where the case claims and that a kernel which truncates an offset cannot pass.

The layouts are restated by hand from include/droid_backends_hip.h and include/droid_update_hip.h, and the named
entries are written out as numbers, on purpose: a table that computed them from the boundaries would agree with itself.
"""

SENTINEL = 0x7B          # every byte that is no named entry, as in tests/test_gpu_pyramid_slots.py
SLICE = 1 << 30          # whole-buffer fills and checks go in pieces of at most this many bytes
SIZE = {"f16": 2, "f32": 4}
LIMIT = 24 << 30         # no test may hold more device memory than this

# what a case may claim for one of its tensors: (unit, offset)
BOUNDARIES = {"e31": ("element", 1 << 31), "e32": ("element", 1 << 32), "b32": ("byte", 1 << 32), "b33": ("byte", 1 << 33)}
CLAIMS = {"f16": ("e31", "e32"), "f32": ("b32", "b33")}


# ---- layouts (element offsets) --------------------------------------------------------------------------------------
def pyramid_level(slot, p, y, x, HW, H2, W2):
    """Level of a correlation pyramid [cap, H1, W1, H2, W2]: query pixel p of slot `slot`, plane position (y, x)."""
    return ((slot * HW + p) * H2 + y) * W2 + x


def planes(b, k, p, K, HW):
    """Outputs of the lookups, of corr_encode and of alt-corr [B, K, H1, W1]: channel k of entry b at pixel p."""
    return (b * K + k) * HW + p


def rows(e, c, plane):
    """graph_mean / scatter_mean: element c of row e of src [E, plane]."""
    return e * plane + c


def mask(e, ch, p, HW):
    """Upsampling mask [n, 576, H, W]."""
    return (e * 576 + ch) * HW + p


class Large:
    """One tensor of a case that crosses a boundary.  `count` entries (slots, batch entries, edges, rows, frames);
    first(e) / last(e): the offsets of the first and the last element of entry e by the layout formula; `claims`: keys
    of BOUNDARIES; `written`: the kernel under test writes it (else it reads it)."""

    def __init__(self, name, dtype, count, first, last, written, claims=None):
        self.name, self.dtype, self.count, self.first, self.last, self.written = name, dtype, count, first, last, written
        self.itemsize = SIZE[dtype]
        self.claims = CLAIMS[dtype] if claims is None else claims

    @property
    def elems(self):
        return self.last(self.count - 1) + 1

    @property
    def nbytes(self):
        return self.elems * self.itemsize

    def boundary_elems(self, key):
        unit, at = BOUNDARIES[key]
        return at if unit == "element" else at // self.itemsize


class Case:
    """id; op: the operator; dtype; named: the entries compared; larges: its large tensors; path: the kernel the
    dispatch must pick for the large tensor (None where the operator has one kernel); dims: the shape, for the test."""

    def __init__(self, id, op, dtype, named, larges, path=None, **dims):
        self.id, self.op, self.dtype, self.named, self.larges, self.path, self.dims = id, op, dtype, tuple(named), larges, path, dims

    def __repr__(self):
        return self.id


def _level0(dtype, cap, H, W, written):
    HW = H * W
    return Large("level 0", dtype, cap, lambda s: pyramid_level(s, 0, 0, 0, HW, H, W),
                 lambda s: pyramid_level(s, HW - 1, H - 1, W - 1, HW, H, W), written)


def _planes(name, dtype, B, K, HW, claims=None):
    return Large(name, dtype, B, lambda b: planes(b, 0, 0, K, HW), lambda b: planes(b, K - 1, HW - 1, K, HW), True, claims)


# ---- the 16 x 24 pyramids: 147 456 elements per slot of level 0 -------------------------------------------------------
PYR_H, PYR_W, PYR_C = 16, 24, 32
PYR_CAP = {"f16": 29131, "f32": 14567}
PYR_NAMED = {"f16": (0, 14563, 14564, 29127, 29128, 29130), "f32": (0, 7281, 7282, 14563, 14564, 14566)}
# corr_pyramid_forward without slots writes [cap, 196, 16, 24]: 75 264 elements per entry, which passes 2^31 elements
# (half) inside entry 28 532 and 2^32 bytes (fp32) inside entry 14 266 and ends below the second boundary; the entries
# beyond the first are those of the pyramid
BATCH_NAMED = {"f16": PYR_NAMED["f16"][:3] + (28532,) + PYR_NAMED["f16"][3:],
               "f32": PYR_NAMED["f32"][:3] + (14266,) + PYR_NAMED["f32"][3:]}
PYR_PATH = {"f16": "coop", "f32": "row"}     # level 0 at radius 3 (corr_cases.volume_path)

# ---- one-level lookups on the other kernels: (H, W), cap, named slots, kernel ----------------------------------------
# 8 x 8 and 16 x 16 maps give slots of 2^12 and 2^16 elements, which no boundary falls inside; 8 x 12 (96 positions, 192
# bytes per plane: the largest the small-plane kernel takes) and 16 x 12 do
LOOKUP1 = {
    "small-f16": ("f16", 8, 12, 466037, (0, 233016, 233017, 466033, 466034, 466036), "small"),
    "row-f16": ("f16", 8, 40, 41947, (0, 20971, 20972, 41943, 41944, 41946), "row"),
    "coop-f32": ("f32", 16, 12, 58258, (0, 29127, 29128, 58254, 58255, 58257), "coop"),
}

# ---- alt-corr: 8 frames of 48 x 64 x 32, output [3570, 196, 48, 64] fp32, 602 112 elements per edge -------------------
ALT_E, ALT_FRAMES, ALT_H, ALT_W, ALT_C = 3570, 8, 48, 64, 32
ALT_NAMED = (0, 1783, 1784, 3566, 3567, 3569)

# ---- graph_mean: rows of 128 x 24 x 32 = 98 304 elements; 8 groups, the named rows dealt to them in turn ---------------
GM_PLANE, GM_GROUPS = 128 * 24 * 32, 8
GM_E = {"f16": 43700, "f32": 21850}
GM_ROWS = {
    "f16": (0, 1, 2, 4095, 8191, 10922, 10923, 16383, 16384, 20000, 21843, 21844, 21845,
            21846, 21847, 24000, 28000, 30000, 32767, 32768, 36000, 40000, 43000, 43688, 43689, 43690,
            43691, 43692, 43693, 43694, 43695, 43696, 43697, 43698, 43699),
    "f32": (0, 1, 2, 4095, 5000, 6000, 7000, 8191, 9000, 10920, 10921, 10922,
            10923, 10924, 12000, 13000, 14000, 15000, 16383, 16384, 17000, 18000, 19000, 20000, 21843, 21844, 21845,
            21846, 21847, 21848, 21849),
}


def gm_group(k):
    """Group of the k-th named row: dealt round-robin, so every group holds rows below, between and beyond the boundaries."""
    return k % GM_GROUPS


# ---- upsampling: mask [n, 576, 16, 24], 221 184 elements per entry; 19 419 (9 710) entries reach the boundary but leave
# the entry that holds it the last one, so three (two) more follow
UP_H, UP_W, UP_BUFFER = 16, 24, 16
UP_N = {"f16": 19422, "f32": 9712}
UP_NAMED = {"f16": (0, 1, 5000, 9708, 9709, 9710, 15000, 19417, 19418, 19419, 19420, 19421),
            "f32": (0, 1, 2500, 4853, 4854, 4855, 6000, 7000, 9708, 9709, 9710, 9711)}
UP_FRAMES = (7, 2, 9, 15, 0, 4, 11, 13, 5, 1, 14, 8)     # distinct frames of the 16-frame buffer, one per named entry


def _cases():
    out = []
    HW = PYR_H * PYR_W
    for dt in ("f16", "f32"):
        cap, named = PYR_CAP[dt], PYR_NAMED[dt]
        dims = dict(H=PYR_H, W=PYR_W, cap=cap)
        for mode in ("offset", "slots"):
            out.append(Case(f"build-{mode}-{dt}", "corr_volume_pyramid", dt, named,
                            [_level0(dt, cap, PYR_H, PYR_W, True)], mode=mode, **dims))
        out.append(Case(f"lookup-slots-{dt}", "corr_pyramid_forward_slots", dt, named,
                        [_level0(dt, cap, PYR_H, PYR_W, False)], PYR_PATH[dt], **dims))
        out.append(Case(f"lookup-batch-{dt}", "corr_pyramid_forward", dt, BATCH_NAMED[dt],
                        [_level0(dt, cap, PYR_H, PYR_W, False), _planes("corr", dt, cap, 4 * 49, HW, CLAIMS[dt][:1])],
                        PYR_PATH[dt], **dims))
        for r, path in ((3, PYR_PATH[dt]), (2, "generic")):
            out.append(Case(f"index-r{r}-{dt}", "corr_index_forward", dt, named,
                            [_level0(dt, cap, PYR_H, PYR_W, False)], path, r=r, **dims))
        for layout in ("2hw", "hw2"):
            out.append(Case(f"encode-{layout}-{dt}", "corr_encode", dt, named,
                            [_level0(dt, cap, PYR_H, PYR_W, False)], layout=layout, **dims))
    for key, (dt, H, W, cap, named, path) in LOOKUP1.items():
        out.append(Case(f"lookup1-{key}", "corr_pyramid_forward_slots", dt, named, [_level0(dt, cap, H, W, False)], path,
                        H=H, W=W, cap=cap))
    out.append(Case("backward-f16", "corr_index_backward", "f16", PYR_NAMED["f16"],
                    [_level0("f16", PYR_CAP["f16"], PYR_H, PYR_W, True)], H=PYR_H, W=PYR_W, cap=PYR_CAP["f16"]))
    for dt, path in (("f16", "wave_f16"), ("f32", "mfma_f32")):      # dtype of the feature pyramid; the output is fp32
        out.append(Case(f"altcorr-{dt}", "altcorr_pyramid_forward", "f32", ALT_NAMED,
                        [_planes("corr", "f32", ALT_E, 4 * 49, ALT_H * ALT_W)], path, pyramid=dt))
    for dt in ("f16", "f32"):
        for op in ("graph_mean", "scatter_mean"):
            E = GM_E[dt]
            out.append(Case(f"{op}-{dt}", op, dt, GM_ROWS[dt],
                            [Large("src", dt, E, lambda e: rows(e, 0, GM_PLANE), lambda e: rows(e, GM_PLANE - 1, GM_PLANE), False)],
                            E=E))
    for dt in ("f16", "f32"):
        n, hw = UP_N[dt], UP_H * UP_W
        out.append(Case(f"upsample-{dt}", "upsample_disps", dt, UP_NAMED[dt],
                        [Large("mask", dt, n, lambda e: mask(e, 0, 0, hw), lambda e: mask(e, 575, hw - 1, hw), False)], n=n))
    return out


CASES = _cases()
BY_ID = {c.id: c for c in CASES}


# ---- integers only: where a truncated offset lands --------------------------------------------------------------------
TRUNCATIONS = ("element offset mod 2^32", "element offset as signed 32 bits", "byte offset mod 2^32")


def truncate(kind, off, itemsize):
    """Element location a kernel reaches for the element offset `off` (a Python int or a numpy int64 array) when it
    commits truncation `kind`.  Negative: before the first element of the tensor."""
    if kind == TRUNCATIONS[0]:
        return off & 0xFFFFFFFF
    if kind == TRUNCATIONS[1]:
        low = off & 0xFFFFFFFF
        return low - ((low >> 31) << 32)
    return ((off * itemsize) & 0xFFFFFFFF) // itemsize
