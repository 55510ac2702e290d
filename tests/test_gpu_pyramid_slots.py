"""The slot-indexed pyramid on the device: corr_volume_pyramid(..., slots=) and corr_pyramid_forward(..., slots=)
against the existing entry points (which the rest of the suite pins to the oracle), and PyramidStore against the stock
sequence corr_volume_pyramid + torch.cat + boolean indexing + corr_pyramid_forward.

Indirection changes addresses, not arithmetic: every comparison is on the raw bits, with no tolerance."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
SIZES = [(48, 64), (30, 40)]   # 48x64 x 4 levels: row-load, cooperative and small-plane kernels; 30x40: HW % 64 != 0
INTS = {1: torch.uint8, 2: torch.int16, 4: torch.int32, 8: torch.int64}
SENTINEL = 0x7B


def _bits(x):
    return x.contiguous().view(INTS[x.element_size()])


def _same(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and torch.equal(_bits(a), _bits(b))


def _idx(v):
    return torch.tensor(v, dtype=torch.int64, device=DEV)


def _fmaps(seed, nbuf, ncam, C, h, w, dtype):
    g = torch.Generator().manual_seed(seed)
    return torch.randn((nbuf, ncam, C, h, w), generator=g).to(dtype).to(DEV)


def _coords(seed, B, h, w):
    """[B,2,h,w] at level-0 scale: a third of the queries near their own pixel, a third anywhere in a frame 10 pixels
    wider than the map (windows hang over every border at every level), the rest far outside (empty windows)."""
    rng = np.random.default_rng(seed)
    gy, gx = np.meshgrid(np.arange(h, dtype=np.float64), np.arange(w, dtype=np.float64), indexing="ij")
    kind = rng.integers(0, 3, (B, h, w))
    near = np.stack([gx + rng.normal(0, 3, (B, h, w)), gy + rng.normal(0, 3, (B, h, w))], 1)
    wide = np.stack([rng.uniform(-10, w + 10, (B, h, w)), rng.uniform(-10, h + 10, (B, h, w))], 1)
    far = np.stack([rng.choice([-300.0, 1e9, w + 77.7], (B, h, w)), rng.choice([-1e9, h + 40.2, -55.5], (B, h, w))], 1)
    c = np.where(kind[:, None] == 0, near, np.where(kind[:, None] == 1, wide, far)).astype(np.float32)
    # the two ends of the buffer: the first plane's first row entered from the left, the last plane's last row left on
    # the right -- the wide row loads there would leave the tensor (the whole-tensor guards)
    c[:, :, 0, 0] = [0.5, 3.5]
    c[:, :, h - 1, w - 1] = [w - 0.5, h - 0.5]
    return torch.from_numpy(c).to(DEV)


def _random_pyramid(seed, cap, h, w, dtype, levels=4):
    g = torch.Generator(device=DEV).manual_seed(seed)
    return [torch.randn((cap, h, w, h >> l, w >> l), generator=g, dtype=torch.float32, device=DEV).to(dtype)
            for l in range(levels)]


def _poison_free_memory(shape, dtype):
    """Leave NaN bits in the block the allocator hands out next for this shape: 'zeros' must have been written."""
    junk = torch.full(shape, float("nan"), dtype=dtype, device=DEV)
    del junk


# ---------------------------------------------------------------------------------------------------- build
@pytest.mark.parametrize("dtype", [torch.float16, torch.float32])
@pytest.mark.parametrize("h,w", SIZES)
def test_build_writes_the_named_slots_and_nothing_else(backends, dtype, h, w):
    fmaps = _fmaps(3, 5, 2, 128, h, w, dtype)
    ii, jj = _idx([0, 2, 1, 4, 3, 0]), _idx([3, 2, 4, 0, 3, 1])   # edges 1 and 4 are stereo (ii == jj: camera 1)
    cap = 9
    slots = [5, -1, 0, cap, cap - 1, 2]                           # edges 1 and 3 name no slot: skipped
    want = backends.corr_volume_pyramid(fmaps, ii, jj, 4)
    out = [torch.empty((cap, h, w, h >> l, w >> l), dtype=dtype, device=DEV) for l in range(4)]
    for o in out:
        o.view(torch.uint8).fill_(SENTINEL)
    got = backends.corr_volume_pyramid(fmaps, ii, jj, 4, out=out, slots=_idx(slots))
    torch.cuda.synchronize()
    assert all(g.data_ptr() == o.data_ptr() for g, o in zip(got, out))
    written = {s: e for e, s in enumerate(slots) if 0 <= s < cap}
    for l in range(4):
        for s in range(cap):
            if s in written:
                assert _same(out[l][s], want[l][written[s]]), f"level {l} slot {s} != edge {written[s]}"
            else:
                assert bool((out[l][s].view(torch.uint8) == SENTINEL).all()), f"level {l} slot {s} was touched"
    assert bool(want[0][1].any()) and not _same(want[0][1], want[0][4])   # the stereo edges are real edges


@pytest.mark.parametrize("dtype", [torch.float16, torch.float32])
def test_build_with_only_out_of_range_slots_changes_nothing(backends, dtype):
    h, w, cap = 30, 40, 3
    fmaps = _fmaps(4, 3, 1, 64, h, w, dtype)
    out = [torch.empty((cap, h, w, h >> l, w >> l), dtype=dtype, device=DEV) for l in range(4)]
    for o in out:
        o.view(torch.uint8).fill_(SENTINEL)
    backends.corr_volume_pyramid(fmaps, _idx([0, 1, 2]), _idx([1, 2, 0]), 4, out=out, slots=_idx([-1, cap, 2 ** 40]))
    torch.cuda.synchronize()
    for o in out:
        assert bool((o.view(torch.uint8) == SENTINEL).all())


def test_build_keyword_refusals(backends):
    fmaps = _fmaps(5, 3, 1, 32, 8, 8, torch.float16)
    out = [torch.empty((4, 8, 8, 8 >> l, 8 >> l), dtype=torch.float16, device=DEV) for l in range(4)]
    ix = _idx([0, 1])
    with pytest.raises(RuntimeError, match="slots needs out"):
        backends.corr_volume_pyramid(fmaps, ix, ix, 4, slots=ix)
    with pytest.raises(RuntimeError, match="exclude"):
        backends.corr_volume_pyramid(fmaps, ix, ix, 4, out=out, offset=1, slots=ix)
    with pytest.raises(RuntimeError, match=r"slots must be \[E\]"):
        backends.corr_volume_pyramid(fmaps, ix, ix, 4, out=out, slots=_idx([0]))
    with pytest.raises(RuntimeError, match="int64"):
        backends.corr_volume_pyramid(fmaps, ix, ix, 4, out=out, slots=ix.int())


# ---------------------------------------------------------------------------------------------------- lookup
@pytest.mark.parametrize("radius", [3, 4])
@pytest.mark.parametrize("dtype", [torch.float16, torch.float32, torch.float64])
@pytest.mark.parametrize("h,w", SIZES)
def test_lookup_through_slots_equals_lookup_of_the_gathered_copy(backends, dtype, radius, h, w):
    cap = 7
    pyr = _random_pyramid(11, cap, h, w, dtype)
    slots = _idx([cap - 1, 0, 3, 3, 5, 0])            # both ends of the buffer, and two entries reading one slot
    coords = _coords(12, len(slots), h, w)
    want, = backends.corr_pyramid_forward([p[slots] for p in pyr], coords, radius)
    got, = backends.corr_pyramid_forward(pyr, coords, radius, slots=slots)
    torch.cuda.synchronize()
    assert got.shape == (len(slots), 4 * (2 * radius + 1) ** 2, h, w)
    assert _same(got, want)
    assert bool(want.any()) and not _same(got[2], got[3])   # same slot, different coordinates: really looked up


@pytest.mark.parametrize("dtype", [torch.float16, torch.float32, torch.float64])
@pytest.mark.parametrize("h,w", SIZES)
def test_lookup_of_an_out_of_range_slot_gives_zeros_and_spares_its_neighbours(backends, dtype, h, w):
    cap = 4
    pyr = _random_pyramid(13, cap, h, w, dtype)
    slots = [0, -1, cap - 1, cap, 2, 2 ** 40]
    good = [b for b, s in enumerate(slots) if 0 <= s < cap]
    coords = _coords(14, len(slots), h, w)
    want, = backends.corr_pyramid_forward([p[_idx([slots[b] for b in good])] for p in pyr], coords[good].contiguous(), 3)
    _poison_free_memory((len(slots), 4 * 49, h, w), dtype)
    got, = backends.corr_pyramid_forward(pyr, coords, 3, slots=_idx(slots))
    torch.cuda.synchronize()
    assert _same(got[good], want)
    for b in range(len(slots)):
        if b not in good:
            assert not bool(_bits(got[b]).any()), f"entry {b} (slot {slots[b]}) is not all zero bits"


def test_lookup_keyword_refusals(backends):
    pyr = _random_pyramid(15, 3, 8, 8, torch.float16)
    coords = _coords(16, 2, 8, 8)
    with pytest.raises(RuntimeError, match="int64"):
        backends.corr_pyramid_forward(pyr, coords, 3, slots=_idx([0, 1]).int())
    with pytest.raises(RuntimeError, match="coords must be"):
        backends.corr_pyramid_forward(pyr, coords, 3, slots=_idx([0, 1, 2]))
    out, = backends.corr_pyramid_forward(pyr, coords[:0].contiguous(), 3, slots=_idx([]))
    assert out.shape == (0, 4 * 49, 8, 8)


# ---------------------------------------------------------------------------------------------------- store
class _Stock:
    """What factor_graph.py does today, on the project's existing entry points."""

    def __init__(self, backends, fmaps):
        self.db, self.fmaps, self.pyr = backends, fmaps, None

    def add(self, ii, jj):
        new = self.db.corr_volume_pyramid(self.fmaps, ii, jj, 4)
        self.pyr = new if self.pyr is None else [torch.cat([a, b], 0) for a, b in zip(self.pyr, new)]   # CorrBlock.cat

    def keep(self, mask):
        self.pyr = [p[mask] for p in self.pyr]                                                      # __getitem__

    def __call__(self, coords):
        c = coords.permute(0, 1, 4, 2, 3).contiguous().view(coords.shape[1], 2, *coords.shape[2:4])
        return self.db.corr_pyramid_forward(self.pyr, c, 3)[0][None]


@pytest.mark.parametrize("h,w", SIZES)
def test_store_replay_equals_the_stock_sequence_and_moves_no_bytes(backends, h, w):
    from droid_backends.pyramid_store import PyramidStore
    rng = np.random.default_rng(21)
    nbuf = 10
    fmaps = _fmaps(22, nbuf, 2, 128, h, w, torch.float16)
    store, stock = PyramidStore(fmaps, cap=4), _Stock(backends, fmaps)   # the first add (6 edges) forces a growth
    slot_bytes = fmaps.element_size() * (h * w) ** 2        # level 0 of one edge
    nonempty_lookups = plain_adds = 0
    for step in range(20):
        # ---- rm_factors: 0-8 of the edges held
        E = len(store)
        if E:
            mask = np.ones(E, bool)
            mask[rng.choice(E, size=min(E, int(rng.integers(0, 9))), replace=False)] = False
            before = [p.clone() for p in store.pyramid]
            ptrs = [p.data_ptr() for p in store.pyramid]
            torch.cuda.synchronize()
            torch.cuda.reset_peak_memory_stats()
            base = torch.cuda.memory_allocated()
            store.keep(torch.from_numpy(mask).to(DEV) if step % 2 else mask.tolist())   # device and host masks
            torch.cuda.synchronize()
            assert torch.cuda.max_memory_allocated() - base < slot_bytes // 4, "keep allocated pyramid-sized memory"
            assert [p.data_ptr() for p in store.pyramid] == ptrs
            for l, (a, b) in enumerate(zip(before, store.pyramid)):
                assert _same(a, b), f"step {step}: keep changed bytes of level {l}"
            del before
            stock.keep(torch.from_numpy(mask).to(DEV))
            assert len(store) == int(mask.sum())
        # ---- add_factors: 0-8 new edges
        n = 6 if step == 0 else int(rng.integers(0, 9))
        if n:
            ii = rng.integers(0, nbuf, n)
            jj = np.where(rng.random(n) < 0.2, ii, rng.integers(0, nbuf, n))   # some stereo edges
            grows, held = store.grows, set(store.table.slots)
            before = [p.clone() for p in store.pyramid]
            store.add(_idx(ii), _idx(jj))
            stock.add(_idx(ii), _idx(jj))
            torch.cuda.synchronize()
            if store.grows == grows:
                fresh = set(store.table.slots) - held
                assert len(fresh) == n
                plain_adds += 1
                old = _idx(sorted(set(range(store.cap)) - fresh))
                for l, (a, b) in enumerate(zip(before, store.pyramid)):
                    assert _same(a[old], b[old]), f"step {step}: add changed a slot it did not allocate (level {l})"
            del before
        # ---- update: one lookup
        E = len(store)
        assert E == (0 if stock.pyr is None else stock.pyr[0].shape[0])
        if E:
            coords = _coords(100 + step, E, h, w).permute(0, 2, 3, 1)[None].contiguous()   # [1,E,h,w,2]
            ptrs = [p.data_ptr() for p in store.pyramid]
            got, want = store(coords), stock(coords)
            torch.cuda.synchronize()
            assert got.shape == (1, E, 4 * 49, h, w)
            assert _same(got, want), f"step {step}: lookup through the store differs from the stock sequence"
            assert [p.data_ptr() for p in store.pyramid] == ptrs
            nonempty_lookups += 1
    assert store.grows >= 1 and plain_adds >= 5 and nonempty_lookups >= 15, (store.grows, plain_adds, nonempty_lookups)
