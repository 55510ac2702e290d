"""The correlation pyramids of a factor graph's edges in capacity buffers, addressed through a slot list.

`FactorGraph` keeps one all-pairs pyramid per edge in a `CorrBlock` (droid_slam/modules/corr.py:23-60): `add_factors`
concatenates (`CorrBlock.cat`, :52-55) and `rm_factors` indexes with a boolean mask (`self.corr = self.corr[~mask]`,
factor_graph.py:151-152 -> `__getitem__`, :57-60).  Both re-materialise every level of every surviving edge, about
25 MB per edge at 48x64 in half precision.  Here an edge lives in ANY slot of buffers allocated once, the lookup and
the build take the slot of each edge from a small int64 list (droid_corr_pyramid_forward_slots,
droid_corr_volume_pyramid_slots), and the order of that list is the order of the edges: dropping edges edits the
list, adding edges fills free slots, and no pyramid bytes move.

`SlotTable` is the bookkeeping alone (plain Python, no device, no library call); `PyramidStore` owns the buffers and is
what a caller puts where `self.corr` is.
"""
from __future__ import annotations

import heapq

import torch

from . import corr_pyramid_forward, corr_volume_pyramid


class SlotTable:
    """Which slot of `cap` each edge occupies, in edge order.

    The order of `slots` is the order `CorrBlock` gives its rows: `alloc` appends like `cat`, `keep(mask)` orders the
    survivors like `x[mask]`.  `alloc` hands out the lowest free slots in ascending order, so a sequence of calls
    always produces the same layout."""

    def __init__(self, cap):
        cap = int(cap)
        if cap < 1:
            raise ValueError(f"SlotTable: cap must be at least 1, got {cap}")
        self.cap = cap
        self._slots = []
        self._free = list(range(cap))   # a heap; an ascending list is one

    def __len__(self):
        return len(self._slots)

    @property
    def slots(self):
        """The slots of the live edges, in edge order (a copy)."""
        return list(self._slots)

    @property
    def free(self):
        return len(self._free)

    def alloc(self, n):
        """Append n edges; returns their slots, the n lowest free ones in ascending order."""
        n = int(n)
        if n < 0:
            raise ValueError("SlotTable.alloc: n must not be negative")
        if n > len(self._free):
            raise RuntimeError(f"SlotTable.alloc: {n} edges asked for, {len(self._free)} of {self.cap} slots free "
                               "(grow the table first)")
        new = [heapq.heappop(self._free) for _ in range(n)]
        self._slots.extend(new)
        return new

    def keep(self, mask):
        """Drop the edges whose mask entry is false; returns the slots they gave back."""
        mask = [bool(m) for m in mask]
        if len(mask) != len(self._slots):
            raise ValueError(f"SlotTable.keep: mask has {len(mask)} entries for {len(self._slots)} edges")
        freed = [s for s, m in zip(self._slots, mask) if not m]
        self._slots = [s for s, m in zip(self._slots, mask) if m]
        for s in freed:
            heapq.heappush(self._free, s)
        return freed

    def grow(self, new_cap):
        """Enlarge the table to new_cap slots; the live edges keep theirs."""
        new_cap = int(new_cap)
        if new_cap < self.cap:
            raise ValueError(f"SlotTable.grow: {new_cap} is below the capacity {self.cap}")
        for s in range(self.cap, new_cap):
            heapq.heappush(self._free, s)
        self.cap = new_cap


class PyramidStore:
    """`self.corr` of a factor graph on capacity buffers: `add` for `CorrBlock(fmap1, fmap2)` + `cat`, `keep` for
    `self.corr[mask]`, `store(coords)` for `self.corr(coords)`.

    fmaps is the feature buffer as DepthVideo holds it ([nbuf, ncam, C, h, w] or [nbuf, C, h, w], half or fp32); it is
    read in place by every `add`.  The buffers are allocated once; an `add` beyond the capacity doubles them with one
    copy per level (counted in `grows`).  `keep` and the lookup neither allocate nor copy pyramid memory."""

    def __init__(self, fmaps, cap, levels=4, radius=3):
        self.fmaps = fmaps
        self.levels, self.radius = int(levels), int(radius)
        h, w = int(fmaps.shape[-2]), int(fmaps.shape[-1])
        self._shapes = [(h, w, h >> l, w >> l) for l in range(self.levels)]
        self.table = SlotTable(cap)
        self.pyramid = [torch.empty((self.table.cap,) + s, dtype=fmaps.dtype, device=fmaps.device) for s in self._shapes]
        self.grows = 0
        self._slots_dev = None   # device copy of table.slots, refreshed when the list changes

    def __len__(self):
        return len(self.table)

    @property
    def cap(self):
        return self.table.cap

    def _slots_to_device(self, slots):
        return torch.tensor(slots, dtype=torch.int64, device=self.fmaps.device)

    def _grow(self, need):
        old_cap, new_cap = self.table.cap, self.table.cap
        while new_cap < need:
            new_cap *= 2
        for l, s in enumerate(self._shapes):
            new = torch.empty((new_cap,) + s, dtype=self.fmaps.dtype, device=self.fmaps.device)
            new[:old_cap].copy_(self.pyramid[l])
            self.pyramid[l] = new
        self.table.grow(new_cap)
        self.grows += 1

    def add(self, ii, jj):
        """Build the pyramids of the edges ii -> jj ([n] int64 on the device) behind the edges held."""
        n = int(ii.shape[0])
        if n == 0:
            return
        if n > self.table.free:
            self._grow(len(self.table) + n)
        new = self._slots_to_device(self.table.alloc(n))
        corr_volume_pyramid(self.fmaps, ii, jj, self.levels, out=self.pyramid, slots=new)
        self._slots_dev = self._slots_to_device(self.table.slots)

    def keep(self, mask):
        """Keep the edges where mask ([E] bool, on the host or on the device) is true, in their order."""
        if hasattr(mask, "tolist"):
            mask = mask.tolist()   # the one device -> host read, which boolean indexing pays as well
        if self.table.keep(mask):
            self._slots_dev = self._slots_to_device(self.table.slots)

    def __call__(self, coords):
        """coords [1, E, h, w, 2] float32 -> [1, E, levels (2r+1)^2, h, w], like CorrBlock.__call__ (corr.py:40-50)."""
        batch, num, ht, wd, _ = coords.shape
        if batch != 1 or num != len(self.table):
            raise RuntimeError(f"PyramidStore: coords must be [1, {len(self.table)}, h, w, 2], got {tuple(coords.shape)}")
        if num == 0:
            return torch.empty((1, 0, self.levels * (2 * self.radius + 1) ** 2, ht, wd), dtype=self.fmaps.dtype,
                               device=self.fmaps.device)
        c = coords.permute(0, 1, 4, 2, 3).contiguous().view(num, 2, ht, wd)
        corr, = corr_pyramid_forward(self.pyramid, c, self.radius, slots=self._slots_dev)
        return corr[None]

    def encode(self, coords1, enc):
        """coords1 [1, E, h, w, 2] float32 as `reproject` returns it, enc a `CorrEncoder` -> [E, 128, h, w] half:
        `corr_encoder[0:2]` of `self(coords1)` in one launch, without the lookup tensor and without the permuted copy of
        the coordinates (droid_corr_encode).  What `corr_encoder[2:]` takes next."""
        if coords1.dim() != 5 or coords1.shape[0] != 1 or coords1.shape[1] != len(self.table) or coords1.shape[4] != 2:
            raise RuntimeError(f"PyramidStore.encode: coords1 must be [1, {len(self.table)}, h, w, 2], "
                               f"got {tuple(coords1.shape)}")
        if len(self.table) == 0:
            return torch.empty((0, 128) + tuple(coords1.shape[2:4]), dtype=torch.float16, device=self.fmaps.device)
        return enc(self.pyramid, coords1[0], slots=self._slots_dev, layout="hw2")
