"""The address model of tests/test_gpu_large_offsets.py, proved with integers only (no GPU, no tensors of the sizes
in question): for every large tensor of every case of tests/large_offset_cases.py

  * two named entries lie wholly beyond each boundary the case claims and one holds it;
  * the first and the last entry are named, and the last element of the last entry ends the tensor;
  * whichever 32-bit truncation a kernel commits, every compared element whose location that changes is looked for
    (or written) in another entry of the same tensor -- sentinel bytes, or a named entry with another seed -- or, for the
    signed truncation of an offset with bit 31 set, before the tensor's first element.  In no case at its true place: a
    kernel that truncates cannot return the true content by coincidence.

This is what makes the GPU test a test: it needs no mutant to be run."""
import numpy as np
import pytest

import corr_cases as cc
import large_offset_cases as lo

CASES = lo.CASES
LARGES = [(c, t) for c in CASES for t in c.larges]
IDS = [f"{c.id}:{t.name}" for c, t in LARGES]


def _entry_elems(t):
    return t.first(1) - t.first(0)


# ---- the layouts ----------------------------------------------------------------------------------------------------
def test_layout_formulas_are_the_row_major_offsets_of_their_shapes():
    rng = np.random.default_rng(0)
    for _ in range(200):
        cap, H1, W1, H2, W2, K = (int(v) for v in rng.integers(1, 7, 6))
        s, p, y, x, k = (int(rng.integers(0, n)) for n in (cap, H1 * W1, H2, W2, K))
        assert lo.pyramid_level(s, p, y, x, H1 * W1, H2, W2) == np.ravel_multi_index((s, p, y, x), (cap, H1 * W1, H2, W2))
        assert lo.planes(s, k, p, K, H1 * W1) == np.ravel_multi_index((s, k, p), (cap, K, H1 * W1))
        assert lo.rows(s, p, H1 * W1) == np.ravel_multi_index((s, p), (cap, H1 * W1))
        ch = int(rng.integers(0, 576))
        assert lo.mask(s, ch, p, H1 * W1) == np.ravel_multi_index((s, ch, p), (cap, 576, H1 * W1))


@pytest.mark.parametrize("case,t", LARGES, ids=IDS)
def test_entries_tile_the_tensor(case, t):
    n = _entry_elems(t)
    assert n > 0 and t.first(0) == 0
    for e in sorted(set(case.named) | {0, t.count - 1}):
        assert t.first(e) == e * n and t.last(e) == (e + 1) * n - 1
    assert t.elems == t.count * n and t.nbytes == t.elems * lo.SIZE[t.dtype]


# ---- where the named entries lie --------------------------------------------------------------------------------------
@pytest.mark.parametrize("case,t", LARGES, ids=IDS)
def test_named_entries_reach_every_claimed_boundary(case, t):
    assert t.claims == lo.CLAIMS[t.dtype][:len(t.claims)] and len(t.claims) >= 1
    assert len(t.claims) == 2 or (case.op == "corr_pyramid_forward" and t.name == "corr")   # an output of half the size
    named = [e for e in case.named if e < t.count]
    assert named == sorted(set(named)) and len(named) == len(case.named)
    for key in t.claims:
        at = t.boundary_elems(key)
        assert at < t.elems, f"{key}: the tensor ends before it"
        beyond = [e for e in named if t.first(e) >= at]
        holds = [e for e in named if t.first(e) < at <= t.last(e)]
        assert len(beyond) >= 2, (key, beyond)
        assert len(holds) == 1, (key, holds)
        # the entry that holds the boundary has elements on both sides: the boundary is no entry's first element
        assert t.first(holds[0]) < at and t.last(holds[0]) >= at


@pytest.mark.parametrize("case,t", LARGES, ids=IDS)
def test_first_and_last_entry_are_named_and_the_last_element_ends_the_tensor(case, t):
    assert 0 in case.named and t.count - 1 in case.named
    assert t.first(0) == 0
    assert t.last(t.count - 1) + 1 == t.elems          # vend of the row loads' whole-tensor guard
    assert t.elems > max(t.boundary_elems(k) for k in t.claims)


# ---- truncations ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", lo.TRUNCATIONS)
@pytest.mark.parametrize("case,t", LARGES, ids=IDS)
def test_a_truncated_location_never_holds_the_true_content(case, t, kind):
    n = _entry_elems(t)
    moved_entries, before_tensor = 0, 0
    for e in case.named:
        off = np.arange(t.first(e), t.last(e) + 1, dtype=np.int64)
        loc = lo.truncate(kind, off, t.itemsize)
        moved = loc != off
        if not moved.any():
            continue
        moved_entries += 1
        neg = loc < 0
        if neg.any():
            # only the signed truncation leaves the tensor, only downwards, and only for offsets with bit 31 set
            assert kind == lo.TRUNCATIONS[1] and bool(((off[neg] >> 31) & 1).all())
            before_tensor += int(neg.sum())
        inside = moved & ~neg
        assert bool((loc[inside] < t.elems).all())
        there = loc[inside] // n
        assert not bool((there == e).any()), "a truncated location inside the true entry"
        # what lies there: a named entry (another seed) or sentinel bytes -- both are other content than entry e's
        other = np.unique(there)
        assert all(int(o) != e and 0 <= int(o) < t.count for o in other)
    # the truncation is committed at all on these entries: every entry wholly beyond the boundary it wraps at moves
    wraps_at = {lo.TRUNCATIONS[0]: 1 << 32, lo.TRUNCATIONS[1]: 1 << 31, lo.TRUNCATIONS[2]: (1 << 32) // t.itemsize}[kind]
    if t.elems > wraps_at:
        beyond = [e for e in case.named if t.first(e) >= wraps_at]
        assert moved_entries >= len(beyond) >= 2, (kind, moved_entries, beyond)
    else:
        assert moved_entries == 0       # fp32 tensors end below 2^32 elements: their byte offsets are what wraps
    if kind != lo.TRUNCATIONS[1]:
        assert before_tensor == 0


def test_truncate_agrees_with_c_casts():
    for off in (0, 5, (1 << 31) - 1, 1 << 31, (1 << 31) + 7, (1 << 32) - 1, 1 << 32, (1 << 32) + 9, (3 << 31) + 1):
        a = np.array([off], np.int64)
        assert lo.truncate(lo.TRUNCATIONS[0], a, 2)[0] == int(a.astype(np.uint32)[0])
        assert lo.truncate(lo.TRUNCATIONS[1], a, 2)[0] == int(a.astype(np.int32)[0])
        for size in (2, 4):
            assert lo.truncate(lo.TRUNCATIONS[2], a, size)[0] == int((a * size).astype(np.uint32)[0]) // size
            assert lo.truncate(lo.TRUNCATIONS[2], off, size) == ((off * size) % (1 << 32)) // size


# ---- the table itself -------------------------------------------------------------------------------------------------
def test_every_operator_of_the_issue_has_a_half_and_an_fp32_case():
    ops = {}
    for c in CASES:
        ops.setdefault(c.op, set()).add(c.dims.get("pyramid", c.dtype))
    assert set(ops) == {"corr_volume_pyramid", "corr_pyramid_forward_slots", "corr_pyramid_forward", "corr_index_forward",
                        "corr_encode", "corr_index_backward", "altcorr_pyramid_forward", "graph_mean", "scatter_mean",
                        "upsample_disps"}
    for op, dts in ops.items():
        assert dts == ({"f16"} if op == "corr_index_backward" else {"f16", "f32"}), op
    assert len({c.id for c in CASES}) == len(CASES)


@pytest.mark.parametrize("case", [c for c in CASES if c.op.startswith("corr_") and c.path], ids=lambda c: c.id)
def test_the_dispatch_picks_the_kernel_the_case_names(case):
    H, W = case.dims["H"], case.dims["W"]
    if case.op == "corr_index_forward":
        got = cc.volume_path(case.dtype, case.dims["r"], H * W, H, W, 0, False)
    else:
        slotted = case.op == "corr_pyramid_forward_slots"
        got = cc.volume_path(case.dtype, 3, H * W, H, W, 0, slotted, "slots" if slotted else "pyramid")
    assert got == case.path
    # between them the one-level cases and the 16 x 24 pyramids reach all three fast kernels in both element sizes'
    # large buffers: small and row on half, coop on both, row on fp32


def test_the_lookup_cases_reach_every_kernel():
    seen = {(c.path, c.dtype) for c in CASES if c.op in ("corr_pyramid_forward_slots", "corr_index_forward")}
    assert {("small", "f16"), ("row", "f16"), ("coop", "f16"), ("coop", "f32"), ("row", "f32"), ("generic", "f16"),
            ("generic", "f32")} <= seen


def test_named_rows_of_graph_mean_mix_both_sides_in_every_group():
    for dt in ("f16", "f32"):
        t = lo.BY_ID[f"graph_mean-{dt}"].larges[0]
        cut = [t.boundary_elems(k) for k in t.claims]
        for g in range(lo.GM_GROUPS):
            mine = [r for k, r in enumerate(lo.GM_ROWS[dt]) if lo.gm_group(k) == g]
            assert len(mine) >= 3
            assert any(t.last(r) < cut[0] for r in mine) and any(t.first(r) >= cut[0] for r in mine)
        assert 30 <= len(lo.GM_ROWS[dt]) <= 45


def test_upsample_entries_go_to_distinct_frames():
    assert len(set(lo.UP_FRAMES)) == len(lo.UP_FRAMES) == 12 and all(0 <= f < lo.UP_BUFFER for f in lo.UP_FRAMES)
    assert all(len(v) == 12 for v in lo.UP_NAMED.values())


def test_no_case_needs_more_than_the_limit():
    for c in CASES:
        need = sum(t.nbytes for t in c.larges)
        if c.op == "corr_index_backward":      # the volume that carries the shape, its gradient, corr_grad
            need = 2 * c.larges[0].nbytes + c.larges[0].count * 49 * 384 * 2
        elif (c.dims.get("H"), c.dims.get("W")) == (lo.PYR_H, lo.PYR_W):
            need += c.larges[0].nbytes // 3   # levels 1-3 of the shared pyramid: 1/4 + 1/16 + 1/64 of level 0
            if c.op == "corr_index_forward":
                need += c.larges[0].count * 49 * lo.PYR_H * lo.PYR_W * lo.SIZE[c.dtype]   # its output at radius 3
        assert need < lo.LIMIT, (c.id, need)
