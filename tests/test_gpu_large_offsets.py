"""Tensors beyond 2^31 and 2^32 elements and beyond 4 GiB and 8 GiB on the device: the cases of
tests/large_offset_cases.py (tests/test_large_offsets.py proves on the CPU where their named entries lie and that a kernel
which truncates an offset cannot pass).

Indirection and batch position change addresses, not arithmetic: on the named entries the large call must return, bit for
bit, what the same operator returns on a small tensor that holds copies of only those entries -- the call the rest of the
suite pins to the oracle, and which one case per operator pins again here.  No tolerance, no element left out.  Every
byte that is no named entry holds 0x7B before the call and, where the operator must not write it, after it; whole-buffer
fills and checks go in pieces of at most 2^30 bytes.  At most one large buffer lives at a time."""
import time

import numpy as np
import pytest
import torch

import corr_cases as cc
import corr_encode_ref as cer
import cvx_upsample_ref as cur
import graph_mean_ref as gmr
import large_offset_cases as lo
from test_gpu_corr_encode import _params, _relu, _selection, _worst_ratio
from test_gpu_corr_volume import _check as _check_build
from test_gpu_pyramid_slots import _coords as _mix_coords

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
TDT = {"f16": torch.float16, "f32": torch.float32}
NDT = {"f16": np.float16, "f32": np.float32}
INTS = {2: torch.int16, 4: torch.int32}
DTYPES = ["f16", "f32"]


# ---- helpers ----------------------------------------------------------------------------------------------------------
def _same(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and torch.equal(a.contiguous().view(INTS[a.element_size()]),
                                                                     b.contiguous().view(INTS[b.element_size()]))


def _idx(v):
    return torch.tensor(list(v), dtype=torch.int64, device=DEV)


def _raw(t):
    assert t.is_contiguous()
    return t.view(-1).view(torch.uint8)


def _fill(t, value=lo.SENTINEL):
    b = _raw(t)
    for a in range(0, b.numel(), lo.SLICE):
        b[a:a + lo.SLICE].fill_(value)


def _foreign_bytes(t, entries, value=lo.SENTINEL):
    """8-byte words of t outside `entries` (indices along dimension 0) in which a byte does not hold `value`.  Compared
    as words so that the comparison's own result stays at an eighth of a piece."""
    w = _raw(t).view(torch.int64)
    per, step = w.numel() // t.shape[0], lo.SLICE // 8
    assert per * t.shape[0] * 8 == t.numel() * t.element_size()
    word = int.from_bytes(bytes([value]) * 8, "little", signed=True)
    bad = torch.zeros((), dtype=torch.int64, device=DEV)
    pos = 0
    for e in sorted(entries) + [t.shape[0]]:
        for a in range(pos, e * per, step):
            bad += torch.count_nonzero(w[a:min(a + step, e * per)] != word)
        pos = (e + 1) * per
    return int(bad)


def _poison(shape, dtype):
    """Sentinel bytes in the block the allocator hands out next for this shape: an output must have been written."""
    junk = torch.empty(shape, dtype=dtype, device=DEV)
    _fill(junk)
    del junk


def _begin(case, need):
    """Skips (with the numbers) when the device cannot hold the case; the clock of the case's report line."""
    torch.cuda.synchronize()
    torch.cuda.empty_cache()
    free, total = torch.cuda.mem_get_info()
    assert need <= lo.LIMIT, (case.id, need)
    if need > free:
        pytest.skip(f"{case.id}: needs {need} bytes, {free} of {total} are free")
    torch.cuda.reset_peak_memory_stats()
    return time.perf_counter()


def _report(case, shape, t0):
    torch.cuda.synchronize()
    large = " + ".join(f"{t.name} {t.nbytes} B reaching {'/'.join(t.claims)}" for t in case.larges)
    print(f"LARGE {case.id}: {case.op} {shape}; {large}; kernel {case.path or '-'}; "
          f"peak {torch.cuda.max_memory_allocated()} B; {time.perf_counter() - t0:.2f} s")


def _pyramid_bytes(dt):
    hw = lo.PYR_H * lo.PYR_W
    return sum(lo.PYR_CAP[dt] * hw * (lo.PYR_H >> l) * (lo.PYR_W >> l) for l in range(4)) * lo.SIZE[dt]


class _Big:
    """Holds at most one large buffer: the 16 x 24 pyramid of one dtype, its named slots filled from the small build."""

    def __init__(self):
        self.key = self.val = None

    def drop(self):
        self.key = self.val = None
        torch.cuda.synchronize()
        torch.cuda.empty_cache()

    def pyramid(self, db, dt):
        if self.key != dt:
            self.drop()
            H, W, cap, named = lo.PYR_H, lo.PYR_W, lo.PYR_CAP[dt], lo.PYR_NAMED[dt]
            g = torch.Generator().manual_seed(31)
            fmaps = torch.randn((4, 1, lo.PYR_C, H, W), generator=g).to(torch.float16).to(TDT[dt]).to(DEV)
            ii, jj = [0, 1, 2, 3, 0, 2], [1, 2, 3, 0, 3, 1]
            small = db.corr_volume_pyramid(fmaps, _idx(ii), _idx(jj), 4)
            buf = [torch.empty((cap, H, W, H >> l, W >> l), dtype=TDT[dt], device=DEV) for l in range(4)]
            for b in buf:
                _fill(b)
            self.key, self.val = dt, dict(buf=buf, small=small, fmaps=fmaps, ii=ii, jj=jj, named=named)
            self.restore()
        return self.val

    def restore(self):
        p = self.val
        for l in range(4):
            for k, s in enumerate(p["named"]):
                p["buf"][l][s].copy_(p["small"][l][k])
        torch.cuda.synchronize()


@pytest.fixture(scope="module")
def big():
    b = _Big()
    yield b
    b.drop()


def _pyramid(backends, big, case, extra=0):
    """The pyramid of the case's dtype (built once while consecutive cases share it) and the case's clock; `extra`:
    bytes the case allocates besides."""
    have = big.key == case.dtype
    t0 = _begin(case, extra + (0 if have else _pyramid_bytes(case.dtype)))
    return big.pyramid(backends, case.dtype), t0


def _tiled_coords(small, count, named):
    """[count, ...]: the small coordinate sets in turn, entry named[k] holding set k."""
    big = small[torch.arange(count, device=DEV) % small.shape[0]].contiguous()
    for k, b in enumerate(named):
        big[b] = small[k]
    return big


def _oracle_lookup(oracle, levels, coords, r):
    """corr_pyramid_forward of numpy levels [B,h,w,h>>l,w>>l] by oracle/corr.py: [B, levels (2r+1)^2, h, w]."""
    B, _, H, W = coords.shape
    with np.errstate(invalid="ignore", over="ignore"):
        return np.concatenate([oracle.corr_index_forward(v, coords * np.float32(1.0 / (1 << l)), r).reshape(B, -1, H, W)
                               for l, v in enumerate(levels)], 1)


# ---- corr_volume_pyramid ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", ["slots", "offset"])
@pytest.mark.parametrize("dt", DTYPES)
def test_build_writes_the_named_slots_beyond_4_gib_and_nothing_else(backends, big, dt, mode):
    case = lo.BY_ID[f"build-{mode}-{dt}"]
    p, t0 = _pyramid(backends, big, case)
    buf, small, named, ii, jj = p["buf"], p["small"], list(p["named"]), p["ii"], p["jj"]
    assert all(not _same(small[0][a], small[0][b]) for a in range(6) for b in range(a))     # six different edges
    try:
        for l in range(4):
            for s in named:
                _fill(buf[l][s])
        if mode == "slots":
            backends.corr_volume_pyramid(p["fmaps"], _idx(ii), _idx(jj), 4, out=buf, slots=_idx(named))
        else:   # one call per run of consecutive slots
            k = 0
            while k < len(named):
                n = 1
                while k + n < len(named) and named[k + n] == named[k] + n:
                    n += 1
                backends.corr_volume_pyramid(p["fmaps"], _idx(ii[k:k + n]), _idx(jj[k:k + n]), 4, out=buf, offset=named[k])
                k += n
        torch.cuda.synchronize()
        for l in range(4):
            for k, s in enumerate(named):
                assert _same(buf[l][s], small[l][k]), f"level {l} slot {s} != edge {k}"
            assert _foreign_bytes(buf[l], named) == 0, f"level {l}: a slot that was not named was written"
    finally:
        big.restore()
    if mode == "slots":   # the small call against the restatement of the contract, at the bars of test_gpu_corr_volume.py
        dev = _check_build(backends, p["fmaps"].cpu().numpy(), ii, jj, 4, NDT[dt], case.id)
        assert all(np.array_equal(d, s.cpu().numpy()) for d, s in zip(dev, small))
    _report(case, tuple(buf[0].shape), t0)


# ---- lookups through slots --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dt", DTYPES)
def test_lookup_through_slots_beyond_4_gib(backends, oracle, big, dt):
    case = lo.BY_ID[f"lookup-slots-{dt}"]
    p, t0 = _pyramid(backends, big, case)
    buf, small, named = p["buf"], p["small"], p["named"]
    H, W = lo.PYR_H, lo.PYR_W
    assert cc.volume_path(dt, 3, H * W, H, W, buf[0].data_ptr() % 16, True, "slots") == case.path
    coords = _mix_coords(41, len(named), H, W)
    want, = backends.corr_pyramid_forward(small, coords, 3)
    _poison(tuple(want.shape), want.dtype)
    got, = backends.corr_pyramid_forward(buf, coords, 3, slots=_idx(named))
    torch.cuda.synchronize()
    assert _same(got, want) and bool(want.any())
    ref = _oracle_lookup(oracle, [s.cpu().numpy() for s in small], coords.cpu().numpy(), 3)
    assert np.array_equal(want.cpu().numpy(), ref)
    for l in range(4):
        assert _foreign_bytes(buf[l], named) == 0
    _report(case, tuple(buf[0].shape), t0)


@pytest.mark.parametrize("key", list(lo.LOOKUP1))
def test_one_level_lookup_on_each_kernel_beyond_4_gib(backends, oracle, big, key):
    case = lo.BY_ID[f"lookup1-{key}"]
    dt, H, W, cap, named, path = lo.LOOKUP1[key]
    big.drop()
    t0 = _begin(case, case.larges[0].nbytes)
    buf = torch.empty((cap, H, W, H, W), dtype=TDT[dt], device=DEV)
    assert cc.volume_path(dt, 3, H * W, H, W, buf.data_ptr() % 16, True, "slots") == path
    _fill(buf)
    g = torch.Generator(device=DEV)
    small = torch.stack([torch.randn((H, W, H, W), generator=g.manual_seed(50 + k), device=DEV).to(TDT[dt])
                         for k in range(len(named))])
    for k, s in enumerate(named):
        buf[s].copy_(small[k])
    coords = _mix_coords(43, len(named), H, W)
    want, = backends.corr_pyramid_forward([small], coords, 3)
    _poison(tuple(want.shape), want.dtype)
    got, = backends.corr_pyramid_forward([buf], coords, 3, slots=_idx(named))
    torch.cuda.synchronize()
    assert _same(got, want) and bool(want.any())
    assert np.array_equal(want.cpu().numpy(), _oracle_lookup(oracle, [small.cpu().numpy()], coords.cpu().numpy(), 3))
    assert _foreign_bytes(buf, named) == 0
    _report(case, tuple(buf.shape), t0)
    del buf


# ---- lookups whose batch index is the slot ----------------------------------------------------------------------------
@pytest.mark.parametrize("dt", DTYPES)
def test_lookup_of_the_whole_buffer_writes_beyond_2_31_elements(backends, big, dt):
    case = lo.BY_ID[f"lookup-batch-{dt}"]
    p, t0 = _pyramid(backends, big, case, case.larges[1].nbytes)
    buf, cap, named = p["buf"], lo.PYR_CAP[dt], list(case.named)
    H, W = lo.PYR_H, lo.PYR_W
    assert cc.volume_path(dt, 3, H * W, H, W, buf[0].data_ptr() % 16, False, "pyramid") == case.path
    small = [torch.stack([b[s] for s in named]) for b in buf]      # one of them a slot of sentinel bytes
    cs = _mix_coords(45, len(named), H, W)
    coords = _tiled_coords(cs, cap, named)
    want, = backends.corr_pyramid_forward(small, cs, 3)
    _poison((cap, 4 * 49, H, W), TDT[dt])
    got, = backends.corr_pyramid_forward(buf, coords, 3)
    torch.cuda.synchronize()
    assert tuple(got.shape) == (cap, 4 * 49, H, W)
    for k, b in enumerate(named):
        assert _same(got[b], want[k]), f"entry {b}"
    for l in range(4):
        assert _foreign_bytes(buf[l], p["named"]) == 0
    _report(case, tuple(buf[0].shape), t0)
    del got


@pytest.mark.parametrize("r", [3, 2])
@pytest.mark.parametrize("dt", DTYPES)
def test_corr_index_forward_on_a_volume_beyond_4_gib(backends, oracle, big, dt, r):
    case = lo.BY_ID[f"index-r{r}-{dt}"]
    p, t0 = _pyramid(backends, big, case, lo.PYR_CAP[dt] * (2 * r + 1) ** 2 * lo.PYR_H * lo.PYR_W * lo.SIZE[dt])
    vol, cap, named = p["buf"][0], lo.PYR_CAP[dt], list(case.named)
    H, W = lo.PYR_H, lo.PYR_W
    assert cc.volume_path(dt, r, H * W, H, W, vol.data_ptr() % 16, False) == case.path
    small = torch.stack([vol[s] for s in named])
    cs = _mix_coords(47 + r, len(named), H, W)
    coords = _tiled_coords(cs, cap, named)
    want, = backends.corr_index_forward(small, cs, r)
    _poison((cap, 2 * r + 1, 2 * r + 1, H, W), TDT[dt])
    got, = backends.corr_index_forward(vol, coords, r)
    torch.cuda.synchronize()
    for k, b in enumerate(named):
        assert _same(got[b], want[k]), f"entry {b}"
    with np.errstate(invalid="ignore", over="ignore"):
        ref = oracle.corr_index_forward(small.cpu().numpy(), cs.cpu().numpy(), r)
    assert np.array_equal(want.cpu().numpy(), ref) and bool(want.any())
    assert _foreign_bytes(vol, p["named"]) == 0
    _report(case, tuple(vol.shape), t0)
    del got


# ---- corr_encode ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("layout", ["2hw", "hw2"])
@pytest.mark.parametrize("dt", DTYPES)
def test_corr_encode_through_slots_beyond_4_gib(backends, big, dt, layout):
    case = lo.BY_ID[f"encode-{layout}-{dt}"]
    p, t0 = _pyramid(backends, big, case)
    buf, small, named = p["buf"], p["small"], p["named"]
    H, W, E = lo.PYR_H, lo.PYR_W, len(named)
    c2 = _mix_coords(53, E, H, W)
    c = c2 if layout == "2hw" else c2.permute(0, 2, 3, 1).contiguous()
    enc = backends.CorrEncoder(*_params(9))
    want = enc(list(small), c, layout=layout)
    _poison((E, cer.N, H, W), torch.float16)
    got = enc(buf, c, slots=_idx(named), layout=layout)
    torch.cuda.synchronize()
    assert _same(got, want)
    # the small call: within tests/corr_encode_ref.bound of relu(s), s in float64 from the device's own lookup bits
    corr, = backends.corr_pyramid_forward(list(small), c2, 3)
    a = corr.half().cpu().numpy()
    wt, b = _params(9, "cpu")
    s, S = cer.sums(a, wt.numpy().reshape(cer.N, cer.KTOT), b.numpy())
    worst, excluded = _worst_ratio(want.cpu().numpy(), a, s, S)
    assert excluded == 0 and worst <= 1.0, (worst, excluded)
    # one selection-weight pass: the output is the bits of relu(+-corr[:, k])
    wsel, sign = _selection(68, 1)
    sel = backends.CorrEncoder(wsel, torch.zeros(cer.N, device=DEV))
    _poison((E, cer.N, H, W), torch.float16)
    got = sel(buf, c, slots=_idx(named), layout=layout)
    torch.cuda.synchronize()
    assert _same(got, _relu(corr.half()[:, 68:68 + cer.N] * sign.half()[None, :, None, None]))
    assert _foreign_bytes(buf[0], named) == 0
    _report(case, tuple(buf[0].shape), t0)


# ---- corr_index_backward ------------------------------------------------------------------------------------------------
def test_corr_index_backward_clears_and_scatters_beyond_4_gib(backends, oracle, big):
    from oracle import corr as oc
    case = lo.BY_ID["backward-f16"]
    cap, named = lo.PYR_CAP["f16"], list(case.named)
    H, W, r = lo.PYR_H, lo.PYR_W, 3
    shape = (cap, H, W, H, W)
    big.drop()
    t0 = _begin(case, 2 * case.larges[0].nbytes + cap * 49 * H * W * 2 + cap * 2 * H * W * 4)
    vol = torch.empty(shape, dtype=torch.float16, device=DEV)     # carries the shape; never read
    cs = _mix_coords(59, len(named), H, W)
    g = torch.Generator().manual_seed(60)
    cgs = torch.randn((len(named), 7, 7, H, W), generator=g).to(torch.float16).to(DEV)
    coords = _tiled_coords(cs, cap, named)
    cg = torch.zeros((cap, 7, 7, H, W), dtype=torch.float16, device=DEV)
    for k, b in enumerate(named):
        cg[b] = cgs[k]
    want, = backends.corr_index_backward(vol[:len(named)].contiguous(), cs, cgs, r)
    _poison(shape, torch.float16)
    got, = backends.corr_index_backward(vol, coords, cg, r)
    torch.cuda.synchronize()
    assert tuple(got.shape) == shape
    for k, b in enumerate(named):
        assert _same(got[b], want[k]), f"entry {b}"
    assert _foreign_bytes(got, named, 0) == 0, "a plane whose gradient is zero holds a non-zero bit"
    with np.errstate(invalid="ignore"):
        ref = oc.corr_index_backward((len(named), H, W, H, W), cs.cpu().numpy(), cgs.cpu().numpy(), r)
    assert np.array_equal(want.cpu().numpy(), ref) and bool(want.any())
    _report(case, shape, t0)
    del got, vol, cg


# ---- alt-corr ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dt", DTYPES)
def test_altcorr_pyramid_writes_beyond_8_gib(backends, oracle, big, dt):
    import torch.nn.functional as F
    case = lo.BY_ID[f"altcorr-{dt}"]
    E, frames, H, W, C, named, r = lo.ALT_E, lo.ALT_FRAMES, lo.ALT_H, lo.ALT_W, lo.ALT_C, list(lo.ALT_NAMED), 3
    big.drop()
    t0 = _begin(case, case.larges[0].nbytes + E * H * W * 2 * 4)
    rng = np.random.default_rng(61)
    x = torch.from_numpy((rng.normal(0, 1, (frames, C, H, W)) / 4).astype(np.float32)).to(DEV).to(TDT[dt])
    pyr = []
    for _ in range(4):
        pyr.append(x.permute(0, 2, 3, 1).contiguous()[None])      # [1, frames, h, w, C], as AltCorrBlock.pyramid
        x = F.avg_pool2d(x.float(), 2, stride=2).to(TDT[dt])
    nset = 16   # coordinate sets: smooth flow, windows over the borders, and a few queries far outside
    yy, xx = np.meshgrid(np.arange(H, dtype=np.float32), np.arange(W, dtype=np.float32), indexing="ij")
    base = np.stack([xx[None] + rng.uniform(-6, 6, (nset, 1, 1)) + rng.uniform(-1.2, 1.2, (nset, H, W)),
                     yy[None] + rng.uniform(-6, 6, (nset, 1, 1)) + rng.uniform(-1.2, 1.2, (nset, H, W))], -1).astype(np.float32)
    base[:, 5, 7] = (-300.0, 1e9)
    base[:, H - 1, W - 1] = (W + 2.5, H + 1.5)
    base = torch.from_numpy(base).to(DEV)
    coords = base[torch.arange(E, device=DEV) % nset].contiguous()
    ii = torch.from_numpy(rng.integers(0, frames, E)).to(DEV)
    jj = torch.from_numpy(rng.integers(0, frames, E)).to(DEV)
    assert len({e % nset for e in named}) == len(named)
    sel = _idx(named)
    want, = backends.altcorr_pyramid_forward(pyr, coords[sel].contiguous(), ii[sel], jj[sel], r)
    _poison((E, 4 * 49, H, W), torch.float32)
    got, = backends.altcorr_pyramid_forward(pyr, coords, ii, jj, r)
    torch.cuda.synchronize()
    assert tuple(got.shape) == (E, 4 * 49, H, W) and got.dtype == torch.float32
    for k, e in enumerate(named):
        assert _same(got[e], want[k]), f"edge {e}"
    assert not _same(want[1], want[2])
    # the small call against the fp64 oracle on the same values, at the bar of test_gpu_baseline_shapes.py
    w = want.cpu().numpy()
    for l in range(4):
        f1 = pyr[0][0][ii[sel]].float().cpu().numpy()
        f2 = pyr[l][0][jj[sel]].float().cpu().numpy()
        cl = (coords[sel] / 2 ** l).reshape(len(named), 1, H, W, 2).cpu().numpy()
        ref = oracle.altcorr_forward(f1, f2, cl, r, acc_dtype=np.float64)[:, 0]
        err = np.abs(w[:, l * 49:(l + 1) * 49] - ref).max() / np.abs(ref).max()
        assert err < 1e-5, (l, err)
    _report(case, (E, 4 * 49, H, W), t0)
    del got


# ---- graph_mean / scatter_mean ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("op", ["graph_mean", "scatter_mean"])
@pytest.mark.parametrize("dt", DTYPES)
def test_source_frame_mean_of_rows_beyond_4_gib(backends, big, dt, op):
    case = lo.BY_ID[f"{op}-{dt}"]
    E, rows_, M = lo.GM_E[dt], list(lo.GM_ROWS[dt]), lo.GM_GROUPS
    groups = [lo.gm_group(k) for k in range(len(rows_))]
    big.drop()
    t0 = _begin(case, case.larges[0].nbytes)
    src = torch.empty((E, 128, 24, 32), dtype=TDT[dt], device=DEV)
    _fill(src)
    x = np.random.default_rng(71).normal(0.0, 4.0, (len(rows_), lo.GM_PLANE)).astype(NDT[dt])
    xs = torch.from_numpy(x).to(DEV).view(len(rows_), 128, 24, 32)
    for k, e in enumerate(rows_):
        src[e].copy_(xs[k])
    index = torch.full((E,), -1, dtype=torch.int64, device=DEV)
    index[_idx(rows_)] = _idx(groups)
    if op == "graph_mean":
        run = lambda s, i: backends.graph_mean(s, i, num_groups=M, nbuf=M)
    else:
        run = lambda s, i: backends.scatter_mean(s, i, dim=0, dim_size=M)
    want = run(xs, _idx(groups))
    _poison((M, 128, 24, 32), TDT[dt])
    got = run(src, index)
    torch.cuda.synchronize()
    assert tuple(got.shape) == (M, 128, 24, 32) and _same(got, want)
    ref = gmr.ref(x, np.array(groups, np.int64), M, M, int(op == "graph_mean"))
    assert gmr.same_bits(want.cpu().numpy().reshape(M, -1), ref) and bool(ref.any())
    assert _foreign_bytes(src, rows_) == 0
    _report(case, tuple(src.shape), t0)
    del src


# ---- convex upsampling --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dt", DTYPES)
def test_upsample_with_a_mask_beyond_4_gib(backends, big, dt):
    case = lo.BY_ID[f"upsample-{dt}"]
    n, named, frames, H, W, nbuf = lo.UP_N[dt], list(lo.UP_NAMED[dt]), list(lo.UP_FRAMES), lo.UP_H, lo.UP_W, lo.UP_BUFFER
    big.drop()
    t0 = _begin(case, case.larges[0].nbytes)
    mask = torch.empty((n, 576, H, W), dtype=TDT[dt], device=DEV)
    _fill(mask)
    rng = np.random.default_rng(81)
    m16 = rng.normal(0.0, 4.0, (len(named), 576, H, W)).astype(np.float16)
    ms = torch.from_numpy(m16).to(DEV).to(TDT[dt])
    for k, e in enumerate(named):
        mask[e].copy_(ms[k])
    data = rng.uniform(0.001, 10.0, (nbuf, H, W)).astype(np.float32)
    disps = torch.from_numpy(data).to(DEV)
    ix = torch.full((n,), -1, dtype=torch.int64, device=DEV)
    ix[_idx(named)] = _idx(frames)
    out = [torch.empty((nbuf, 8 * H, 8 * W), dtype=torch.float32, device=DEV) for _ in range(2)]
    for o in out:
        _fill(o)
    assert backends.upsample_disps(disps, _idx(frames), ms, out[0]) is out[0]
    assert backends.upsample_disps(disps, ix, mask, out[1]) is out[1]
    torch.cuda.synchronize()
    assert _same(out[1], out[0])
    rest = sorted(set(range(nbuf)) - set(frames))
    assert len(rest) == 4 and _foreign_bytes(out[1], frames) == 0
    got = out[0][_idx(frames)].cpu().numpy()
    e = cur.err_nb(got, cur.ref(data[frames], m16, np.float64), cur.nb(data[frames]))
    assert e <= cur.BAR, e / cur.U
    assert _foreign_bytes(mask, named) == 0
    _report(case, tuple(mask.shape), t0)
    del mask
