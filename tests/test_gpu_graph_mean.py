"""The source-frame mean on the device (droid_graph_mean through droid_backends.graph_mean / scatter_mean and through
the C entry point) against the numpy restatement of its contract (tests/graph_mean_ref.py), bit for bit: every plane size
around the 16-byte chunk and the workgroup tile, group sizes around the load-unroll depth, misaligned views (the
element-wise path), ignored index values, M above and below the distinct count, the value cases, sentinel guards,
determinism, independence of a group from everything that is not its own entries, the call GraphAgg.forward would make
on a side stream, and the distance from the stock index_add_ chain a user sees when switching."""
import numpy as np
import pytest
import torch

import graph_mean_ref as gr

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
TORCH = {np.float16: torch.float16, np.float32: torch.float32}
CODE = {np.float16: 0, np.float32: 1}                                   # DROID_F16, DROID_F32
INT = {np.float16: torch.int16, np.float32: torch.int32}
SENTINEL = {np.float16: 0x7DAD, np.float32: 0x7FC0DEAD}                 # NaN bit patterns no mean of these inputs produces
SHAPES = [(d, p) for d in gr.DTYPES for p in gr.PLANES[d]]


def _dev(a):
    return torch.from_numpy(np.array(a)).to(DEV)   # a copy: the shared problems are read-only


def _sentinel(n, dtype):
    return torch.full((n,), SENTINEL[dtype], dtype=INT[dtype], device=DEV).view(TORCH[dtype])


def _is_sentinel(t, dtype):
    return bool((t.contiguous().view(INT[dtype]) == SENTINEL[dtype]).all())


def _call(backends, src, index, out, M, rng, compact, dtype, groups=None, ws=None):
    """The C entry point on the current stream; src [E, plane], out [>= M, plane] (views allowed)."""
    lib = backends._lib.load()
    E, plane = int(src.shape[0]), int(src.shape[1])
    if ws is None:
        ws = torch.empty(max(int(lib.droid_graph_mean_workspace_bytes(E, rng)), 4), dtype=torch.uint8, device=DEV)
    rc = lib.droid_graph_mean(src.data_ptr(), index.data_ptr(), out.data_ptr(), E, plane, M, rng, compact, CODE[dtype],
                              None if groups is None else groups.data_ptr(), ws.data_ptr(), ws.numel(),
                              torch.cuda.current_stream().cuda_stream)
    assert rc == 0, lib.droid_last_error()
    return out


def _run(backends, x, index, M, rng, compact):
    """[M, plane] numpy through the C entry point, on a fresh output."""
    dtype = x.dtype.type
    out = _sentinel(M * x.shape[1], dtype).view(M, x.shape[1])
    _call(backends, _dev(x), _dev(index), out, M, rng, compact, dtype)
    return out.cpu().numpy()


@pytest.mark.parametrize("dtype,plane", SHAPES)
def test_every_plane_size_bit_for_bit(backends, dtype, plane):
    """Both modes through the Python entry points; the index holds -1, RANGE and 2**40, which belong to no group."""
    x, index = gr.shape_problem(dtype, plane)
    xd, idx = _dev(x), _dev(index)
    M = len(gr.FRAMES)
    got = backends.graph_mean(xd.view(-1, plane, 1, 1), idx, num_groups=M, nbuf=gr.RANGE)
    assert got.shape == (M, plane, 1, 1) and got.dtype == TORCH[dtype]
    assert gr.same_bits(got.view(M, plane).cpu().numpy(), gr.ref(x, index, M, gr.RANGE, 1))
    got = backends.scatter_mean(xd, idx, dim=0, dim_size=gr.RANGE)
    want = gr.ref(x, index, gr.RANGE, gr.RANGE, 0)
    assert gr.same_bits(got.cpu().numpy(), want)
    empty = [r for r in range(gr.RANGE) if r not in gr.FRAMES]
    assert not got[empty].view(INT[dtype]).any()                         # +0.0 bit for bit, not -0.0
    got = backends.scatter_mean(xd[None], idx, dim_size=gr.RANGE)           # the call shape GraphAgg uses: dim = 1
    assert got.shape == (1, gr.RANGE, plane) and gr.same_bits(got[0].cpu().numpy(), want)
    worst, ok = gr.within_bound(want, x, index, gr.RANGE, gr.RANGE, 0)
    assert ok, worst


@pytest.mark.parametrize("dtype", gr.DTYPES)
def test_a_single_entry(backends, dtype):
    x = np.random.default_rng(1).normal(0.0, 4.0, (1, 37)).astype(dtype)
    for frame, live in ((2, True), (5, False), (-1, False)):
        index = np.array([frame], np.int64)
        assert gr.same_bits(_run(backends, x, index, 1, 5, 1), x if live else np.zeros_like(x))   # mean of one = itself
        assert gr.same_bits(_run(backends, x, index, 5, 5, 0), gr.ref(x, index, 5, 5, 0))
    got = backends.graph_mean(_dev(x).view(1, 1, 37, 1, 1), _dev(np.array([7], np.int64)))   # unique + max read here
    assert got.shape == (1, 1, 37, 1, 1) and gr.same_bits(got.view(1, 37).cpu().numpy(), x)


@pytest.mark.parametrize("dtype", gr.DTYPES)
@pytest.mark.parametrize("plane", [9, 6144])
@pytest.mark.parametrize("shift", [1, 16])   # elements of offset: 2 or 4 bytes (element-wise path), 16 elements (aligned)
def test_views_into_a_larger_buffer_between_guards(backends, dtype, plane, shift):
    """src and out start `shift` elements into larger buffers: the element-wise path where that breaks the 16-byte
    alignment gives the bits of the vector path, and nothing outside out is written."""
    x, index = gr.shape_problem(dtype, plane)
    E, M, guard = x.shape[0], len(gr.FRAMES), 1024 + shift
    big_in = _sentinel(2 * guard + E * plane, dtype)
    src = big_in[guard:guard + E * plane].view(E, plane)
    src.copy_(_dev(x))
    big_out = _sentinel(2 * guard + M * plane, dtype)
    out = big_out[guard:guard + M * plane].view(M, plane)
    assert src.data_ptr() % 16 == (shift * x.itemsize) % 16
    idx = _dev(index)
    groups = torch.full((1,), -7, dtype=torch.int32, device=DEV)
    _call(backends, src, idx, out, M, gr.RANGE, 1, dtype, groups)
    torch.cuda.synchronize()
    assert gr.same_bits(out.cpu().numpy(), gr.ref(x, index, M, gr.RANGE, 1))
    assert int(groups) == M
    for big in (big_in, big_out):
        assert _is_sentinel(big[:guard], dtype) and _is_sentinel(big[-guard:], dtype)
    assert np.array_equal(src.cpu().numpy().view(np.uint8), x.view(np.uint8))          # src and index are only read
    assert np.array_equal(idx.cpu().numpy(), index)


@pytest.mark.parametrize("dtype", gr.DTYPES)
def test_rows_above_and_below_the_distinct_count(backends, dtype):
    plane = 9
    x, index = gr.shape_problem(dtype, plane)
    xd, idx = _dev(x), _dev(index)
    D = len(gr.FRAMES)
    full = gr.ref(x, index, D, gr.RANGE, 1)
    groups = torch.zeros(1, dtype=torch.int32, device=DEV)
    # M above the distinct count, above RANGE and above one launch's 65535 rows: the rest is +0.0
    for M in (D + 3, gr.RANGE + 2, 70000):
        out = _sentinel(M * plane, dtype).view(M, plane)
        groups.fill_(-1)
        _call(backends, xd, idx, out, M, gr.RANGE, 1, dtype, groups)
        assert gr.same_bits(out[:D].cpu().numpy(), full)
        assert not out[D:].view(INT[dtype]).any()
        assert int(groups) == D
    # M below: the groups from M onward are not written
    M = D - 3
    out = _sentinel(D * plane, dtype).view(D, plane)
    groups.fill_(-1)
    _call(backends, xd, idx, out, M, gr.RANGE, 1, dtype, groups)
    assert gr.same_bits(out[:M].cpu().numpy(), full[:M]) and _is_sentinel(out[M:], dtype)
    assert int(groups) == D                                               # the true count: the caller can check its M
    # dense mode: entries >= M are ignored, the count is the rows that have an entry
    M = 10
    out = _sentinel((M + 2) * plane, dtype).view(M + 2, plane)
    groups.fill_(-1)
    _call(backends, xd, idx, out, M, M, 0, dtype, groups)
    assert gr.same_bits(out[:M].cpu().numpy(), gr.ref(x, index, M, M, 0)) and _is_sentinel(out[M:], dtype)
    assert int(groups) == sum(f < M for f in gr.FRAMES)


@pytest.mark.parametrize("E", [8191, 8192, 8193, 9000])
def test_entry_counts_around_the_prepare_step_s_two_list_builders(backends, E):
    """Up to 8192 entries the lists are sorted in LDS, beyond a thread per frame walks the index: the same lists."""
    rng = np.random.default_rng(E)
    frames = rng.choice(512, 300, replace=False)
    index = np.concatenate([frames[rng.integers(0, 300, E - 40)], rng.choice([-1, 512, 2 ** 40, -2 ** 40], 40)])
    index = index[rng.permutation(E)].astype(np.int64)
    x = rng.normal(0.0, 4.0, (E, 8)).astype(np.float16)
    D = len(np.unique(index[(index >= 0) & (index < 512)]))
    groups = torch.zeros(1, dtype=torch.int32, device=DEV)
    out = _sentinel(D * 8, np.float16).view(D, 8)
    _call(backends, _dev(x), _dev(index), out, D, 512, 1, np.float16, groups)
    assert gr.same_bits(out.cpu().numpy(), gr.ref(x, index, D, 512, 1)) and int(groups) == D
    assert gr.same_bits(_run(backends, x, index, 512, 512, 0), gr.ref(x, index, 512, 512, 0))


@pytest.mark.parametrize("dtype", gr.DTYPES)
def test_no_entries_zero_fills(backends, dtype):
    lib = backends._lib.load()
    out = _sentinel(3 * 11, dtype).view(3, 11)
    groups = torch.full((1,), 5, dtype=torch.int32, device=DEV)
    rc = lib.droid_graph_mean(None, None, out.data_ptr(), 0, 11, 3, 8, 1, CODE[dtype], groups.data_ptr(), None, 0,
                              torch.cuda.current_stream().cuda_stream)
    assert rc == 0
    assert not out.view(INT[dtype]).any() and int(groups) == 0
    empty = torch.zeros((0, 4, 2, 2), dtype=TORCH[dtype], device=DEV)
    none = torch.zeros(0, dtype=torch.int64, device=DEV)
    assert backends.graph_mean(empty, none).shape == (0, 4, 2, 2)
    got = backends.scatter_mean(empty, none, dim=0, dim_size=3)
    assert got.shape == (3, 4, 2, 2) and not got.view(INT[dtype]).any()


@pytest.mark.parametrize("dtype", gr.DTYPES)
def test_value_cases(backends, dtype):
    """Half subnormals, three times 65504, cancelling signs, one NaN, one inf, a lone -0.0: IEEE, nothing sanitised."""
    x, index, where = gr.value_problem(dtype)
    D = len(gr.V_FRAMES)
    got = _run(backends, x, index, D, gr.V_RANGE, 1)
    assert gr.same_bits(got, gr.ref(x, index, D, gr.V_RANGE, 1))
    dense = _run(backends, x, index, gr.V_RANGE, gr.V_RANGE, 0)
    assert gr.same_bits(dense, gr.ref(x, index, gr.V_RANGE, gr.V_RANGE, 0))
    for name, frame in gr.V_FRAMES.items():
        assert gr.same_bits(dense[frame], got[gr.compact_row(name)])
    row = {name: got[gr.compact_row(name)] for name in gr.V_FRAMES}
    assert (row["max3"] == 65504.0).all() and (row["big2"] == 40000.0).all()
    assert (row["negzero"] == 0).all() and np.signbit(row["negzero"]).all()
    assert np.isnan(got).sum() == 1 and np.isnan(row["nan"][3])            # exactly their own group's element
    assert np.isinf(got).sum() == 1 and np.isposinf(row["inf"][3])
    if dtype is np.float16:
        assert (row["subnormal"] != 0).any() and (np.abs(row["subnormal"].astype(np.float64)) < 2.0 ** -14).all()


def test_one_workspace_serves_two_graphs(backends):
    lib = backends._lib.load()
    xa, ia = gr.shape_problem(np.float16, 2049)
    xb, ib, _ = gr.value_problem(np.float32)
    ws = torch.empty(int(max(lib.droid_graph_mean_workspace_bytes(len(ia), gr.RANGE),
                             lib.droid_graph_mean_workspace_bytes(len(ib), gr.V_RANGE))), dtype=torch.uint8, device=DEV)
    wa, wb = gr.ref(xa, ia, gr.RANGE, gr.RANGE, 0), gr.ref(xb, ib, len(gr.V_FRAMES), gr.V_RANGE, 1)
    a, b = (_dev(xa), _dev(ia)), (_dev(xb), _dev(ib))
    for _ in range(2):                                                     # a, b, a, b back to back on one stream
        oa = _call(backends, *a, torch.empty((gr.RANGE, 2049), dtype=torch.float16, device=DEV), gr.RANGE, gr.RANGE, 0,
                   np.float16, ws=ws)
        ob = _call(backends, *b, torch.empty((len(gr.V_FRAMES), gr.VPLANE), device=DEV), len(gr.V_FRAMES), gr.V_RANGE, 1,
                   np.float32, ws=ws)
        assert gr.same_bits(oa.cpu().numpy(), wa) and gr.same_bits(ob.cpu().numpy(), wb)


@pytest.mark.parametrize("dtype", gr.DTYPES)
def test_deterministic_and_independent_of_everything_foreign(backends, dtype):
    plane = 2049
    x, index = gr.shape_problem(dtype, plane)
    D = len(gr.FRAMES)
    a = _run(backends, x, index, D, gr.RANGE, 1)
    assert gr.same_bits(a, _run(backends, x, index, D, gr.RANGE, 1))       # two runs, the same bits
    for g, frame in enumerate(gr.FRAMES):
        own = np.flatnonzero(index == frame)
        alone = _run(backends, x[own], index[own], 1, gr.RANGE, 1)         # alone: another E, no other group
        assert gr.same_bits(alone[0], a[g]), frame
    # one group's entries among foreign ones at other places: only the order of its own entries matters
    frame, g = gr.FRAMES[3], 3
    own = np.flatnonzero(index == frame)
    rng = np.random.default_rng(3)
    foreign = rng.normal(0.0, 100.0, (200, plane)).astype(dtype)
    slots = np.sort(rng.choice(200 + len(own), len(own), replace=False))   # where the own entries go, order kept
    x2 = np.empty((200 + len(own), plane), dtype)
    i2 = np.empty(200 + len(own), np.int64)
    mask = np.zeros(200 + len(own), bool)
    mask[slots] = True
    x2[mask], i2[mask] = x[own], frame
    x2[~mask], i2[~mask] = foreign, rng.choice([1, 2, 5, 38, -4, 77], 200)
    got = _run(backends, x2, i2, gr.RANGE, gr.RANGE, 0)
    assert gr.same_bits(got[frame], a[g])


def test_caller_replay_on_a_side_stream(backends):
    """droid_net.py:63-67 with the body replaced: relu(conv1(net)) under autocast, then the mean over each source."""
    E, C, H, W = 9, 128, 6, 8
    torch.manual_seed(4)
    conv1 = torch.nn.Conv2d(C, C, 3, padding=1).to(DEV)
    x = torch.randn((E, C, H, W), device=DEV)
    ii = _dev(np.array([3, 3, 5, 9, 9, 9, 12, 5, 3], np.int64))            # sources repeat
    torch.cuda.synchronize()
    # a high-priority stream: PyTorch and the runtime keep those apart from the default-priority ones, so the streams
    # (and hardware queues) the tests after this one draw are the ones they drew before this test existed
    side = torch.cuda.Stream(priority=-1)
    with torch.cuda.stream(side), torch.no_grad():
        with torch.autocast("cuda", dtype=torch.float16):
            net = torch.relu(conv1(x))
        assert net.dtype == torch.float16
        net = net.view(1, E, C, H, W)
        _, ix = torch.unique(ii, return_inverse=True)
        fused = backends.graph_mean(net, ii)
        total = fused.double().sum()                                       # a following op on the stream sees it complete
        dense = backends.scatter_mean(net, ix, dim=1)
        known = backends.graph_mean(net, ii, num_groups=4, nbuf=16)        # no host read on this path
    side.synchronize()
    net_np, ii_np = net[0].cpu().numpy().reshape(E, -1), ii.cpu().numpy()
    want = gr.ref(net_np, ii_np, 4, 16, 1)
    assert fused.shape == (1, 4, C, H, W) and dense.shape == fused.shape and known.shape == fused.shape
    for got in (fused, dense, known):
        assert gr.same_bits(got.cpu().numpy().reshape(4, -1), want)
    assert np.isclose(float(total), want.astype(np.float64).sum(), rtol=1e-10, atol=0.0)
    assert (want != 0).any()


@pytest.mark.parametrize("dtype,plane", [(d, p) for d in gr.DTYPES for p in (9, 6144)])
def test_distance_from_the_stock_chain(backends, dtype, plane):
    """What a user sees when switching from zeros + index_add_ / bincount.  In fp32 both sides are within the bound of
    the fp64 mean, so they are within twice the bound of each other; in half the stock chain keeps half partial sums and
    is the less accurate side: printed only, the correctness bar is the restatement."""
    x, index = gr.shape_problem(dtype, plane)
    keep = (index >= 0) & (index < gr.RANGE)                               # the stock chain has no notion of ignored entries
    x, index = x[keep], index[keep]
    xd, idx = _dev(x), _dev(index)
    uniq, ix = torch.unique(idx, return_inverse=True)
    M = int(uniq.numel())
    stock = torch.zeros((M, plane), dtype=TORCH[dtype], device=DEV).index_add_(0, ix, xd)
    stock = (stock / torch.bincount(ix, minlength=M).view(-1, 1).to(TORCH[dtype])).cpu().numpy().astype(np.float64)
    got = backends.graph_mean(xd.view(-1, plane, 1, 1), idx).view(M, plane).cpu().numpy().astype(np.float64)
    mean, absmean, n = gr.mean64(x, index, M, gr.RANGE, 1)
    b = gr.bound(mean, absmean, n, dtype)
    d = float((np.abs(got - stock) / b).max())
    print(f"{np.dtype(dtype).name} plane {plane}: {d:.3f} x the bound from the stock chain "
          f"(stock {float((np.abs(stock - mean) / b).max()):.3f}, fused {float((np.abs(got - mean) / b).max()):.3f} from fp64)")
    if dtype is np.float32:
        assert d <= 2.0, d
