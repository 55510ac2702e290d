"""The numpy restatement of droid_graph_mean (tests/graph_mean_ref.py) checked against independent evaluations, so that
the GPU tests compare bit for bit against something that is itself right: within the derived bound of the fp64 means on
every case, compact mode = torch.unique(return_inverse) + dense mode, dense mode = a per-group torch mean, and the half
running sums of the stock chain fail where the cases were built to make them fail while the restatement does not."""
import numpy as np
import pytest
import torch

import graph_mean_ref as gr

SHAPES = [(d, p) for d in gr.DTYPES for p in gr.PLANES[d]]


@pytest.mark.parametrize("dtype,plane", SHAPES)
def test_restatement_within_the_bound_on_every_shape(dtype, plane):
    x, index = gr.shape_problem(dtype, plane)
    for compact, M in ((1, len(gr.FRAMES)), (0, gr.RANGE)):
        got = gr.ref(x, index, M, gr.RANGE, compact)
        worst, ok = gr.within_bound(got, x, index, M, gr.RANGE, compact)
        print(f"{np.dtype(dtype).name} plane {plane} compact {compact}: {worst:.3f} of the bound")
        assert ok, (dtype, plane, compact, worst)


@pytest.mark.parametrize("dtype", gr.DTYPES)
def test_restatement_on_the_value_cases(dtype):
    x, index, where = gr.value_problem(dtype)
    M = len(gr.V_FRAMES)
    got = gr.ref(x, index, M, gr.V_RANGE, 1)
    worst, ok = gr.within_bound(got, x, index, M, gr.V_RANGE, 1)
    assert ok, worst
    row = {name: got[gr.compact_row(name)] for name in gr.V_FRAMES}
    assert (row["max3"] == 65504.0).all()                                   # not inf: the sum is fp32
    assert (row["negzero"] == 0).all() and np.signbit(row["negzero"]).all()
    assert (row["big2"] == 40000.0).all()
    b = x[where["cancel"][2]].astype(np.float32)
    assert gr.same_bits(row["cancel"], (b / np.float32(3)).astype(dtype))    # +a - a is exactly 0: only b / 3 is left
    assert np.isnan(row["nan"][3]) and np.isfinite(np.delete(row["nan"], 3)).all()
    assert np.isposinf(row["inf"][3]) and np.isfinite(np.delete(row["inf"], 3)).all()
    others = [n for n in gr.V_FRAMES if n not in ("nan", "inf")]
    assert all(np.isfinite(row[n]).all() for n in others)                    # NaN / inf stay in their own group
    if dtype is np.float16:
        assert (np.abs(row["subnormal"].astype(np.float64)) < 2.0 ** -14).all() and (row["subnormal"] != 0).any()


@pytest.mark.parametrize("dtype", gr.DTYPES)
def test_compact_is_unique_inverse_plus_dense(dtype):
    x, index = gr.shape_problem(dtype, 9)
    keep = (index >= 0) & (index < gr.RANGE)                 # torch.unique would rank the ignored values too
    xi, ii = x[keep], index[keep]
    uniq, inv = torch.unique(torch.from_numpy(ii.copy()), return_inverse=True)
    M = int(uniq.numel())
    assert M == len(gr.FRAMES)
    dense = gr.ref(xi, inv.numpy(), M, M, 0)
    assert gr.same_bits(gr.ref(x, index, M, gr.RANGE, 1), dense)             # the ignored entries change nothing
    assert gr.same_bits(gr.ref(xi, ii, M, gr.RANGE, 1), dense)
    more = gr.ref(x, index, M + 3, gr.RANGE, 1)                              # rows beyond the distinct count: +0.0
    assert gr.same_bits(more[:M], dense) and gr.same_bits(more[M:], np.zeros_like(more[M:]))
    assert gr.same_bits(gr.ref(x, index, M - 2, gr.RANGE, 1), dense[:M - 2])
    assert gr.lists(index, M, gr.RANGE, 1)[1] == M


@pytest.mark.parametrize("dtype", gr.DTYPES)
def test_dense_is_a_per_group_mean(dtype):
    x, index = gr.shape_problem(dtype, 9)
    got = gr.ref(x, index, gr.RANGE, gr.RANGE, 0)
    xt, it = torch.from_numpy(x.copy()), torch.from_numpy(index.copy())
    mean, absmean, n = gr.mean64(x, index, gr.RANGE, gr.RANGE, 0)
    b = gr.bound(mean, absmean, n, dtype)
    for r in range(gr.RANGE):
        sel = xt[it == r]
        if sel.shape[0] == 0:
            assert gr.same_bits(got[r], np.zeros_like(got[r]))              # +0.0, not -0.0
            continue
        want = sel.float().mean(0).double().numpy()                          # torch's own fp32 mean: within the bound too
        assert (np.abs(got[r].astype(np.float64) - want) <= 2 * b[r]).all(), r
    assert gr.lists(index, gr.RANGE, gr.RANGE, 0)[1] == len(gr.FRAMES)


def test_half_running_sums_fail_where_the_restatement_does_not():
    x, index, where = gr.value_problem(np.float16)
    M = gr.V_RANGE
    xt, it = torch.from_numpy(x.copy()), torch.from_numpy(index.copy())
    stock = torch.zeros((M, gr.VPLANE), dtype=torch.float16).index_add_(0, it, xt)
    stock = (stock / torch.bincount(it, minlength=M).clamp(min=1).view(-1, 1).half()).numpy()
    got = gr.ref(x, index, M, M, 0)
    mean, absmean, n = gr.mean64(x, index, M, M, 0)
    b = gr.bound(mean, absmean, n, np.float16)
    seq = gr.half_chain(x, index, M)
    for chain in (stock, seq):                              # overflow does not depend on the order of the additions
        assert np.isinf(chain[gr.V_FRAMES["big2"]]).all() and np.isinf(chain[gr.V_FRAMES["max3"]]).all()
    r = gr.V_FRAMES["long60"]                               # ascending e: the sum stays at 2048 and drops 59 entries
    lost = (np.abs(seq[r].astype(np.float64) - mean[r]) / b[r]).min()
    print(f"half running sum over 60 entries: at least {lost:.1f} x the bound at every element")
    assert lost > 1.0   # outside what a correct fp32 evaluation meets; the restatement (below) is inside
    for name in ("big2", "max3", "long60"):
        r = gr.V_FRAMES[name]
        assert (np.abs(got[r].astype(np.float64) - mean[r]) <= b[r]).all(), name
