"""CPU checks of the convex-upsampling reference side (tests/cvx_upsample_ref.py): the error bar the device test holds
the kernel to is reachable in fp32, the stock torch sequence sits where DESIGN.md says it does, and one-hot masks pin
the (k, a, b) channel order and the zero padding without a tolerance."""
import numpy as np
import pytest
import torch

import cvx_upsample_ref as cr

TABLE = [(c, s) for c in range(len(cr.CASES)) for s in cr.SIGMAS]


@pytest.mark.parametrize("case,sigma", TABLE)
def test_fp32_restatement_reaches_the_bar(case, sigma):
    p = cr.problem(case, sigma)
    got = cr.ref(p["data"], p["mask16"], np.float32)
    assert got.dtype == np.float32
    e = cr.err_nb(got, p["ref64"], p["nb"])
    print(f"{cr.CASES[case]} sigma {sigma}: fp32 restatement {e / cr.U:.2f} u nb")
    assert e <= cr.BAR, (cr.CASES[case], sigma, e / cr.U)


@pytest.mark.parametrize("case,sigma", TABLE)
def test_stock_chain_fp32_masks(case, sigma):
    p = cr.problem(case, sigma)
    got = cr.stock(torch.from_numpy(p["data"].copy()), torch.from_numpy(p["mask32"].copy())).numpy()
    e = cr.err_nb(got, p["ref64"], p["nb"])
    print(f"{cr.CASES[case]} sigma {sigma}: stock fp32 {e / cr.U:.2f} u nb")
    assert e <= cr.BAR, (cr.CASES[case], sigma, e / cr.U)


@pytest.mark.parametrize("case,sigma", TABLE)
def test_stock_chain_half_masks_round_their_weights(case, sigma):
    p = cr.problem(case, sigma)
    got = cr.stock(torch.from_numpy(p["data"].copy()), torch.from_numpy(p["mask16"].copy()))
    assert got.dtype == torch.float32
    e = cr.err_nb(got.numpy(), p["ref64"], p["nb"])
    print(f"{cr.CASES[case]} sigma {sigma}: stock half {e * 2 ** 12:.2f} x 2^-12 nb")
    assert e <= cr.STOCK_F16_CPU_BAR, (cr.CASES[case], sigma, e * 2 ** 12)


def test_stock_indexed_form_writes_only_the_named_frames():
    p = cr.problem(0, 4.0)
    n, H, W = cr.CASES[0]
    disps = torch.zeros((n + 2, H, W))
    ix = torch.tensor([4, 0, 2])
    disps[ix] = torch.from_numpy(p["data"].copy())
    out = torch.full((n + 2, 8 * H, 8 * W), -7.0)
    cr.stock(disps, torch.from_numpy(p["mask32"].copy()), ix, out)
    assert cr.err_nb(out[ix].numpy(), p["ref64"], p["nb"]) <= cr.BAR
    assert bool((out[[1, 3]] == -7.0).all())


@pytest.mark.parametrize("case", range(len(cr.CASES)))
def test_one_hot_masks_select_exactly(case):
    data, mask16, want = cr.onehot(case)
    n, H, W = cr.CASES[case]
    m = mask16.reshape(n, 9, 64, H, W).astype(np.float32)
    assert ((m == 60000.0).sum(axis=1) == 1).all() and ((m == -60000.0).sum(axis=1) == 8).all()
    assert {int(k) for k in np.unique(m.argmax(axis=1))} == set(range(9))      # the selected tap cycles over all 9
    for dt in (np.float64, np.float32):
        assert cr.same_bits(cr.ref(data, mask16, dt).astype(np.float32), want), (cr.CASES[case], dt)
    assert not np.signbit(want).any()
    if H == 1:                                   # every tap but the centre row is padding: two thirds select a zero
        assert (want == 0).mean() > 0.6
    got = cr.stock(torch.from_numpy(data.copy()), torch.from_numpy(mask16.astype(np.float32))).numpy()
    assert cr.same_bits(got, want), cr.CASES[case]
