"""The numpy restatement of droid_ba_inputs (tests/ba_inputs_ref.py) against the stock tail of `FactorGraph.update`
written independently with torch operators on the CPU (`+`, `unique`, boolean indexing, `cat`, `permute().contiguous()`),
bit for bit on every case of the table, eta included.  The torch chain is the yardstick.  Two things the stock tail
cannot express are stated here as the contract states them: a source outside the damping buffer is left out of `unique`
(the stock indexing would raise, or wrap -1 to the last frame), and with another number of damping rows than sources the
rows below the smaller of the two are assigned (the stock assignment would raise)."""
import numpy as np
import pytest
import torch

import ba_inputs_ref as br


def stock_tail(c):
    ii, jj = torch.from_numpy(c.ii), torch.from_numpy(c.jj)
    coords1 = torch.from_numpy(c.a)[None]
    damping_buf = torch.from_numpy(c.damping_buf).clone()
    nbuf = damping_buf.shape[0]
    ht, wd = coords1.shape[2:4]
    t0 = c.t0 if c.t0 >= 0 else max(1, ii.min().item() + 1)

    def unique(x):
        u = torch.unique(x)
        return u[(u >= 0) & (u < nbuf)]

    if c.delta is not None:
        target = coords1 + torch.from_numpy(c.delta)[None].to(dtype=torch.float)
        weight = torch.from_numpy(c.w)[None].to(dtype=torch.float)
    else:
        target, weight = coords1, torch.from_numpy(c.w)[None]
    state = (target, weight)
    if c.damping_net is not None:
        damping = torch.from_numpy(c.damping_net)
        ix = unique(ii)
        n = min(len(ix), len(damping))
        damping_buf[ix[:n]] = damping[:n].float()
    ii_inac, jj_inac = torch.from_numpy(c.ii_inac), torch.from_numpy(c.jj_inac)
    m = (ii_inac >= t0 - 3) & (jj_inac >= t0 - 3)
    ii = torch.cat([ii_inac[m], ii], 0)
    jj = torch.cat([jj_inac[m], jj], 0)
    target = torch.cat([torch.from_numpy(c.target_inac)[None][:, m], target], 1)
    weight = torch.cat([torch.from_numpy(c.weight_inac)[None][:, m], weight], 1)
    eta = .2 * damping_buf[unique(ii)].contiguous() + c.ep
    target = target.view(-1, ht, wd, 2).permute(0, 3, 1, 2).contiguous()
    weight = weight.view(-1, ht, wd, 2).permute(0, 3, 1, 2).contiguous()
    t1 = max(ii.max().item(), jj.max().item()) + 1
    return dict(t0=t0, t1=t1, ii_ba=ii, jj_ba=jj, target_ba=target, weight_ba=weight, eta=eta, damping_buf=damping_buf,
                target_state=state[0][0], weight_state=state[1][0], K=int(m.sum()))


@pytest.mark.parametrize("case", br.CASES, ids=repr)
def test_restatement_equals_the_stock_tail(case):
    ref, want = br.reference(case), stock_tail(case)
    for key in ("ii_ba", "jj_ba", "target_ba", "weight_ba", "eta", "damping_buf"):
        assert br.same_bits(ref[key], want[key].numpy()), key
    if case.delta is not None:
        for key in ("target_state", "weight_state"):
            assert br.same_bits(ref[key], want[key].numpy()), key
    else:
        assert ref["target_state"] is None and ref["weight_state"] is None
    assert ref["K"] == want["K"] and ref["Eb"] == want["K"] + len(case.ii) == len(ref["ii_ba"])
    assert ref["t0"] == min(want["t0"], br.INT_MAX) and ref["t1"] == min(want["t1"], br.INT_MAX)
    assert ref["M"] == len(ref["eta"]) == len(ref["frames_eta"]) and ref["G"] == len(ref["frames_active"])
    inside = lambda x: x[(x >= 0) & (x < case.nbuf)]   # noqa: E731
    assert np.array_equal(ref["frames_active"], inside(np.unique(case.ii)))
    assert np.array_equal(ref["frames_eta"], inside(np.unique(ref["ii_ba"])))


def test_the_table_covers_what_the_contract_distinguishes():
    refs = {c.name: br.reference(c) for c in br.CASES}
    by = {c.name: c for c in br.CASES}
    assert {r["flags"] for r in refs.values()} == {0, 1, 2}
    assert refs["boundary_6x9"]["K"] == 3 and refs["boundary_6x9"]["t0"] == 8
    assert refs["all_kept_8x16"]["K"] == 12 and refs["all_dropped_16x16_f32"]["K"] == 0
    assert refs["t0_none_min_0_1x1"]["t0"] == 1 and refs["explicit_t0_5x7"]["t0"] == 5
    r = refs["shared_and_inactive_only_sources_6x9"]
    assert list(r["frames_eta"]) == [4, 6, 7, 8] and list(r["frames_active"]) == [6, 7, 8]
    c = by["shared_and_inactive_only_sources_6x9"]
    assert br.same_bits(r["damping_buf"][4], c.damping_buf[4])          # a source of inactive edges only: row unchanged
    assert br.same_bits(r["eta"][0], (np.float32(0.2) * c.damping_buf[4] + np.float32(c.ep)).astype(np.float32))
    r = refs["frames_0_and_last_8x16"]
    assert r["frames_active"][0] == 0 and r["frames_active"][-1] == 14 == by["frames_0_and_last_8x16"].nbuf - 1
    for name in ("outside_explicit_t0_5x7", "outside_min_ii_6x9"):
        assert refs[name]["flags"] == 1 and refs[name]["Eb"] == len(refs[name]["ii_ba"])
    assert refs["outside_explicit_t0_5x7"]["t1"] == br.INT_MAX and 2 ** 40 in refs["outside_explicit_t0_5x7"]["ii_ba"]
    assert refs["n_damp_below_G_5x7"]["flags"] == 2 and refs["n_damp_above_G_5x7"]["flags"] == 2
    c, r = by["n_damp_below_G_5x7"], refs["n_damp_below_G_5x7"]
    assert br.same_bits(r["damping_buf"][4], c.damping_buf[4]) and not br.same_bits(r["damping_buf"][3], c.damping_buf[3])
    for name in ("specials_half_5x7", "specials_f32_8x16"):
        c, r = by[name], refs[name]
        row = 2 if name == "specials_half_5x7" else 1       # the eta row of the zeroed damping row
        assert np.all(r["eta"][row] == np.float32(c.ep)), name              # damping 0: eta == ep exactly
        assert np.isnan(r["target_ba"]).sum() == 1 and np.isinf(r["target_ba"]).sum() == 2
        assert np.signbit(r["target_state"].reshape(-1)[-1]) == False and r["target_state"].reshape(-1)[-1] == 0   # noqa: E712
        assert (r["weight_ba"] == 0).sum() >= 2 and (r["weight_ba"] == 1).sum() >= 2    # weights exactly 0 and 1
    half = by["specials_half_5x7"].delta.reshape(-1)
    assert 0 < abs(float(half[19])) < 6.2e-5 and float(half[13]) == 65504.0    # a half subnormal, the largest half
    big = refs["big_2500_edges"]
    assert big["Eb"] > 2500 + 1024 and big["M"] > big["G"] == 300 and 0 < big["K"] < 1300
    assert len({int(f) >> 5 for f in big["frames_eta"]}) > 8                   # the bitmaps span several words


def test_a_fused_multiply_add_would_differ():
    """Why the kernel must not contract 0.2f * d + ep: on random d the fused result differs from the two roundings."""
    rng = np.random.default_rng(0)
    d = rng.uniform(1e-3, 1, 100000).astype(np.float32)
    two = ((np.float32(0.2) * d).astype(np.float32) + np.float32(1e-7)).astype(np.float32)
    fused = (np.float64(np.float32(0.2)) * d.astype(np.float64) + np.float64(np.float32(1e-7))).astype(np.float32)
    assert 0.05 < np.mean(two != fused) < 0.6
