"""Every path the dispatch of csrc/corr.hip can take, held to oracle/corr.py on the cases of tests/corr_cases.py
(tests/test_corr_cases.py proves on the CPU which kernel and which per-tile branch each case runs).  Volume lookups and
their gradient are bit-exact; the alt-corr operators meet a componentwise bar derived from the arithmetic."""
import numpy as np
import pytest

import corr_cases as cc

pytestmark = pytest.mark.gpu


def _torch():
    import torch
    assert torch.cuda.is_available()
    return torch


def _dev(a, offset=False):
    """The array on the device; with `offset` as a contiguous view one element into its storage."""
    torch = _torch()
    t = torch.from_numpy(np.ascontiguousarray(a))
    if not offset:
        return t.cuda()
    buf = torch.zeros(t.numel() + 1, dtype=t.dtype, device="cuda")
    v = buf[1:].view(t.shape)
    v.copy_(t)
    assert v.is_contiguous() and v.storage_offset() == 1 and v.data_ptr() % 16 == t.element_size() % 16
    return v


@pytest.mark.parametrize("case", cc.VOLUME_CASES, ids=lambda c: c.id)
def test_volume_lookup_bit_exact(backends, oracle, case):
    """corr_index_forward, corr_pyramid_forward and its slotted form on small / coop / row / generic, f16 / f32 / f64,
    radii 1..5: integer, .5 and near-integer fractions, windows over each border, empty windows, NaN and +-inf (zeros),
    normal and wide-exponent values, aligned bases and a storage offset of one element."""
    torch = _torch()
    vols, coords, _ = case.build()
    r, rd2 = case.r, (2 * case.r + 1) ** 2
    H1, W1 = case.qmap
    with np.errstate(invalid="ignore"):
        if case.entry == "index":
            ref = oracle.corr_index_forward(vols[0], coords, r)
        else:
            parts = []
            for l, v in enumerate(vols):
                cl = coords * np.float32(1.0 / (1 << l))     # exact
                if case.slotted:
                    live = (case.slots >= 0) & (case.slots < case.cap)
                    o = oracle.corr_index_forward(v[np.where(live, case.slots, 0)], cl, r)
                    o[~live] = 0
                else:
                    o = oracle.corr_index_forward(v, cl, r)
                parts.append(o.reshape(case.B, rd2, H1, W1))
            ref = np.concatenate(parts, 1)
    assert np.isfinite(ref.astype(np.float64)).all()
    dv = [_dev(v, case.offset) for v in vols]
    dc = _dev(coords)
    if case.entry == "index":
        out, = backends.corr_index_forward(dv[0], dc, r)
    elif case.slotted:
        out, = backends.corr_pyramid_forward(dv, dc, r, slots=_dev(case.slots))
    else:
        out, = backends.corr_pyramid_forward(dv, dc, r)
    got = out.cpu().numpy()
    assert got.shape == ref.shape and got.dtype == ref.dtype
    bad = np.argwhere(~(got == ref))
    assert np.array_equal(got, ref), (case.paths(), len(bad), bad[:4].tolist())


@pytest.mark.parametrize("case", cc.INDEX_BACKWARD_CASES, ids=lambda c: c.id)
def test_corr_index_backward_bit_exact(backends, oracle, case):
    """The oracle restates the rounding order of the scatter, so the gradient is exact in every element type; elements no
    window reaches are exactly zero (NaN and +-inf queries reach none)."""
    torch = _torch()
    from oracle import corr as oc
    shape, coords, cg, _ = case.build()
    with np.errstate(invalid="ignore"):
        ref = oc.corr_index_backward(shape, coords, cg, case.r)
    assert np.isfinite(ref.astype(np.float64)).all()
    vol = torch.zeros(shape, dtype=getattr(torch, {"f16": "float16", "f32": "float32", "f64": "float64"}[case.dtype]), device="cuda")
    got, = backends.corr_index_backward(vol, _dev(coords), _dev(cg), case.r)
    got = got.cpu().numpy()
    assert got.dtype == ref.dtype and np.array_equal(got, ref)
    B, H1, W1, H2, W2 = shape
    x1, y1 = cc.bilin_origin(coords[:, 0], coords[:, 1], case.r)
    nt = 2 * case.r + 2
    yy, xx = np.arange(H2)[:, None], np.arange(W2)[None, :]
    reach = ((xx >= x1[..., None, None]) & (xx < x1[..., None, None] + nt) &
             (yy >= y1[..., None, None]) & (yy < y1[..., None, None] + nt))
    assert not got[~reach].any()


@pytest.mark.parametrize("case", cc.ALT_BACKWARD_CASES, ids=lambda c: c.id)
def test_altcorr_backward_componentwise(backends, oracle, case):
    """altcorr_backward on the tiled kernel (hit lists, incoherent tiles, both and an empty tile in one launch, 17 channel
    passes) and on the per-tap kernel (register and atomic branch, radius 2): the project's 2e-5 max-norm bar, and on
    every element |got - ref| <= (n + 8) 2^-24 sum|terms| (corr_cases.backward_bound), which also forces exact zeros
    where nothing contributes.  Measured worst error / bound: profiles/corr_paths_accuracy.txt."""
    torch = _torch()
    from oracle import corr as oc
    f1, f2, coords = case.build()
    rng = np.random.default_rng(case.seed)
    cg = rng.normal(size=(case.B, case.N, (2 * case.r + 1) ** 2) + case.qmap).astype(np.float32)
    r1, r2 = oc.altcorr_backward(f1, f2, coords, cg, case.r)
    n1, n2 = oc.altcorr_backward(np.ones_like(f1), np.ones_like(f2), coords, np.ones_like(cg), case.r)
    a1, a2 = oc.altcorr_backward(np.abs(f1), np.abs(f2), coords, np.abs(cg), case.r)
    g1, g2, gc = backends.altcorr_backward(_dev(f1), _dev(f2), _dev(coords), _dev(cg), case.r)
    g1, g2 = g1.cpu().numpy().astype(np.float64), g2.cpu().numpy().astype(np.float64)
    assert np.isfinite(g1).all() and np.isfinite(g2).all()
    b1, b2 = cc.backward_bound(n1, a1), cc.backward_bound(n2, a2)
    e1, e2 = np.abs(g1 - r1), np.abs(g2 - r2)
    q1 = float((e1[b1 > 0] / b1[b1 > 0]).max())
    q2 = float((e2[b2 > 0] / b2[b2 > 0]).max())
    m1, m2 = e1.max() / np.abs(r1).max(), e2.max() / np.abs(r2).max()
    print(f"ACC altcorr_backward {case.id:34s} {case.backward_path():16s} fmap1_grad err/bound {q1:.3f} max-norm {m1:.1e}   "
          f"fmap2_grad err/bound {q2:.3f} max-norm {m2:.1e}")
    assert m1 < 2e-5 and m2 < 2e-5
    assert (e1 <= b1).all() and (e2 <= b2).all(), (q1, q2)
    assert not g1[b1 == 0].any() and not g2[b2 == 0].any()
    assert float(gc.abs().max()) == 0.0


@pytest.mark.parametrize("case", cc.ALT_FORWARD_CASES, ids=lambda c: c.id)
def test_altcorr_forward_componentwise(backends, oracle, case):
    """altcorr_forward on the generic kernel (f64, f16, an odd radius) and, with border, empty and non-finite queries,
    on the matrix-core, wave and LDS-staged kernels including their per-query branches, which no earlier input reaches:
    |got - ref| <= corr_cases.forward_bound on every element against the fp64 oracle, zeros where no tap is taken."""
    from oracle import corr as oc
    f1, f2, coords = case.build()
    a, b = f1.astype(np.float64), f2.astype(np.float64)
    ref = oc.altcorr_forward(a, b, coords, case.r, acc_dtype=np.float64)
    abs_sum = oc.altcorr_forward(np.abs(a), np.abs(b), coords, case.r, acc_dtype=np.float64)
    out, = backends.altcorr_forward(_dev(f1), _dev(f2), _dev(coords), case.r)
    assert out.dtype == _dev(f1[:1, :1, :1, :1]).dtype
    got = out.cpu().numpy().astype(np.float64)
    assert got.shape == ref.shape and np.isfinite(got).all()
    bound = cc.forward_bound(case, abs_sum, ref)
    err = np.abs(got - ref)
    q = float((err[abs_sum > 0] / bound[abs_sum > 0]).max())
    print(f"ACC altcorr_forward  {case.id:34s} {case.forward_path():16s} err/bound {q:.3f} max-norm {err.max() / np.abs(ref).max():.1e}")
    assert (err <= bound).all(), q
    assert not got[abs_sum == 0].any()
