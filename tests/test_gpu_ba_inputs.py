"""droid_ba_inputs on the device, through the C entry point and through droid_backends.ba_inputs, against the numpy
restatement of its contract (tests/ba_inputs_ref.py), bit for bit on the whole case table: every pixel count that takes
another path (1 x 1, odd planes whose alternate rows are misaligned, planes = 2 mod 4, multiples of 4, one tile + 1),
both network dtypes, the prepare launch's loops beyond its 1024 threads, the flags, and the guarantees around the
values: unwritten rows keep their bits, misplaced buffers and a garbage workspace change nothing, two runs agree, a
side stream works, `ba` fed from it computes what it computes from the stock tail, and sync=False reads nothing."""
import numpy as np
import pytest
import torch

import ba_inputs_ref as br

pytestmark = pytest.mark.gpu
DEV = "cuda"
CODE = {np.dtype(np.float16): 0, np.dtype(np.float32): 1}
OUT_KEYS = ("target_state", "weight_state", "ii_ba", "jj_ba", "target_ba", "weight_ba", "eta", "frames_active",
            "frames_eta", "info")


@pytest.fixture(scope="module")
def refs():
    return {c.name: br.reference(c) for c in br.CASES}   # computed once, shared, never modified


def _dev(x, offset=False):
    """x on the device; offset: one element into a larger buffer, so that no float row is 16-byte aligned"""
    if x is None:
        return None
    t = torch.from_numpy(np.ascontiguousarray(x))
    if not offset:
        return t.to(DEV)
    flat = torch.empty(t.numel() + 1, dtype=t.dtype, device=DEV)
    flat[1:] = t.reshape(-1).to(DEV)
    return flat[1:].view(t.shape)


def _guarded(shape, dtype, offset=False):
    """an output filled with its sentinel"""
    n = int(np.prod(shape)) + (1 if offset else 0)
    if dtype == torch.float32:
        t = torch.full((n,), br.SENTINEL_F32, dtype=torch.int32, device=DEV).view(torch.float32)
    else:
        t = torch.full((n,), br.SENTINEL_I64 if dtype == torch.int64 else br.SENTINEL_I32, dtype=dtype, device=DEV)
    return (t[1:] if offset else t).view(shape)


def _ptr(t):
    return None if t is None else t.data_ptr()


def run_c(lib, c, extra=0, offset=False, ws=None, stream=None):
    """The C entry point on case c with sentinel-filled outputs of capacity E + Ei + extra (edges) and
    min(nbuf, E + Ei) + extra (frames).  Returns the outputs, damping_buf and the inputs after the call as numpy."""
    E, Ei = len(c.ii), len(c.ii_inac)
    h, w = c.a.shape[1:3]
    cap_e, cap_m = E + Ei + extra, min(c.nbuf, E + Ei) + extra
    names = ("ii", "jj", "a", "delta", "w", "damping_net", "damping_buf", "ii_inac", "jj_inac", "target_inac", "weight_inac")
    ins = {k: _dev(getattr(c, k), offset) if (Ei or "inac" not in k) else None for k in names}
    absorb = c.delta is not None
    f32, i64 = torch.float32, torch.int64
    outs = dict(target_state=_guarded((E, h, w, 2), f32, offset) if absorb else None,
                weight_state=_guarded((E, h, w, 2), f32, offset) if absorb else None,
                ii_ba=_guarded((cap_e,), i64, offset), jj_ba=_guarded((cap_e,), i64, offset),
                target_ba=_guarded((cap_e, 2, h, w), f32, offset), weight_ba=_guarded((cap_e, 2, h, w), f32, offset),
                eta=_guarded((cap_m, h, w), f32, offset), frames_active=_guarded((cap_m,), i64, offset),
                frames_eta=_guarded((cap_m,), i64, offset), info=_guarded((8,), torch.int32))
    if ws is None:
        ws = torch.empty(int(lib.droid_ba_inputs_workspace_bytes(E, Ei, c.nbuf)), dtype=torch.uint8, device=DEV)
    rc = lib.droid_ba_inputs(
        *(_ptr(ins[k]) for k in names), E, Ei, h, w, c.nbuf, 0 if c.damping_net is None else len(c.damping_net),
        CODE[c.delta.dtype] if absorb else 1, CODE[c.damping_net.dtype] if c.damping_net is not None else 1, c.t0, c.ep,
        *(_ptr(outs[k]) for k in OUT_KEYS[:6]), cap_e, *(_ptr(outs[k]) for k in OUT_KEYS[6:9]), cap_m,
        outs["info"].data_ptr(), ws.data_ptr(), ws.numel(), stream)
    assert rc == 0, lib.droid_last_error()
    torch.cuda.synchronize()
    got = {k: None if v is None else v.cpu().numpy() for k, v in outs.items()}
    got["damping_buf"] = ins["damping_buf"].cpu().numpy()
    got["inputs"] = {k: None if v is None else v.cpu().numpy() for k, v in ins.items() if k != "damping_buf"}
    return got


def _untouched(x, dtype):
    if x.dtype == np.float32:
        return bool(np.all(x.view(np.uint32) == br.SENTINEL_F32))
    return bool(np.all(x == (br.SENTINEL_I64 if x.dtype == np.int64 else br.SENTINEL_I32)))


def check(c, got, ref):
    assert np.array_equal(got["info"], br.info_of(ref)), (got["info"], br.info_of(ref))
    Eb, M, G = ref["Eb"], ref["M"], ref["G"]
    for key, n in (("ii_ba", Eb), ("jj_ba", Eb), ("target_ba", Eb), ("weight_ba", Eb), ("eta", M), ("frames_eta", M),
                   ("frames_active", G)):
        assert br.same_bits(got[key][:n], ref[key]), key
        assert _untouched(got[key][n:], got[key].dtype), key + ": a row beyond the count was written"
    for key in ("target_state", "weight_state"):
        assert (got[key] is None and ref[key] is None) or br.same_bits(got[key], ref[key]), key
    # the rows of A below n_damp hold the network's damping; every other row of the buffer keeps every bit
    assert np.array_equal(got["damping_buf"].view(np.uint32), ref["damping_buf"].view(np.uint32))
    for k, v in got["inputs"].items():
        if v is not None:
            assert np.array_equal(v.view(np.uint8), np.ascontiguousarray(getattr(c, k)).view(np.uint8)), k + " was written"


@pytest.mark.parametrize("case", br.CASES, ids=repr)
def test_c_entry_point_equals_the_restatement(backends, refs, case):
    """cap_e = E + Ei exactly, then a larger capacity, then every buffer one element off its alignment: the same bits,
    and nothing written beyond the counts."""
    lib = backends._lib.load()
    ref = refs[case.name]
    check(case, run_c(lib, case), ref)
    check(case, run_c(lib, case, extra=3), ref)
    check(case, run_c(lib, case, extra=1, offset=True), ref)


@pytest.mark.parametrize("case", br.CASES, ids=repr)
def test_python_entry_point_equals_the_restatement(backends, refs, case):
    ref = refs[case.name]
    E, Ei = len(case.ii), len(case.ii_inac)
    lead = lambda x: None if x is None else _dev(x)[None]   # noqa: E731  (the factor graph's batch dimension of 1)
    buf = _dev(case.damping_buf)
    inactive = (_dev(case.ii_inac), _dev(case.jj_inac), lead(case.target_inac), lead(case.weight_inac)) if Ei else None
    args = (lead(case.a), lead(case.delta), lead(case.w), lead(case.damping_net), buf, _dev(case.ii), _dev(case.jj))
    kw = dict(inactive=inactive, t0=None if case.t0 < 0 else case.t0, EP=case.ep)
    out = backends.ba_inputs(*args, sync=False, **kw)
    torch.cuda.synchronize()
    assert out.t0 is None and out.t1 is None and out.info.is_cuda
    assert np.array_equal(out.info.cpu().numpy(), br.info_of(ref))
    Eb, M, G = ref["Eb"], ref["M"], ref["G"]
    assert out.ii.shape == (E + Ei,) and out.target.shape == (E + Ei, 2, case.h, case.wd)
    assert out.eta.shape == (min(case.nbuf, E + Ei), case.h, case.wd)
    for t, key, n in ((out.ii, "ii_ba", Eb), (out.jj, "jj_ba", Eb), (out.target, "target_ba", Eb), (out.weight, "weight_ba", Eb),
                      (out.eta, "eta", M), (out.frames_eta, "frames_eta", M), (out.frames, "frames_active", G)):
        assert br.same_bits(t[:n].cpu().numpy(), ref[key]), key
    assert np.array_equal(buf.cpu().numpy().view(np.uint32), ref["damping_buf"].view(np.uint32))
    assert out.target_state.shape == out.weight_state.shape == (1, E, case.h, case.wd, 2)
    if case.delta is not None:
        assert br.same_bits(out.target_state[0].cpu().numpy(), ref["target_state"])
        assert br.same_bits(out.weight_state[0].cpu().numpy(), ref["weight_state"])
    else:   # emit-only: the state is the caller's own
        assert out.target_state.data_ptr() == args[0].data_ptr() and out.weight_state.data_ptr() == args[2].data_ptr()

    buf.copy_(_dev(case.damping_buf))
    if ref["flags"]:
        with pytest.raises(RuntimeError, match="ba_inputs: .*(outside the damping buffer|another number of rows)"):
            backends.ba_inputs(*args, **kw)
        return
    out = backends.ba_inputs(*args, **kw)
    assert (out.t0, out.t1) == (ref["t0"], ref["t1"])
    for t, key in ((out.ii, "ii_ba"), (out.jj, "jj_ba"), (out.target, "target_ba"), (out.weight, "weight_ba"),
                   (out.eta, "eta"), (out.frames_eta, "frames_eta"), (out.frames, "frames_active")):
        assert t.is_contiguous() and br.same_bits(t.cpu().numpy(), ref[key]), key   # trimmed to the counts


def _by_name(name):
    return next(c for c in br.CASES if c.name == name)


def test_a_garbage_workspace_reused_after_a_larger_call(backends, refs):
    lib = backends._lib.load()
    big, small = _by_name("big_2500_edges"), _by_name("boundary_6x9")
    ws = torch.full((int(lib.droid_ba_inputs_workspace_bytes(len(big.ii), len(big.ii_inac), big.nbuf)) + 64,), 0xFF,
                    dtype=torch.uint8, device=DEV)
    check(small, run_c(lib, small, ws=ws), refs[small.name])      # all ones: row tables of -1, counts of -1
    check(big, run_c(lib, big, ws=ws), refs[big.name])
    check(small, run_c(lib, small, ws=ws), refs[small.name])      # the larger call's tables
    ws.fill_(0x7F)
    check(small, run_c(lib, small, ws=ws), refs[small.name])      # huge positive counts and rows


@pytest.mark.parametrize("name", ["specials_half_5x7", "big_2500_edges", "tile_plus_one_25x41"])
def test_two_runs_give_equal_bits(backends, name):
    lib = backends._lib.load()
    a, b = run_c(lib, _by_name(name)), run_c(lib, _by_name(name))
    for key in OUT_KEYS + ("damping_buf",):
        assert np.array_equal(a[key].view(np.uint8), b[key].view(np.uint8)), key   # NaN payloads included


def test_a_call_on_a_side_stream(backends, refs):
    lib = backends._lib.load()
    case = _by_name("all_kept_8x16")
    # A high-priority stream, as tests/test_gpu_graph_mean.py draws its own: PyTorch hands streams out of a pool per
    # priority, in turn, and the runtime maps them onto a few hardware queues.  A default-priority stream drawn here
    # moves every later test one place along that pool, and the overlap test of tests/test_gpu_sharded.py then feeds its
    # spinning solver from a stream that shares the solver's queue: status 8, measured in a whole-suite run.
    side = torch.cuda.Stream(priority=-1)
    with torch.cuda.stream(side):
        check(case, run_c(lib, case, stream=side.cuda_stream), refs[case.name])
        out = backends.ba_inputs(_dev(case.a), _dev(case.delta), _dev(case.w), _dev(case.damping_net),
                                 _dev(case.damping_buf), _dev(case.ii), _dev(case.jj),
                                 inactive=tuple(_dev(getattr(case, k)) for k in ("ii_inac", "jj_inac", "target_inac", "weight_inac")))
        assert br.same_bits(out.target.cpu().numpy(), refs[case.name]["target_ba"])
        assert br.same_bits(out.eta.cpu().numpy(), refs[case.name]["eta"])
    assert (torch.cuda.current_device(), side.cuda_stream) in backends.update_tail._bi_ws   # scratch of its own per stream


def _ba_problem(backends):
    """6 frames, 14 edges, 8 x 16 from the synthetic generator, as a factor graph holds it after an update: the edges
    from frame 3 on are active (coords1 + a half delta), the others inactive (held target / weight)."""
    from droid_backends import synth
    p = synth.make_ba_problem(N=6, E=14, H=8, W=16, seed=3)
    rng = np.random.default_rng(3)
    act = p.ii >= 3
    assert 0 < act.sum() < len(p.ii)
    inter = lambda x: np.ascontiguousarray(x.transpose(0, 2, 3, 1))   # noqa: E731  [E,2,H,W] -> [E,H,W,2]
    delta = rng.normal(0, 0.5, inter(p.targets[act]).shape).astype(np.float16)
    coords1 = (inter(p.targets[act]) - delta.astype(np.float32)).astype(np.float32)
    damping = rng.uniform(1e-3, 0.5, (len(np.unique(p.ii[act])),) + p.disps.shape[1:]).astype(np.float16)
    buf = rng.uniform(1e-3, 0.5, p.disps.shape).astype(np.float32)
    return p, dict(ii=p.ii[act], jj=p.jj[act], coords1=coords1, delta=delta, weight=inter(p.weights[act]).astype(np.float16),
                   damping=damping, buf=buf, ii_inac=p.ii[~act], jj_inac=p.jj[~act], target_inac=inter(p.targets[~act]),
                   weight_inac=inter(p.weights[~act]))


def test_ba_from_ba_inputs_equals_ba_from_the_stock_tail(backends):
    import callers
    p, g = _ba_problem(backends)
    h, w = p.disps.shape[1:]
    d = {k: _dev(v) for k, v in g.items()}
    EP = 1e-7

    # the stock tail (factor_graph.py:213-238), with use_inactive
    buf = d["buf"].clone()
    target = d["coords1"][None] + d["delta"][None].to(dtype=torch.float)
    weight = d["weight"][None].to(dtype=torch.float)
    buf[torch.unique(d["ii"])] = d["damping"].float()
    t0 = p.t0
    m = (d["ii_inac"] >= t0 - 3) & (d["jj_inac"] >= t0 - 3)
    ii = torch.cat([d["ii_inac"][m], d["ii"]], 0)
    jj = torch.cat([d["jj_inac"][m], d["jj"]], 0)
    tg, wt, eta = callers.ba_inputs(torch.cat([d["target_inac"][None][:, m], target], 1),
                                    torch.cat([d["weight_inac"][None][:, m], weight], 1), buf, ii, h, w, EP)

    buf2 = d["buf"].clone()
    inp = backends.ba_inputs(d["coords1"][None], d["delta"][None], d["weight"][None], d["damping"][None], buf2, d["ii"],
                             d["jj"], inactive=(d["ii_inac"], d["jj_inac"], d["target_inac"][None], d["weight_inac"][None]),
                             t0=t0, EP=EP)
    assert (inp.t0, inp.t1) == (p.t0, p.t1) and len(inp.ii) == len(p.ii)
    for a, b in ((inp.ii, ii), (inp.jj, jj), (inp.target, tg), (inp.weight, wt), (inp.eta, eta), (buf2, buf),
                 (inp.target_state, target), (inp.weight_state, weight), (inp.frames, torch.unique(d["ii"]))):
        assert a.shape == b.shape and torch.equal(a, b)   # bit-equal inputs (no NaN here)

    results = []
    for tgt, wgt, et, i, j in ((tg, wt, eta, ii, jj), (inp.target, inp.weight, inp.eta, inp.ii, inp.jj)):
        poses, disps = _dev(p.poses), _dev(p.disps)
        backends.ba(poses, disps, _dev(p.intrinsics), _dev(p.disps_sens), tgt, wgt, et, i, j, p.t0, inp.t1, 2, p.lm, p.ep,
                    False)
        torch.cuda.synchronize()
        assert backends.ba_status()[0] == 0
        results.append((poses.cpu().numpy(), disps.cpu().numpy()))
    assert np.array_equal(results[0][0].view(np.uint32), results[1][0].view(np.uint32))
    assert np.array_equal(results[0][1].view(np.uint32), results[1][1].view(np.uint32))
    assert not np.array_equal(results[0][0], p.poses)   # and ba moved something


def test_sync_false_reads_nothing_on_the_host(backends, refs):
    """Under torch's sync debug mode a blocking read raises.  The mode is first shown to work in this build (an .item()
    raises); if it does not, the call is still made and checked, and the absence of a read is not shown by a tool."""
    case = _by_name("all_kept_8x16")
    args = [_dev(getattr(case, k)) for k in ("a", "delta", "w", "damping_net", "damping_buf", "ii", "jj")]
    inactive = tuple(_dev(getattr(case, k)) for k in ("ii_inac", "jj_inac", "target_inac", "weight_inac"))
    backends.ba_inputs(*args, inactive=inactive, sync=False)   # the scratch exists now
    args[4].copy_(_dev(case.damping_buf))
    probe = torch.ones(1, device=DEV)
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        try:
            probe.item()
            honoured = False
        except RuntimeError:
            honoured = True
        out = backends.ba_inputs(*args, inactive=inactive, sync=False)
        if honoured:
            with pytest.raises(RuntimeError):
                backends.ba_inputs(*args, inactive=inactive, sync=True)   # the one read of `info`
    finally:
        torch.cuda.set_sync_debug_mode("default")
    print(f"sync debug mode honoured by this torch build: {honoured}")
    assert np.array_equal(out.info.cpu().numpy(), br.info_of(refs[case.name]))
    assert br.same_bits(out.eta[:refs[case.name]["M"]].cpu().numpy(), refs[case.name]["eta"])
