"""A result is a function of the arguments only, whatever the workspace held before the call.

Every operator that takes device scratch keeps one grow-only buffer per (device, stream) and reuses it for every call of a
session (droid_backends._workspaces, _prox_ws, _gm_ws), and ba_carve lays its regions out from the call's dimensions: a
call finds the bytes of earlier, differently laid-out calls under its own tables, partial sums, flags and solver scratch.
The stage tests zero their workspace first; this file runs the same checks where the workspace holds 0xFF bytes (NaN as
fp32 and fp64, -1 as an int: a stale index cannot leave the workspace) or what another call left there.  Which launch
writes which region, and what bounds the readers of the regions that are not written completely, is tabulated in
DESIGN.md ("The workspace contract"); the figures measured on the MI355X are in profiles/workspace_history.txt.

  (a) every stage of one Gauss-Newton iteration (run_ba_stages) on a dirty workspace, for a table of graphs that together
      reach every branch of ba_carve / ba_launch_plan / ba_prep_kernel named in BRANCHES -- asserted per case;
  (b) a session: one BaBinding, a fixed sequence of those graphs forward and backward with the workspace kept;
  (c) the same sequence through droid_backends.ba on a side stream whose workspace was filled with 0xFF;
  (d) the deterministic operators bit for bit: proximity_edges, graph_mean / scatter_mean, droid_chol_solve.
"""
import copy
from dataclasses import dataclass, field

import numpy as np
import pytest

import chol_cases as C
import chol_device
import graph_mean_ref as gr
import hard_scenes as hs
import proximity_ref as pr
import shard_cases as sc
import stage_graphs as sg
from util import (HDR_M, HDR_NC1, HDR_NC2, PACKED_BAR, STAGE_BARS, assert_system_close, run_ba_stages, run_hip_ba,
                  scaled_system_errors, slot_classes, stage_errors, stage_state_relative, stepwise_parity)

pytestmark = pytest.mark.gpu

POSE_BAR, DISP_BAR = 1e-6, 1e-5     # "same arithmetic, another dispatch" (test_hard_scene_through_the_public_entry)
# Clean against dirty, scaled system: PACKED_BAR, the project's figure for the same sums in another order of the fp64
# atomics.  A graph whose CLEAN runs already differ by more gets 4 x its largest clean-against-clean difference over five
# repeats (clean_spread below, measured before any dirty run; profiles/workspace_history.txt): none does.
CLEAN_BARS = {}


def _torch():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    return torch


def _synth():
    from droid_backends import synth
    return synth


# ---------------------------------------------------------------------------------------------------------------------
# The table of (a).  A case claims the branches it is there for (`covers`); `reached` restates ba_carve and
# ba_launch_plan on the host (like stage_graphs.predicted_classes restates the classes) and reads the classes from the
# device's header and hint words; a case that stops reaching a branch it claims fails its test.
BRANCHES = {"class0", "class1", "class2", "class3", "wide", "not_wide", "zsplit>1", "zsplit=1", "s2_split>1", "pair_taken",
            "pair_skipped", "motion_only", "t0>1", "stereo", "rgbd", "packed", "E=0", "own",
            "prep_global"}      # ba_prep_kernel with its work arrays in the workspace itself, not in LDS
LIN_WGS, LIN_CP, S2_WGS = 1536, 512, 1536      # csrc/ba_internal.hpp
PREP_LDS_BYTES = 150 * 1024                    # launch_prep: above it the tables are built in global memory


@dataclass
class Case:
    name: str
    make: object                 # () -> (problem, own or None)
    family: str                  # util.STAGE_BARS
    covers: set
    motion_only: bool = False
    packed: bool = False
    hard: str = None             # id of hard_scenes.SCENES: its bars
    classes: object = None       # the exact set the device must report; None: predicted on the host (a shard)
    _made: object = field(default=None, repr=False)

    def problem(self):
        if self._made is None:
            self._made = self.make()
        return self._made


def _graph(name):
    return lambda: (sg.GRAPHS[name][0](_synth()), None)


def _hard(sid):
    return lambda: (hs.SCENES[sid].problem(), None)


def _empty_graph():
    """E = 0 the way test_gpu_ba_full.py::test_empty_graph_is_a_noop builds it: the window's eta rows remain."""
    p = _synth().make_ba_problem(N=5, E=12, H=16, W=24, seed=3)
    p.ii, p.jj = p.ii[:0], p.jj[:0]
    p.targets, p.weights = p.targets[:0], p.weights[:0]
    p.eta = np.ascontiguousarray(p.eta[:p.t1 - p.t0]) if p.eta.shape[0] >= p.t1 - p.t0 else \
        np.full((p.t1 - p.t0,) + p.disps.shape[1:], 1e-3, np.float32)
    return p, None


def _shard_rank():
    """Rank 1 of shard_cases' cut at frame 6: window [3, 8) in a buffer of 12, own = (6, 12)."""
    _, _, shards = sc.shards(sc.CASES["cut_sweep[6]"])
    q = shards[1]
    return q, q.own


def _all_pairs():
    """100 frames, every ordered pair, 8x8 pixels: 9900 edges, more than the LDS of ba_prep_kernel<true> holds, so the
    tables are counted and scanned in the workspace's own arrays (99 edges and 601 rows per slot: class 3 everywhere)."""
    N = 100
    pairs = [(i, j) for i in range(N) for j in range(N) if i != j]
    return _synth().make_ba_problem(N=N, H=8, W=8, seed=41, lm=1e-4, ep=0.1, edges=sg._edges(pairs)), None


def _g(name, covers, **kw):
    _, family, classes = sg.GRAPHS[name]
    return Case(name, _graph(name), family, set(covers), motion_only=classes == {"motion"}, classes=classes, **kw)


def _h(sid, covers):
    s = hs.SCENES[sid]
    return Case(sid, _hard(sid), s.family, set(covers), motion_only=s.motion_only, packed=s.packed, hard=sid,
                classes=s.classes)


CASES = {c.name: c for c in [
    _g("cfg1", {"class0", "not_wide", "zsplit>1", "s2_split>1", "packed", "pair_skipped"}, packed=True),
    _g("dense20_few_stages", {"class0", "class1", "wide", "zsplit>1"}),
    _g("dense30_block_pair", {"class3", "not_wide", "pair_taken"}),
    _g("dense36_syrk", {"class1", "wide"}),
    _g("every_class", {"class0", "class1", "class2", "class3", "wide", "packed", "pair_taken"}, packed=True),
    _g("cfg3", {"zsplit=1", "class0", "not_wide"}),     # the smallest graph of the tables with M * chunks > LIN_WGS / 2
    _g("variant_window_t0_3", {"t0>1"}),
    _g("variant_rgbd", {"rgbd"}),
    _g("variant_stereo_pairs", {"stereo"}),
    _g("motion_only", {"motion_only", "packed"}, packed=True),
    Case("empty_graph", _empty_graph, "sparse", {"E=0", "class0"}, classes={0}),
    Case("shard_cut6_rank1", _shard_rank, "sparse", {"own", "t0>1"}, packed=True),
    _h("win9x19-rot5-plain", {"class0"}),
    _h("win13x21-rot20-negated", {"class0"}),
    _h("win8x32-rot20-stereo", {"stereo"}),
    _h("win9x19-rot60-rgbd", {"rgbd"}),
    _h("hard_variant_window_t0_3", {"t0>1"}),
    _h("hard_motion_only", {"motion_only", "packed"}),
    _h("ladder", {"class0"}),
    Case("all_pairs100", _all_pairs, "dense", {"prep_global", "class3", "pair_taken"}, classes={3}),
]}
assert BRANCHES <= set().union(*(c.covers for c in CASES.values())), "a branch of the list has no case"


def dims(case):
    """(E, nbuf, H, W, M, t0, t1) the way BaBinding.begin takes them from the tensors."""
    p, _ = case.problem()
    nbuf, H, W = p.disps.shape
    return len(p.ii), nbuf, H, W, 0 if case.motion_only else p.eta.shape[0], p.t0, p.t1


def plan(case):
    """Host restatement of the numbers ba_carve / ba_launch_plan derive from the dimensions (csrc/ba_internal.hpp)."""
    E, nbuf, H, W, M, t0, t1 = dims(case)
    HW = H * W
    nch = (HW + LIN_CP - 1) // LIN_CP
    wide = M > 0 and E >= 12 * M and HW % 32 == 0
    zsplit = min(max(LIN_WGS // (M * nch), 1), 8) if M > 0 else 1
    s2_split = min(max(S2_WGS // M, 1), (HW + 63) // 64) if M > 0 else 1
    return dict(wide=wide, zsplit=zsplit, s2_split=s2_split, depth=M > 0)


def reached(case, st):
    """The branches of BRANCHES one run of `case` took: the classes from the device's words, the rest restated."""
    p, own = case.problem()
    pl = plan(case)
    got = slot_classes(st, case.motion_only)
    out = {f"class{c}" for c in got if c != "motion"}
    if case.motion_only:
        out.add("motion_only")
    if pl["depth"]:
        out.add("wide" if pl["wide"] else "not_wide")
        out.add("zsplit>1" if pl["zsplit"] > 1 else "zsplit=1")
        if pl["s2_split"] > 1:
            out.add("s2_split>1")
        # launch_build_stage leaves the block-pair launch out when the hint of this call's prepare has arrived and names
        # no class-3 slot.  run_ba_stages synchronises before the packed build: the hint is there (slot_classes asserts
        # its tag), so that build skips the launch exactly when n3 == 0; with class-3 slots every build launches it.
        n3 = st["hint"][1]
        if n3 > 0:
            out.add("pair_taken")
        elif case.packed:
            out.add("pair_skipped")
    if p.t0 > 1:
        out.add("t0>1")
    if len(p.ii) and bool((p.ii == p.jj).any()):
        out.add("stereo")
    if bool((p.disps_sens > 0).any()):
        out.add("rgbd")
    if case.packed and "system_packed" in st:
        out.add("packed")
    if len(p.ii) == 0 and pl["depth"]:
        out.add("E=0")
    if own is not None and tuple(own) != (0, p.disps.shape[0]):
        out.add("own")
    if 4 * (9 * (p.disps.shape[0] + 2) + 4 * (len(p.ii) + 1)) > PREP_LDS_BYTES:      # prep_lds_ints (csrc/ba_kernels.hip)
        out.add("prep_global")
    return out, got


def ws_bytes(backends, case):
    E, nbuf, H, W, M, t0, t1 = dims(case)
    return int(backends._lib.load().droid_ba_workspace_bytes(E, nbuf, H, W, t0, t1, M))


def run(backends, case, binding=None, fill="zero"):
    p, own = case.problem()
    st = run_ba_stages(backends, p, _torch(), motion_only=case.motion_only, packed=case.packed, own=own, binding=binding,
                       fill=fill)
    if st["status"] & 8:   # a bounded spin of the single-launch solver ran out: nothing further on this device
        pytest.exit(f"{case.name} ({fill}): the solver reported a stalled grid (status {st['status']}): find the reader of "
                    "unwritten scratch before anything runs again", 3)
    return st


_clean = {}


def clean(backends, name):
    """The fill="zero" run of case `name` on a workspace of its own, once per session."""
    if name not in _clean:
        _clean[name] = run(backends, CASES[name])
    return _clean[name]


def system_distance(a, b, n):
    """util.scaled_system_errors of system `a` against system `b` ([n + 1, n], row n = rhs): (max of H and b, stray + dead)"""
    e = scaled_system_errors(a[:n], a[n], b[:n], b[n])
    return max(e["H"], e["b"]), e["stray"] + e["dead"]


def clean_spread(backends, name, repeats=5):
    """Largest clean-against-clean distance of `repeats` further fill="zero" runs from the session's clean run: the
    figure the contingency of CLEAN_BARS is decided on (to be measured before any dirty run is looked at)."""
    ref = clean(backends, name)
    n = ref["system"].shape[1]
    worst = 0.0
    for _ in range(repeats):
        st = run(backends, CASES[name])
        worst = max(worst, system_distance(st["system"], ref["system"], n)[0])
    return worst


def check(backends, oracle, case, st, tag):
    """The checks of check_graph / test_hard_scene_stages_match_oracle on the run `st` of `case`, then `st` against the
    clean run of the same inputs.  Prints the line of profiles/workspace_history.txt."""
    p, own = case.problem()
    mo = case.motion_only
    took, got = reached(case, st)
    err = stage_errors(oracle, p, st, mo, own=own)
    fam = STAGE_BARS[case.family]
    if case.hard:
        hb = hs.bars(case.hard)
        bars = dict(H=hb["H"], b=hb["b"], dx=hb["dx"], state=hb["state"])
        state = max(stage_state_relative(oracle, p, st, mo))
    elif own is not None:
        bars = dict(fam)
        bars.update({k: v for k, v in sc.shard_bars(oracle, p, case.family, mo)[0].items() if k in ("H", "b")})
        state = err["state"]
    else:
        bars, state = fam, err["state"]
    classes = case.classes if case.classes is not None else sc.shard_classes(p)
    ref = clean(backends, case.name)
    n = ref["system"].shape[1]
    d_sys, d_stray = system_distance(st["system"], ref["system"], n)
    d_pk = system_distance(st["system_packed"], ref["system_packed"], n) if "system_packed" in st else (0.0, 0)
    d_pose = float(np.abs(st["poses"] - ref["poses"]).max())
    d_disp = float(np.abs(st["disps"] - ref["disps"]).max())
    new_nan = {k: int((np.isnan(st[k]) & ~np.isnan(ref[k])).sum()) for k in ("dx", "dz", "poses", "disps")}
    hdr, n3 = st["hdr"], st["hint"][1]
    print(f"ws_history {tag} [{case.name}] classes {sorted(got, key=str)} (M={hdr[HDR_M]} nc1={hdr[HDR_NC1]} nc2={hdr[HDR_NC2]} "
          f"n3={n3}) H {err['H']:.2e} / {bars['H']:.2e} b {err['b']:.2e} / {bars['b']:.2e} dx {err['dx']:.2e} / {bars['dx']:.2e} "
          f"state {state:.2e} / {bars['state']:.2e} stray {err['stray']} dead {err['dead']}"
          + (f" packed {err['packed']:.1e}/{err['packed_stray']}" if "packed" in err else "")
          + f" | against clean: system {d_sys:.1e} packed {d_pk[0]:.1e} poses {d_pose:.1e} disps {d_disp:.1e} new NaN "
          f"{sum(new_nan.values())} | branches {' '.join(sorted(case.covers))}")
    assert st["status"] & 15 == 0, (tag, st["status"])
    assert got == classes, (tag, got, classes)
    assert case.covers <= took, (tag, "the case no longer reaches", sorted(case.covers - took))
    if not mo:
        assert st["M"] == p.eta.shape[0], (tag, st["M"])
    assert_system_close(err, bars, tag)
    if "packed" in err:
        assert err["packed_stray"] == 0 and err["packed"] < PACKED_BAR, (tag, err["packed"])
    assert err["dx"] < bars["dx"], (tag, err["dx"], bars["dx"])
    assert state < bars["state"], (tag, state, bars["state"])
    bar = CLEAN_BARS.get(case.name, PACKED_BAR)
    assert d_stray == 0 and d_sys < bar, (tag, "system against the clean run", d_sys, d_stray)
    assert d_pk[1] == 0 and d_pk[0] < bar, (tag, "packed system against the clean run", d_pk)
    assert d_pose < POSE_BAR and d_disp < DISP_BAR, (tag, "state against the clean run", d_pose, d_disp)
    assert not any(new_nan.values()), (tag, "NaN where the clean run has none", new_nan)


def _binding(backends, nbytes):
    from droid_backends.ba_binding import BaBinding
    b = BaBinding(status_mirror=False, headroom=(1, 0))
    b.reserve(nbytes, "cuda")
    return b


# ------------------------------------------------------------------------------------------------------------ (a)
@pytest.mark.parametrize("fill", ["history", "ff"])
@pytest.mark.parametrize("name", list(CASES))
def test_every_stage_on_a_dirty_workspace(backends, oracle, name, fill):
    """ff: every byte of the workspace 0xFF.  history: the table's previous entry runs first through the same binding
    (itself from 0xFF bytes, so that no byte the case finds is a benign zero), then this one with the workspace kept."""
    case = CASES[name]
    clean(backends, name)
    if fill == "ff":
        st = run(backends, case, fill="ff")
    else:
        names = list(CASES)
        before = CASES[names[names.index(name) - 1]]
        b = _binding(backends, max(ws_bytes(backends, case), ws_bytes(backends, before)))
        try:
            run(backends, before, binding=b, fill="ff")
            st = run(backends, case, binding=b, fill="keep")
        finally:
            b.close()
        fill = f"history({before.name})"
    check(backends, oracle, case, st, fill)


# ------------------------------------------------------------------------------------------------------------ (b)
SESSION = ["every_class", "cfg1", "motion_only", "dense30_block_pair", "empty_graph", "dense36_syrk", "variant_window_t0_3",
           "shard_cut6_rank1", "dense20_few_stages", "win8x32-rot20-stereo"]


def _traits(backends, name):
    case = CASES[name]
    E = dims(case)[0]
    return dict(bytes=ws_bytes(backends, case), mo=case.motion_only, E=E, packed=case.packed, wide=plan(case)["wide"],
                c3=case.classes is not None and 3 in case.classes)


def session_transitions(backends, names):
    """The transitions of the list in (b) that occur along `names`."""
    t = [_traits(backends, n) for n in names]
    out = set()
    for a, b in zip(t, t[1:]):
        if a["bytes"] > b["bytes"]:
            out.add("large->small")
        if a["bytes"] < b["bytes"]:
            out.add("small->large")
        if a["packed"] and not b["packed"]:
            out.add("packed->pitched")
        if a["wide"] and not b["wide"]:
            out.add("wide->not wide")
        if a["c3"] and not b["c3"]:
            out.add("class 3->none")
    for a, b, c in zip(t, t[1:], t[2:]):
        if not a["mo"] and b["mo"] and not c["mo"]:
            out.add("full->motion_only->full")
        if a["E"] > 0 and b["E"] == 0 and c["E"] > 0:
            out.add("E>0->E=0->E>0")
    return out


def test_a_session_on_one_workspace(backends, oracle):
    """One BaBinding reserved once to the largest case; the sequence forward, then backward, the workspace kept all along
    (0xFF bytes before the first step).  Every step is checked like a case of (a)."""
    need = {"large->small", "small->large", "full->motion_only->full", "E>0->E=0->E>0", "packed->pitched", "wide->not wide",
            "class 3->none"}
    assert need <= session_transitions(backends, SESSION), need - session_transitions(backends, SESSION)
    b = _binding(backends, max(ws_bytes(backends, CASES[n]) for n in SESSION))
    buf = b.buf.data_ptr()
    b.buf.fill_(0xFF)
    try:
        for direction, names in (("forward", SESSION), ("backward", SESSION[::-1])):
            for k, name in enumerate(names):
                st = run(backends, CASES[name], binding=b, fill="keep")
                check(backends, oracle, CASES[name], st, f"session {direction} step {k}")
                assert b.buf.data_ptr() == buf      # one workspace all along
    finally:
        b.close()


# ------------------------------------------------------------------------------------------------------------ (c)
PUBLIC = [n for n in SESSION if n != "shard_cut6_rank1"]      # droid_backends.ba has no `own`
TWO_ITERATIONS = ("cfg1", "dense20_few_stages")


def test_the_public_entry_on_a_side_stream(backends, oracle):
    """The session through droid_backends.ba(iterations=1) on a stream of its own, whose workspace object the module
    creates: sized by the largest call, filled with 0xFF, never zeroed again.  Every step ends in the state the phase
    ABI produced from a zeroed workspace; two steps run two iterations (each against the oracle from the device's own
    state, and the composite call against the chained ones, as test_gpu_ba_full.py::_parity does).  No call reports an
    error through the status mirror."""
    torch = _torch()
    assert max(PUBLIC, key=lambda n: ws_bytes(backends, CASES[n])) == PUBLIC[0]
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):
        first, _ = CASES[PUBLIC[0]].problem()
        run_hip_ba(backends, copy.deepcopy(first), torch, 1, CASES[PUBLIC[0]].motion_only)
        wso = backends._workspace_obj(torch.device("cuda", torch.cuda.current_device()))
        assert wso.buf is not None and backends._workspaces[(torch.cuda.current_device(), s.cuda_stream)] is wso
        buf, errors = wso.buf.data_ptr(), int(wso.mirror[2])
        wso.buf.fill_(0xFF)
        for direction, names in (("forward", PUBLIC), ("backward", PUBLIC[::-1])):
            for k, name in enumerate(names):
                case = CASES[name]
                p, _ = case.problem()
                ref = clean(backends, name)
                hip = run_hip_ba(backends, copy.deepcopy(p), torch, 1, case.motion_only)
                d_pose = float(np.abs(hip["poses"] - ref["poses"]).max())
                d_disp = float(np.abs(hip["disps"] - ref["disps"]).max())
                print(f"ws_history public {direction} step {k} [{name}] status {hip['status']} against the clean phase ABI: "
                      f"poses {d_pose:.1e} disps {d_disp:.1e}")
                assert hip["status"] & 15 == 0 and hip["M"] == ref["M"], (name, hip["status"], hip["M"])
                assert d_pose < POSE_BAR and d_disp < DISP_BAR, (name, d_pose, d_disp)
                assert not np.isnan(hip["dx"]).any() and not np.isnan(hip["dz"]).any(), name
                if name in TWO_ITERATIONS:
                    chained, worst = stepwise_parity(backends, oracle, copy.deepcopy(p), torch, 2, 1e-4, f"{name} x2")
                    two = run_hip_ba(backends, copy.deepcopy(p), torch, 2)
                    d2p = float(np.abs(two["poses"] - chained.poses).max())
                    d2d = float(np.abs(two["disps"] - chained.disps).max())
                    print(f"ws_history public {direction} step {k} [{name}] two iterations: worst per-iteration distance "
                          f"from the oracle {max(worst):.1e}, composite against chained poses {d2p:.1e} disps {d2d:.1e}")
                    assert two["status"] & 15 == 0 and d2p < POSE_BAR and d2d < DISP_BAR, (name, two["status"], d2p, d2d)
                assert wso.buf.data_ptr() == buf, "the workspace grew: the 0xFF fill is gone"
        assert int(wso.mirror[2]) == errors, (int(wso.mirror[2]), int(wso.mirror[3]))


# ------------------------------------------------------------------------------------------------------------ (d)
STATES = ["zeros", "ones", "larger"]      # the scratch holds 0x00 bytes, 0xFF bytes, what a larger call left


def _dev(a):
    return _torch().from_numpy(np.ascontiguousarray(a)).cuda()


def _edge_lists(edges):
    e = np.asarray(edges, np.int64).reshape(-1, 2)
    return _dev(e[:, 0].copy()), _dev(e[:, 1].copy())


def _prox_known():
    d, args = pr.banded(140, 5), (140, 0, 0, 2, 1, 18.0, 10000, True)
    full = pr.proximity_edges(d, *args, [])
    return d, args, [tuple(e) for e in full[::3].tolist()] + [(1000, 2), (3, 1000)]


# one test_gpu_proximity.py shape per path: (matrix, (t, t0, t1, rad, nms, thresh, max_factors, stereo), known edges)
PROX = {
    "frontend_rectangle": lambda: (pr.random_symmetric(100, 100), (100, 95, 75, 2, 1, 30.0, 10000, False), None),
    "whole_matrix_t0_t1_0": lambda: (pr.random_symmetric(100, 12), (100, 0, 0, 2, 1, 20.0, 10000, False), None),
    "more_than_one_lds_sort": lambda: (pr.random_symmetric(320, 2), (320, 0, 0, 2, 1, 45.0, 100000, False), None),
    "known_edges_hash": _prox_known,
}
_prox = {}


def _prox_case(name):
    """(device matrix, args, known, expected edges, statistics of the restatement), once per session"""
    if name not in _prox:
        d, args, known = PROX[name]()
        d = np.asarray(d, np.float32)
        st = {}
        want = pr.proximity_edges(d, *args, [], known, stats=st)
        _prox[name] = (d, args, known, want, st)
    return _prox[name]


def _prox_call(backends, d, args, known):
    t, t0, t1, rad, nms, thresh, mf, stereo = args
    si, sj = _edge_lists([])
    ki, kj = _edge_lists(known) if known is not None else (None, None)
    ii, jj = backends.proximity_edges(None, None, None, t, t0, t1, rad, nms, 0.25, thresh, mf, stereo, si, sj, ki, kj,
                                      dist=_dev(d))
    return np.stack([ii.cpu().numpy(), jj.cpu().numpy()], 1)


def _prox_larger(backends):
    """A call with another t, t0, t1 and n_known whose scratch is larger than that of every case of PROX."""
    if "larger" not in _prox:
        _prox["larger"] = (pr.random_symmetric(400, 6), (400, 7, 3, 3, 2, 40.0, 100000, True),
                           [(int(i), int(j)) for i in range(0, 400, 3) for j in range(0, 400, 4)])
    d, args, known = _prox["larger"]
    return _prox_call(backends, d, args, known)


@pytest.mark.parametrize("state", STATES)
@pytest.mark.parametrize("name", list(PROX))
def test_proximity_edges_from_any_scratch(backends, name, state):
    """The edge list, order included, equals tests/proximity_ref.py whatever droid_backends._prox_ws holds: the header
    (memset), the candidate counter and keys, the merge target and the known-edge hash (cleared by prox_compact)."""
    torch = _torch()
    lib = backends._lib.load()
    d, args, known, want, st = _prox_case(name)
    assert st.get("accepted", 0) >= 8, ("badly chosen input", st)
    if name == "more_than_one_lds_sort":
        assert st["under"] > 2 * 16384
    big = _prox_larger(backends)                 # sizes the scratch: grow-only, so every case below runs in this buffer
    assert len(big) > 0
    ws = backends._prox_ws[backends._ws_key(torch.device("cuda", torch.cuda.current_device()))]
    t, t0, t1 = args[:3]
    cap = backends.proximity_edge_bound(t, t0, t1, args[3], args[6], args[7])
    assert ws.numel() >= lib.droid_proximity_workspace_bytes(t, t0, t1, 0 if known is None else len(known), cap)
    if state == "zeros":
        ws.zero_()
    elif state == "ones":
        ws.fill_(0xFF)
    got = _prox_call(backends, d, args, known)
    assert backends._prox_ws[backends._ws_key(torch.device("cuda", torch.cuda.current_device()))] is ws
    print(f"ws_history proximity [{name}] scratch {state}: {st} -> {len(want)} edges, device {len(got)}")
    assert got.shape == want.shape, (got.shape, want.shape)
    bad = np.flatnonzero((got != want).any(1))
    assert bad.size == 0, (bad[:5], got[bad[:5]], want[bad[:5]])


GM = [(compact, dtype, E, rng) for compact in (0, 1) for dtype in gr.DTYPES for E in (8192, 8193) for rng in (1, 16384)]
GM_PLANE = 8
GM_LARGER = (20000, 16384)        # E, range of the larger call
_gm = {}


def _gm_problem(compact, dtype, E, rng):
    """x [E, GM_PLANE], index [E] (a few entries outside [0, range)), rows of out, the expected bits and group count"""
    key = (compact, dtype, E, rng)
    if key not in _gm:
        r = np.random.default_rng(E + 7 * rng + compact)
        frames = r.choice(rng, min(rng, 300), replace=False)
        index = np.concatenate([frames[r.integers(0, len(frames), E - 40)], r.choice([-1, rng, 2 ** 40, -2 ** 40], 40)])
        index = index[r.permutation(E)].astype(np.int64)
        x = r.normal(0.0, 4.0, (E, GM_PLANE)).astype(dtype)
        D = len(np.unique(index[(index >= 0) & (index < rng)]))
        M = min(D + 2, rng + 1) if compact else rng
        _gm[key] = (x, index, M, gr.ref(x, index, M, rng, compact), D)
    return _gm[key]


def _gm_call(backends, ws, x, index, M, rng, compact):
    torch = _torch()
    lib = backends._lib.load()
    dtype = x.dtype.type
    out = torch.full((M, x.shape[1]), float("nan"), dtype={np.float16: torch.float16, np.float32: torch.float32}[dtype],
                     device="cuda")
    groups = torch.full((1,), -7, dtype=torch.int32, device="cuda")
    src, idx = _dev(x), _dev(index)
    rc = lib.droid_graph_mean(src.data_ptr(), idx.data_ptr(), out.data_ptr(), len(index), x.shape[1], M, rng, compact,
                              {np.float16: 0, np.float32: 1}[dtype], groups.data_ptr(), ws.data_ptr(), ws.numel(),
                              torch.cuda.current_stream().cuda_stream)
    assert rc == 0, lib.droid_last_error()
    torch.cuda.synchronize()
    return out.cpu().numpy(), int(groups.item())


@pytest.mark.parametrize("state", STATES)
@pytest.mark.parametrize("compact,dtype,E,rng", GM, ids=[f"{'compact' if c else 'dense'}-{d.__name__}-E{E}-range{r}"
                                                          for c, d, E, r in GM])
def test_graph_mean_from_any_scratch(backends, compact, dtype, E, rng, state):
    """droid_graph_mean (graph_mean: compact, scatter_mean: dense) equals tests/graph_mean_ref.py bit for bit, groups_out
    included, whatever its workspace (offsets, entry lists) holds; E on both sides of the LDS sort's limit."""
    torch = _torch()
    lib = backends._lib.load()
    x, index, M, want, D = _gm_problem(compact, dtype, E, rng)
    ws = torch.empty(int(lib.droid_graph_mean_workspace_bytes(*GM_LARGER)), dtype=torch.uint8, device="cuda")
    assert ws.numel() > lib.droid_graph_mean_workspace_bytes(E, rng) > 0
    if state == "zeros":
        ws.zero_()
    elif state == "ones":
        ws.fill_(0xFF)
    else:
        r = np.random.default_rng(1)
        xl = r.normal(0.0, 1.0, (GM_LARGER[0], 4)).astype(np.float32)
        il = r.integers(0, GM_LARGER[1], GM_LARGER[0]).astype(np.int64)
        _gm_call(backends, ws, xl, il, GM_LARGER[1], GM_LARGER[1], 0)
    got, groups = _gm_call(backends, ws, x, index, M, rng, compact)
    assert gr.same_bits(got, want), (state, int((got.view(np.uint8) != want.view(np.uint8)).sum()))
    assert groups == D, (groups, D)


def test_graph_mean_entry_points_on_a_hostile_module_scratch(backends):
    """graph_mean / scatter_mean through the Python entry points, droid_backends._gm_ws filled with 0xFF after a larger
    call has sized it."""
    torch = _torch()
    r = np.random.default_rng(1)
    big = _dev(r.normal(0.0, 1.0, (GM_LARGER[0], 4)).astype(np.float32))
    backends.scatter_mean(big, _dev(r.integers(0, GM_LARGER[1], GM_LARGER[0]).astype(np.int64)), dim=0, dim_size=GM_LARGER[1])
    torch.cuda.synchronize()
    mine = [w for (dev, stream), w in backends._gm_ws.items() if stream == torch.cuda.current_stream().cuda_stream]
    assert len(mine) == 1
    for compact in (0, 1):
        x, index, M, want, D = _gm_problem(compact, np.float16, 8193, 16384)
        mine[0].fill_(0xFF)
        if compact:
            got = backends.graph_mean(_dev(x).view(-1, GM_PLANE, 1, 1), _dev(index), num_groups=M, nbuf=16384).view(M, GM_PLANE)
        else:
            got = backends.scatter_mean(_dev(x), _dev(index), dim=0, dim_size=M)
        assert gr.same_bits(got.cpu().numpy(), want), compact
    assert [w for (dev, stream), w in backends._gm_ws.items() if stream == torch.cuda.current_stream().cuda_stream][0] is mine[0]


CHOL_LARGER = 641


def _chol_problem(n):
    return (C.spectrum_matrix(np.random.default_rng(n), n, np.logspace(0, -6, n)),
            np.random.default_rng(n + 1).normal(size=n))


def _chol(lib, A, b, scratch=None):
    rc, fl, x, scratch = chol_device.solve(lib, _torch(), A, b, scratch)
    if fl == 2:
        pytest.exit("droid_chol_solve reported a stalled grid (flag 2): find the cause before anything runs again", 3)
    return rc, fl, x, scratch


@pytest.mark.parametrize("n", [63, 64, 65, 129, 378])
def test_chol_solve_from_any_scratch(backends, n):
    """x of droid_chol_solve is bit-identical on a fresh scratch and on one sized for n = 641 that holds 0x00 bytes, 0xFF
    bytes, or what a solve of n = 641 left (test_repeated_solves_are_bit_identical: the solver is deterministic)."""
    torch = _torch()
    lib = backends._lib.load()
    A, b = _chol_problem(n)
    rc, fl, x0, _ = _chol(lib, A, b)
    assert rc == 0 and fl == 0 and np.all(np.isfinite(x0))
    scratch = torch.empty(lib.droid_chol_scratch_doubles(CHOL_LARGER), dtype=torch.float64, device="cuda")
    assert scratch.numel() > lib.droid_chol_scratch_doubles(n)
    for state in STATES:
        if state == "zeros":
            scratch.zero_()
        elif state == "ones":
            scratch.view(torch.uint8).fill_(0xFF)
        else:
            rc, fl, xl, _ = _chol(lib, *_chol_problem(CHOL_LARGER), scratch)
            assert rc == 0 and fl == 0 and np.all(np.isfinite(xl))
        rc, fl, x, _ = _chol(lib, A, b, scratch)
        assert rc == 0 and fl == 0, (state, rc, fl)
        assert np.array_equal(x.view(np.uint64), x0.view(np.uint64)), (n, state, float(np.abs(x - x0).max()))


def test_chol_solve_after_a_failing_one_on_a_hostile_scratch(backends):
    """A failing case of chol_cases on a 0xFF scratch raises the flag; the good solve behind it, in the same scratch, gives
    the bits of a fresh one."""
    torch = _torch()
    lib = backends._lib.load()
    c = min(C.FAILING, key=lambda c: c.n)
    A, b = c.build()
    scratch = torch.empty(lib.droid_chol_scratch_doubles(max(c.n, CHOL_LARGER)), dtype=torch.float64, device="cuda")
    scratch.view(torch.uint8).fill_(0xFF)
    rc, fl, _, _ = _chol(lib, A, b, scratch)
    assert rc == 0 and fl == 1, (c.name, rc, fl)
    rng = np.random.default_rng(c.n)
    G, g = C._well(rng, c.n), rng.normal(size=c.n)
    rc, fl, x0, _ = _chol(lib, G, g)
    assert rc == 0 and fl == 0 and np.all(np.isfinite(x0))
    rc, fl, x, _ = _chol(lib, G, g, scratch)
    assert rc == 0 and fl == 0 and np.array_equal(x.view(np.uint64), x0.view(np.uint64)), (c.name, rc, fl)
