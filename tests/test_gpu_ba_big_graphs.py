"""Stage-by-stage parity of one Gauss-Newton iteration on graphs that take the code chosen by size alone
(tests/big_graphs.py; proved to reach it, and to be decided by it, on the CPU by tests/test_big_graphs.py):

  * source frames with more than SLOT_MAXE = 128 edges: the metadata reload inside ba_lin_kernel's edge loop (with and
    without ZSPLIT, with and without EROWS), the streaming path of ba_schur_fused_kernel (`resident == false`: entry base
    carried from chunk to chunk, weights read from memory) and the chunk loop of ba_backsub_kernel;
  * prep tables at the full 150 KB of dynamic LDS (ba_prep_kernel<true>) and outside it (ba_prep_kernel<false>), from a
    zeroed workspace, from 0xFF bytes and from what another call left.

The harness is the one of tests/test_gpu_ba_stages.py::test_hard_scene_stages_match_oracle: run_ba_stages, slot_classes,
stage_errors, stage_state_relative, with the bars of big_graphs.bars -- derived per scene from the oracle's own float32
evaluation, the number formats and the condition of the scene; nothing in them is measured from the device.  Figures per
scene: profiles/ba_big_graphs_accuracy.txt."""
import copy

import numpy as np
import pytest

import big_graphs as bg
from util import (HDR_M, HDR_NC1, HDR_NC2, HDR_NENT, PACKED_BAR, assert_composite_parity, assert_system_close, ba_args,
                  run_ba_stages, run_hip_ba, scaled_system_errors, sensitive_disparities, slot_classes, stage_errors,
                  stage_state_relative)

pytestmark = pytest.mark.gpu

FAR = 1000.0                        # a consumed chunk, in bars (tests/test_big_graphs.py: the oracle moves by >= 3e4)
POSE_BAR, DISP_BAR = 1e-6, 1e-5     # "same arithmetic, another dispatch" (test_hard_scene_through_the_public_entry)
TOL = 1e-4                          # tests/test_gpu_ba_full.py
HEADER = dict(M=HDR_M, nc1=HDR_NC1, nc2=HDR_NC2, nent=HDR_NENT)


def _torch():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    return torch


def _run(backends, sid, binding=None, fill="zero"):
    sc = bg.scene(sid)
    st = run_ba_stages(backends, sc.problem(), _torch(), packed=sc.packed, binding=binding, fill=fill)
    if st["status"] & 8:   # a bounded spin of the single-launch solver ran out: nothing further on this device
        pytest.exit(f"{sid} ({fill}): the solver reported a stalled grid (status {st['status']}): find the cause by reading "
                    "before anything runs again", 3)
    return st


_clean = {}


def clean(backends, sid):
    """the fill="zero" run of scene `sid` on a workspace of its own, once per session"""
    if sid not in _clean:
        _clean[sid] = _run(backends, sid)
    return _clean[sid]


def words(st):
    return {k: int(st["hdr"][w]) for k, w in HEADER.items()} | {"n3": int(st["hint"][1])}


def check(oracle, sid, st, tag=""):
    """The assertions of test_hard_scene_stages_match_oracle on the run `st` of scene `sid`, and the counts of the table."""
    sc = bg.scene(sid)
    p = sc.problem()
    got = slot_classes(st)
    err = stage_errors(oracle, p, st)
    rel = stage_state_relative(oracle, p, st)
    bar = bg.bars(sid)
    hdr, n3 = st["hdr"], st["hint"][1]
    print(f"[{sid}]{tag} classes {sorted(got, key=str)} (M={hdr[HDR_M]} nc1={hdr[HDR_NC1]} nc2={hdr[HDR_NC2]} n3={n3}) "
          f"H {err['H']:.2e} / {bar['H']:.2e}  b {err['b']:.2e} / {bar['b']:.2e}  dx {err['dx']:.2e} / {bar['dx']:.2e}  "
          f"state {max(rel):.2e} / {bar['state']:.2e} (t {rel[0]:.1e} q {rel[1]:.1e} d {rel[2]:.1e}) "
          f"stray {err['stray']} dead {err['dead']}" + (f" packed {err['packed']:.1e}/{err['packed_stray']}" if "packed" in err else ""))
    print(bg.bars_line(sid))
    assert st["status"] & 15 == 0, st["status"]
    assert st["M"] == p.eta.shape[0]
    assert got == sc.classes, (sid, got, sc.classes)
    assert n3 == sc.counts[3], (sid, n3, sc.counts)
    assert (hdr[HDR_M] - hdr[HDR_NC1] - hdr[HDR_NC2] - n3, hdr[HDR_NC1], hdr[HDR_NC2], n3) == sc.counts, (sid, words(st))
    assert_system_close(err, dict(H=bar["H"], b=bar["b"]), sid)
    if sc.packed:
        assert err["packed_stray"] == 0 and err["packed"] < PACKED_BAR, (sid, err["packed"])
    assert err["dx"] < bar["dx"], (sid, err["dx"], bar["dx"])
    assert max(rel) < bar["state"], (sid, rel, bar["state"])
    return err


def system_distance(a, b):
    """util.scaled_system_errors of system `a` against system `b` ([n + 1, n], row n = rhs)"""
    n = b.shape[1]
    return scaled_system_errors(a[:n], a[n], b[:n], b[n])


@pytest.mark.parametrize("sid", list(bg.SCENES))
def test_big_graph_stages_match_oracle(backends, oracle, sid):
    """Every stage on every scene of the two tables; hub160 and hub262 also through the packed build."""
    assert bg.scene(sid).packed == (sid in ("hub160", "hub262"))
    check(oracle, sid, clean(backends, sid))


def test_device_consumes_the_second_chunk(backends, oracle):
    """hub160 and its copy whose weights of hub 40's edges 128.. are zero: each device system matches its own oracle, and
    the two are more than FAR bars apart in H and in b (the oracle's are: tests/test_big_graphs.py) -- so the Schur
    stage and the linearisation really read the tail, with the right entries."""
    full, cut = clean(backends, "hub160"), clean(backends, "hub160_tail0")
    check(oracle, "hub160_tail0", cut)
    check(oracle, "hub160", full)
    bar = bg.bars("hub160")
    d = system_distance(cut["system"], full["system"])
    print(f"[hub160] tail of hub 40 zeroed: the device's system moves by H {d['H'] / bar['H']:.2e} b {d['b'] / bar['b']:.2e} bars")
    assert d["H"] > FAR * bar["H"] and d["b"] > FAR * bar["b"], (d, bar["H"], bar["b"])


@pytest.mark.parametrize("sid", ["hub160", "prep_global_edges"])
def test_big_graph_through_the_public_entry(backends, oracle, sid):
    """One 1-iteration backends.ba call ends in the state the phase ABI produced from the same inputs; a 2-iteration
    call matches the oracle with float32 storage the way tests/test_gpu_ba_full.py judges a composite call."""
    torch = _torch()
    p = bg.scene(sid).problem()
    st = clean(backends, sid)
    hip = run_hip_ba(backends, copy.deepcopy(p), torch, 1)
    assert hip["status"] & 15 == 0 and hip["M"] == st["M"]
    dev_p, dev_d = np.abs(hip["poses"] - st["poses"]).max(), np.abs(hip["disps"] - st["disps"]).max()
    print(f"[{sid}] backends.ba against the phase ABI: poses {dev_p:.2e} disps {dev_d:.2e}")
    assert dev_p < POSE_BAR and dev_d < DISP_BAR, (dev_p, dev_d)
    two = run_hip_ba(backends, copy.deepcopy(p), torch, 2)
    ref = oracle.ba(*ba_args(p), 2, p.lm, p.ep, False, storage_f32=True)
    assert two["status"] & 15 == 0 and two["M"] == ref["M"]
    assert_composite_parity(two, ref, TOL, f"{sid} composite x2", sensitive=lambda: sensitive_disparities(oracle, p, 2, TOL))


def test_prep_in_lds_and_in_the_workspace_agree(backends, oracle):
    """prep_lds_limit (38400 ints: ba_prep_kernel<true> at the full 150 KB) and the same graph in a buffer of one unused
    frame more (38409 ints: ba_prep_kernel<false>): the same tables, so the same header words and the same sums."""
    a, b = clean(backends, "prep_lds_limit"), clean(backends, "prep_lds_limit+1")
    check(oracle, "prep_lds_limit+1", b)
    assert words(a) == words(b), (words(a), words(b))
    d = system_distance(b["system"], a["system"])
    print(f"[prep_lds_limit] tables in LDS against tables in the workspace: H {d['H']:.1e} b {d['b']:.1e}")
    assert d["stray"] == 0 and d["dead"] == 0 and max(d["H"], d["b"]) < PACKED_BAR, d


@pytest.mark.parametrize("fill", ["ff", "history"])
@pytest.mark.parametrize("sid", bg.GLOBAL_PREP)
def test_global_prep_on_a_dirty_workspace(backends, oracle, sid, fill):
    """ba_prep_kernel<false> builds seg_ptr, cursor and xtmp in memory the previous call left behind and never writes
    slot_of[nbuf].  ff: every byte of the workspace 0xFF.  history: prep_lds_limit runs first through the same
    BaBinding (itself from 0xFF bytes), then the scene with the workspace kept.  Bars and header words as from zeros."""
    from droid_backends.ba_binding import BaBinding
    ref = clean(backends, sid)
    if fill == "ff":
        st = _run(backends, sid, fill="ff")
    else:
        lib = backends._lib.load()

        def nbytes(s):
            p = bg.scene(s).problem()
            nbuf, H, W = p.disps.shape
            return int(lib.droid_ba_workspace_bytes(len(p.ii), nbuf, H, W, p.t0, p.t1, p.eta.shape[0]))

        b = BaBinding(status_mirror=False, headroom=(1, 0))
        b.reserve(max(nbytes(sid), nbytes("prep_lds_limit")), "cuda")
        try:
            _run(backends, "prep_lds_limit", binding=b, fill="ff")
            st = _run(backends, sid, binding=b, fill="keep")
        finally:
            b.close()
    check(oracle, sid, st, f" {fill}")
    assert words(st) == words(ref), (words(st), words(ref))
    d = system_distance(st["system"], ref["system"])
    d_pose, d_disp = float(np.abs(st["poses"] - ref["poses"]).max()), float(np.abs(st["disps"] - ref["disps"]).max())
    print(f"[{sid}] {fill} against the zeroed workspace: system {max(d['H'], d['b']):.1e} poses {d_pose:.1e} disps {d_disp:.1e}")
    assert d["stray"] == 0 and d["dead"] == 0 and max(d["H"], d["b"]) < PACKED_BAR, d
    assert d_pose < POSE_BAR and d_disp < DISP_BAR, (d_pose, d_disp)
