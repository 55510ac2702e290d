"""Stage-by-stage parity of one Gauss-Newton iteration of the HIP bundle adjustment, through the phase ABI: the reduced
system droid_ba_build writes (every Schur kernel class), the packed build, the damped solve and the back-substitution +
retraction, each checked from identical inputs against the fp64 oracle -- so that an error of one stage cannot hide
behind the 1e-4 bar on the final state (an error of 1e-4 relative in S passes that bar).  The graphs and the classes each
one must exercise are in tests/stage_graphs.py; the bars per graph family are util.STAGE_BARS."""
import numpy as np
import pytest

import hard_scenes as hs
from stage_graphs import GRAPHS
from util import (HDR_M, HDR_NC1, HDR_NC2, PACKED_BAR, STAGE_BARS, assert_system_close, run_ba_stages, slot_classes,
                  stage_errors, stage_state_relative)

pytestmark = pytest.mark.gpu

# the packed build (multi-GPU path) on a sparse graph and on dense graphs with every Schur class
PACKED = {"cfg2", "cfg4", "every_class", "motion_only"}


def _torch():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    return torch


@pytest.fixture(scope="module")
def synth():
    from droid_backends import synth
    return synth


def check_graph(backends, oracle, synth, name, bars=True):
    """Runs graph `name` of the table; prints its errors and the Schur classes it covered; asserts them (bars=False:
    print only, how the bars were measured)."""
    torch = _torch()
    build, family, classes = GRAPHS[name]
    p = build(synth)
    mo = classes == {"motion"}
    st = run_ba_stages(backends, p, torch, motion_only=mo, packed=name in PACKED)
    got = slot_classes(st, mo)
    err = stage_errors(oracle, p, st, mo)
    hdr, n3 = st["hdr"], st["hint"][1]
    print(f"[{name}] classes {sorted(got, key=str)} (M={hdr[HDR_M]} nc1={hdr[HDR_NC1]} nc2={hdr[HDR_NC2]} n3={n3}) "
          f"H {err['H']:.2e} b {err['b']:.2e} dx {err['dx']:.2e} state {err['state']:.2e} "
          f"(t {err['state_parts'][0]:.1e} q {err['state_parts'][1]:.1e} d {err['state_parts'][2]:.1e}) "
          f"zero blocks {err['zero_blocks']} stray {err['stray']} dead {err['dead']}"
          + (f" packed {err['packed']:.1e}/{err['packed_stray']}" if "packed" in err else ""))
    if not bars:
        return err, got
    assert st["status"] & 15 == 0, st["status"]
    assert got == classes, (name, got, classes)
    if not mo:
        assert st["M"] == p.eta.shape[0]
    b = STAGE_BARS[family]
    assert_system_close(err, b, name)
    if "packed" in err:
        assert err["packed_stray"] == 0 and err["packed"] < PACKED_BAR, (name, err["packed"])
    assert err["dx"] < b["dx"], (name, err["dx"])
    assert err["state"] < b["state"], (name, err["state_parts"])
    return err, got


@pytest.mark.parametrize("name", list(GRAPHS))
def test_ba_stages_match_oracle(backends, oracle, synth, name):
    check_graph(backends, oracle, synth, name)


# ---------------------------------------------------------------------------------------------------------------------
# Scenes the generator never draws (tests/hard_scenes.py; proved decisive, discriminating and solvable on the CPU by
# tests/test_hard_scenes.py): anisotropic intrinsics and live observations behind MIN_DEPTH.
_hard_stages = {}


def _run_hard(backends, sid):
    """run_ba_stages of scene `sid`, once per session (the public-entry test compares against the same state)"""
    if sid not in _hard_stages:
        sc = hs.SCENES[sid]
        _hard_stages[sid] = run_ba_stages(backends, sc.problem(), _torch(), motion_only=sc.motion_only, packed=sc.packed)
    return _hard_stages[sid]


@pytest.mark.parametrize("sid", list(hs.SCENES))
def test_hard_scene_stages_match_oracle(backends, oracle, sid):
    """Every stage of one Gauss-Newton iteration on a hardened scene, against the fp64 oracle from identical inputs,
    with the bars of hard_scenes.bars (derived from the oracle's own float32 evaluation, the number formats and the
    condition of the scene; nothing measured from the device).  A kernel that reads one intrinsic for another is at
    least 100 bars away (tests/test_hard_scenes.py), and so is one whose MIN_DEPTH test is lost in the linearisation,
    the Schur stage or the back-substitution: 7 to 64 % of the live observations lie behind it.

    These scenes caught one defect: ba_schur2_kernel and ba_backsub_kernel recomputed their E
    rows from a point transformed in fp32 while the linearisation forms A, C and w from one transformed in fp64; with
    S_aa at 30 to 70 x H_aa the rounding that A does not share put H 1.3 to 1.6 bars out on win13x21-rot5-plain and
    win8x32-rot20-stereo, and the disparities of hard_variant_window_t0_3 1.55 bars out.  Both kernels now transform
    in fp64; figures per scene in profiles/ba_hard_scenes_accuracy.txt."""
    sc = hs.SCENES[sid]
    p, mo = sc.problem(), sc.motion_only
    st = _run_hard(backends, sid)
    got = slot_classes(st, mo)
    err = stage_errors(oracle, p, st, mo)
    rel = stage_state_relative(oracle, p, st, mo)
    bar = hs.bars(sid)
    hdr, n3 = st["hdr"], st["hint"][1]
    print(f"[{sid}] classes {sorted(got, key=str)} (M={hdr[HDR_M]} nc1={hdr[HDR_NC1]} nc2={hdr[HDR_NC2]} n3={n3}) "
          f"H {err['H']:.2e} / {bar['H']:.2e}  b {err['b']:.2e} / {bar['b']:.2e}  dx {err['dx']:.2e} / {bar['dx']:.2e}  "
          f"state {max(rel):.2e} / {bar['state']:.2e} (t {rel[0]:.1e} q {rel[1]:.1e} d {rel[2]:.1e}) "
          f"stray {err['stray']} dead {err['dead']}" + (f" packed {err['packed']:.1e}/{err['packed_stray']}" if "packed" in err else ""))
    print(hs.bars_line(sid))
    assert st["status"] & 15 == 0, st["status"]
    assert got == sc.classes, (sid, got, sc.classes)
    if not mo:
        assert st["M"] == p.eta.shape[0]
    assert_system_close(err, dict(H=bar["H"], b=bar["b"]), sid)
    if sc.packed:
        assert err["packed_stray"] == 0 and err["packed"] < PACKED_BAR, (sid, err["packed"])
    assert err["dx"] < bar["dx"], (sid, err["dx"], bar["dx"])
    assert max(rel) < bar["state"], (sid, rel, bar["state"])


@pytest.mark.parametrize("sid", ["win13x21-rot20-negated", "hard_every_class"])
def test_hard_scene_through_the_public_entry(backends, sid):
    """One 1-iteration backends.ba call on a hardened scene ends in the state the phase ABI produced from the same
    inputs: the same arithmetic, so this checks the dispatch (bars of the launch-hint test below)."""
    import copy
    from util import run_hip_ba
    p = hs.SCENES[sid].problem()
    st = _run_hard(backends, sid)
    hip = run_hip_ba(backends, copy.deepcopy(p), _torch(), 1)
    assert hip["status"] & 15 == 0 and hip["M"] == st["M"]
    dev_p, dev_d = np.abs(hip["poses"] - st["poses"]).max(), np.abs(hip["disps"] - st["disps"]).max()
    print(f"[{sid}] backends.ba against the phase ABI: poses {dev_p:.2e} disps {dev_d:.2e}")
    assert dev_p < 1e-6 and dev_d < 1e-5, (dev_p, dev_d)


def _sleep_cycles(torch, seconds):
    """torch.cuda._sleep argument that holds the current stream for about `seconds` (calibrated on this device)."""
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    torch.cuda._sleep(1 << 22)
    b.record()
    b.synchronize()
    ms = max(a.elapsed_time(b), 1e-3)
    return int(min((1 << 22) * seconds * 1e3 / ms, 1 << 31))


def test_launch_hint_after_workspace_growth_is_not_stale(backends, oracle, synth):
    """The words of a workspace's launch hints are re-attached when the workspace grows.  A call on the grown workspace
    whose first kernel is still queued behind other work when the host enqueues its iterations must not read the
    PREVIOUS buffer's hint ("no block-pair slots") as its own: the block-pair Schur kernel would be left out and S would
    be wrong with no status bit set.  A fresh stream (fresh workspace): a call without class-3 slots, then the stream is
    held for 0.1 s and a graph with class-3 slots that needs a bigger workspace is enqueued behind it."""
    import copy
    torch = _torch()
    from util import ba_args, compare_state, run_hip_ba, to_dev
    small = synth.make_ba_problem(N=5, E=14, H=24, W=32, seed=1)    # 2.3 MB of workspace, the graph below needs 12 MB
    big = GRAPHS["dense30_block_pair"][0](synth)
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):
        run_hip_ba(backends, copy.deepcopy(small), torch, 1)
        w = backends._workspaces[(torch.cuda.current_device(), s.cuda_stream)]
        assert int(w.mirror[4]) >= 1 and int(w.mirror[5]) == 0, (int(w.mirror[4]), int(w.mirror[5]))
        buf0 = w.buf.data_ptr()
        d = to_dev(big, torch)
        cycles = _sleep_cycles(torch, 0.1)
        torch.cuda.synchronize()
        torch.cuda._sleep(cycles)
        backends.ba(d["poses"], d["disps"], d["intrinsics"], d["disps_sens"], d["targets"], d["weights"], d["eta"],
                    d["ii"], d["jj"], big.t0, big.t1, 1, big.lm, big.ep, False)
        assert w.buf.data_ptr() != buf0          # the workspace grew: the hint words were attached to a new buffer
        torch.cuda.synchronize()
        assert backends.ba_status()[0] & 11 == 0
        assert int(w.mirror[5]) > 0              # the hint of this call has arrived by now and names class-3 slots
        hip = dict(poses=d["poses"].cpu().numpy(), disps=d["disps"].cpu().numpy(), dx=np.zeros(0))
        w.attach_hints(False)
        try:
            ref_dev = run_hip_ba(backends, copy.deepcopy(big), torch, 1)   # every launch made
        finally:
            w.attach_hints()
    ref = oracle.ba(*ba_args(big), 1, big.lm, big.ep, False, storage_f32=True)
    et, er, ed = compare_state(hip, ref, "grown workspace, stream held")
    dev_p, dev_d = np.abs(hip["poses"] - ref_dev["poses"]).max(), np.abs(hip["disps"] - ref_dev["disps"]).max()
    print(f"against the same call with the hints detached: poses {dev_p:.2e} disps {dev_d:.2e}")
    assert et < 1e-4 and er < 1e-4 and ed < 1e-4, (et, er, ed)
    assert dev_p < 1e-6 and dev_d < 1e-5, (dev_p, dev_d)
