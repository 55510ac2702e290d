"""Stage-by-stage parity of one Gauss-Newton iteration of every SHARD of an edge-sharded bundle adjustment: the device
code that acts on own0/own1 (slot table, partial system, packed build, back-substitution of the rank's own slots), each
stage against the fp64 oracle's evaluation of that same shard -- oracle.BAPhases.build(shard, own0, own1) -- from identical
inputs.  tests/test_gpu_sharded.py holds the end-to-end runs (final state to 1e-4); an error of 1e-4 relative in one
rank's S passes those.  The cases and what makes each decisive: tests/shard_cases.py, pinned on the CPU by
tests/test_shard_cases.py.  The figures measured on the MI355X: profiles/ba_shard_stages_accuracy.txt."""
import numpy as np
import pytest

import shard_cases as sc
from util import (HDR_M, PACKED_BAR, STAGE_BARS, assert_system_close, ba_args, quat_angle, run_shard_stages,
                  scaled_system_errors, slot_classes, stage_errors)

pytestmark = pytest.mark.gpu


def _torch():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    return torch


def check_case(backends, oracle, name):
    """Runs every shard of case `name`; prints one line per rank (the lines of profiles/ba_shard_stages_accuracy.txt);
    asserts every check of the shard-aware stage checker."""
    torch = _torch()
    case = sc.CASES[name]
    mo = case.motion_only
    fam = STAGE_BARS[case.family]
    p, ranges, _ = sc.shards(case)
    outs = run_shard_stages(backends, p, ranges, torch, mo)
    n, nbuf = 6 * (p.t1 - p.t0), p.disps.shape[0]
    lm, ep = float(np.float32(p.lm)), float(np.float32(p.ep))

    # the system every rank solved: the packed tensors summed on the device in rank order, unpacked -- bit for bit the
    # sum of the ranks' unpacked packed systems, and the same on every rank
    solved = outs[0]["system_sum"]
    acc = np.zeros_like(solved)
    for o in outs:
        acc += o["system_packed"]
    low = np.tril(np.ones((n, n), bool))
    assert np.array_equal(acc[:n][low], solved[:n][low]) and np.array_equal(acc[n], solved[n]), name
    for o in outs[1:]:
        assert np.array_equal(o["system_sum"][:n][low], solved[:n][low]) and np.array_equal(o["system_sum"][n], solved[n])

    failures = []
    for r, o in enumerate(outs):
        q = o["shard"]
        slots = sc.slot_frames(q, p)[:0] if mo else sc.slot_frames(q, p)    # motion-only: no depth slot anywhere
        ref = oracle.BAPhases("f64").build(*ba_args(q), q.own[0], q.own[1], mo)
        bars, e32, source = sc.shard_bars(oracle, q, case.family, mo, case.f32_room, ref=ref)
        err = stage_errors(oracle, q, o, mo, own=q.own, solved=solved)
        got = slot_classes(o, mo)
        moved = sc.untouched_frames(p.disps, o["disps"], slots)
        print(f"shard_stage {name} rank {r} own {q.own} E {len(q.ii)} M {o['M']} classes {sorted(got, key=str)} "
              f"H {err['H']:.2e} / {bars['H']:.2e} ({source['H']}) b {err['b']:.2e} / {bars['b']:.2e} ({source['b']}) "
              f"f32-oracle H {e32['H']:.2e} b {e32['b']:.2e} packed {err['packed']:.1e}/{err['packed_stray']} "
              f"dx {err['dx']:.2e} / {fam['dx']:.2e} state {err['state']:.2e} / {fam['state']:.2e} "
              f"stray {err['stray']} dead {err['dead']} foreign maps written {len(moved)}")
        try:
            # slots
            assert o["status"] & 15 == 0, o["status"]
            assert o["M"] == o["hdr"][HDR_M] == len(slots), (o["M"], o["hdr"][HDR_M], len(slots))
            # partial system, packed against pitched
            assert_system_close(err, bars, f"{name} rank {r}")
            assert err["packed_stray"] == 0 and err["packed"] < PACKED_BAR, err["packed"]
            # solve of the summed system; back-substitution of this rank's slots and retraction
            assert err["dx"] < fam["dx"], err["dx"]
            assert err["state"] < fam["state"], err["state_parts"]
            assert np.array_equal(o["dx"], outs[0]["dx"]) and np.array_equal(o["poses"], outs[0]["poses"])
            assert moved == [], moved
            if case.classes is not None:
                assert got == case.classes[r], (got, case.classes[r])
        except AssertionError as e:   # every rank is printed before the case fails
            failures.append((name, r, e))

    # the partial systems, summed in fp64, are the unsharded system
    total = np.zeros_like(solved)
    for o in outs:
        total += o["system"]
    ph = oracle.BAPhases("f64")
    Ho, bo = ph.build(*ba_args(p), 0, nbuf, mo)
    e = scaled_system_errors(total[:n], total[n], Ho, bo)
    # the owners' maps, stitched together, are the unsharded back-substitution of the solved system
    disps = np.array(p.disps, copy=True)
    for (f0, f1), o in zip(ranges, outs):
        disps[f0:f1] = o["disps"][f0:f1]
    rp, rd, _ = ph.finish(np.tril(solved[:n]) + np.tril(solved[:n], -1).T, solved[n], lm, ep)
    poses = outs[0]["poses"]
    state = max(float(np.abs(poses[:, :3] - rp[:, :3]).max()),
                float(quat_angle(poses[:, 3:].astype(np.float64), rp[:, 3:]).max()), float(np.abs(disps - rd).max()))
    print(f"shard_stage {name} sum of {len(outs)} ranks: H {e['H']:.2e} / {fam['H']:.2e} b {e['b']:.2e} / {fam['b']:.2e} "
          f"stray {e['stray']} dead {e['dead']} stitched state {state:.2e} / {fam['state']:.2e}")
    assert not failures, failures
    assert_system_close(e, fam, f"{name} sum")
    assert state < fam["state"], (name, state)
    return outs


@pytest.mark.parametrize("name", list(sc.CASES))
def test_shard_stages_match_oracle(backends, oracle, name):
    check_case(backends, oracle, name)
