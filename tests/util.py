"""Helpers shared by the parity tests."""
import numpy as np


def quat_angle(qa, qb):
    """Rotation angle between unit quaternions (rows), radians."""
    qa = qa / np.linalg.norm(qa, axis=-1, keepdims=True)
    qb = qb / np.linalg.norm(qb, axis=-1, keepdims=True)
    d = np.abs(np.sum(qa * qb, axis=-1)).clip(0, 1)
    return 2 * np.arccos(d)


def ba_args(p):
    return (p.poses, p.disps, p.intrinsics, p.disps_sens, p.targets, p.weights, p.eta, p.ii, p.jj, p.t0, p.t1)


def to_dev(p, torch, device="cuda"):
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(device)
    return dict(poses=t(p.poses), disps=t(p.disps), intrinsics=t(p.intrinsics), disps_sens=t(p.disps_sens),
                targets=t(p.targets), weights=t(p.weights), eta=t(p.eta), ii=t(p.ii), jj=t(p.jj))


def run_hip_ba(backends, p, torch, iterations, motion_only=False):
    d = to_dev(p, torch)
    dx, dz = backends.ba(d["poses"], d["disps"], d["intrinsics"], d["disps_sens"], d["targets"], d["weights"],
                         d["eta"], d["ii"], d["jj"], p.t0, p.t1, iterations, p.lm, p.ep, motion_only)
    torch.cuda.synchronize()
    st, m = backends.ba_status()
    return dict(poses=d["poses"].cpu().numpy(), disps=d["disps"].cpu().numpy(), dx=dx.cpu().numpy(),
                dz=dz.cpu().numpy(), status=st, M=m)


def compare_state(hip, ref, tag=""):
    """max |dt|, max rotation angle, max |ddisp| between two BA results."""
    et = np.abs(hip["poses"][:, :3] - ref["poses"][:, :3]).max()
    er = quat_angle(hip["poses"][:, 3:].astype(np.float64), ref["poses"][:, 3:].astype(np.float64)).max()
    ed = np.abs(hip["disps"] - ref["disps"]).max()
    edx = np.abs(hip["dx"] - ref["dx"]).max() if hip["dx"].size else 0.0
    print(f"[{tag}] max|dt|={et:.3e} max angle={er:.3e} max|ddisp|={ed:.3e} max|ddx|={edx:.3e}")
    return et, er, ed


def stepwise_parity(backends, oracle, p, torch, iterations, tol, tag=""):
    """PER-ITERATION parity from identical inputs, strict max-norm: iteration k of the device starts from the
    device's own float32 state after k-1 iterations, and the oracle evaluates that same iteration from the same
    state.  This is the north star's "match on identical inputs" applied to the map one Gauss-Newton iteration
    computes; a multi-iteration composite additionally carries the PROBLEM's own sensitivity (see
    `assert_composite_parity`).  Returns the device state after `iterations` iterations."""
    import copy
    q = copy.deepcopy(p)
    worst = [0.0, 0.0, 0.0]
    for k in range(iterations):
        hip = run_hip_ba(backends, q, torch, 1)
        ref = oracle.ba(*ba_args(q), 1, q.lm, q.ep, False, storage_f32=True)
        assert hip["status"] & 11 == 0 and hip["M"] == ref["M"]
        et, er, ed = compare_state(hip, ref, f"{tag} iteration {k + 1} from the device state")
        assert et < tol and er < tol and ed < tol, (tag, k, et, er, ed)
        worst = [max(a, b) for a, b in zip(worst, (et, er, ed))]
        q.poses, q.disps = hip["poses"], hip["disps"]
    return q, worst


def sensitive_disparities(oracle, p, iterations, tol, probes=2, seed=0):
    """The ill-conditioned set of a multi-iteration call, measured with the ORACLE ALONE: pixels whose result
    after `iterations` iterations moves by more than tol/4 when nothing but the float32 rounding of the state
    between iterations changes -- (a) fp64 state vs float32 state (`storage_f32`), (b) the float32 state after
    the first iteration nudged by one float32 ulp in a random direction (`probes` draws).  A weakly observed
    depth (C ~ eta, update of 100 % of its value) amplifies a 1-ulp change of the state after iteration 1 by up
    to ~1e3 in iteration 2 (cfg3 seed 12, pixel (238,1,27): 5.4e-5).  Any two float32-state evaluations (two edge
    orders on the device, the reference itself) may differ there by ~1e-4; nowhere else.  Returns a bool mask
    shaped like disps."""
    import copy
    base = oracle.ba(*ba_args(p), iterations, p.lm, p.ep, False, storage_f32=True)
    f64s = oracle.ba(*ba_args(p), iterations, p.lm, p.ep, False, storage_f32=False)
    mask = np.abs(base["disps"] - f64s["disps"]) > tol / 4
    if iterations >= 2:
        first = oracle.ba(*ba_args(p), 1, p.lm, p.ep, False, storage_f32=True)
        rng = np.random.default_rng(seed)
        for _ in range(probes):
            q = copy.deepcopy(p)
            d32 = first["disps"].astype(np.float32)
            p32 = first["poses"].astype(np.float32)
            q.disps = np.where(rng.random(d32.shape) < 0.5, np.nextafter(d32, np.float32(np.inf)),
                               np.nextafter(d32, np.float32(-np.inf))).astype(np.float32)
            q.poses = np.where(rng.random(p32.shape) < 0.5, np.nextafter(p32, np.float32(np.inf)),
                               np.nextafter(p32, np.float32(-np.inf))).astype(np.float32)
            q.poses[:p.t0] = p32[:p.t0]
            r = oracle.ba(*ba_args(q), iterations - 1, p.lm, p.ep, False, storage_f32=True)
            mask |= np.abs(r["disps"] - base["disps"]) > tol / 4
    return mask


def assert_composite_parity(hip, ref, tol, tag="", sensitive=None, hard=2e-3):
    """Composite (multi-iteration) parity: every pose and every pixel strictly within tol, EXCEPT pixels of the
    oracle-measured ill-conditioned set (`sensitive_disparities`: a mask, or a callable that computes it -- only
    called when some pixel exceeds tol), which may differ by up to `hard`.  With `sensitive` None there is no
    exception at all.  Why the set exists: two float32-state evaluations of one problem (device vs oracle with
    float32 storage, two edge orders on the device, the reference itself) round the state after iteration 1
    differently by one ulp, and a weakly observed depth amplifies that by up to ~1e3 in iteration 2; the run-to-run
    order of the device's fp64 atomics alone decides whether cfg3 seed 12 shows 6.3e-5 or 1.3e-4 at its one such
    pixel.  The outliers are printed so that drift is visible; a pixel outside the set fails the test."""
    et, er, ed = compare_state(hip, ref, tag)
    d = np.abs(hip["disps"] - ref["disps"])
    over = d > tol
    n_out = int(over.sum())
    assert et < tol and er < tol, (tag, et, er)
    if n_out == 0:
        print(f"[{tag}] disparities beyond {tol:g}: 0 of {d.size}, max {d.max():.3e}")
        return et, er, ed, 0
    assert sensitive is not None, (tag, n_out, float(d.max()))
    mask = sensitive() if callable(sensitive) else sensitive
    stray = int((over & ~mask).sum())
    where = [tuple(int(v) for v in ix) for ix in np.argwhere(over)[:8]]
    print(f"[{tag}] disparities beyond {tol:g}: {n_out} of {d.size} at {where}, {stray} outside the "
          f"ill-conditioned set ({int(mask.sum())} pixels), max {d.max():.3e}")
    assert mask.sum() <= 2e-4 * mask.size, (tag, int(mask.sum()))   # the set stays tiny
    assert stray == 0 and d.max() < hard, (tag, n_out, stray, float(d.max()))
    return et, er, ed, n_out


# ---- stage-by-stage parity of one Gauss-Newton iteration (tests/test_gpu_ba_stages.py) ------------------------------
# Words of the workspace header (csrc/ba_internal.hpp: enum HDR_*, the first thing ba_carve places in the workspace):
# depth slots, Schur entries of all slots, and the slots served by the two SYRK instances (Schur classes 1 and 2).
# tests/test_stage_checker.py parses the enum so that these stay equal to it.
HDR_M, HDR_NENT, HDR_NC1, HDR_NC2 = 1, 3, 5, 6

# Bars per graph family (tests/stage_graphs.py), set from the errors measured on the MI355X (DESIGN.md section 5,
# "stage by stage"), at most 4x the worst of them:
#   H   max |dH_ab| / sqrt(H_aa H_bb) of the lower triangle, (H_aa: the oracle's fp64 diagonal)
#   b   max |db_a| / sqrt(H_aa), relative to max |b_a| / sqrt(H_aa)
#   dx  max |dx - dx64| / max |dx64|, dx64 = fp64 solve of the device's own damped system
#   state  max over |dt|, rotation angle, |ddisp| against the oracle's back-substitution and retraction of the
#          device's own system
STAGE_BARS = {
    "sparse": dict(H=5.0e-7, b=4.4e-7, dx=1.6e-7, state=2.2e-5),
    "wide": dict(H=4.1e-7, b=2.2e-7, dx=1.3e-7, state=1.3e-5),
    "stereo": dict(H=4.8e-7, b=1.9e-7, dx=1.6e-7, state=7.3e-6),
    "dense": dict(H=5.4e-7, b=3.8e-7, dx=1.5e-7, state=2.7e-6),
    "motion": dict(H=3.4e-7, b=1.3e-7, dx=1.1e-7, state=1.1e-7),
}
PACKED_BAR = 1e-12   # build_packed + unpack vs build: the same sums in another order of the fp64 atomics


def packed_column_bases(n, nb=64):
    """Element offset of every block column of the packed system of n unknowns, and the total behind the last: the
    layout include/droid_backends_hip.h documents (block column J = rows 64 J .. n, row n = rhs, as rows of w_J doubles;
    w_J = 64, the last one n - 64 J)."""
    bases = [0]
    for J in range((n + nb - 1) // nb):
        bases.append(bases[-1] + (n + 1 - nb * J) * min(nb, n - nb * J))
    return bases


def scaled_system_errors(Hd, bd, Ho, bo):
    """Entry-wise distance of a reduced system (Hd, bd) from the reference (Ho, bo), lower triangles.  The Schur
    complement is PSD, so |H_ab| <= sqrt(H_aa H_bb): scaling by the reference's diagonal bounds every entry by 1 and
    separates a wrong kernel from fp32 noise in the well AND the weakly observed parts of the graph.  Rows whose reference
    diagonal is 0 must be exactly 0 (counted in `dead`), and so must every 6x6 block that is exactly 0 in the reference
    (`stray`: a write into the wrong slot)."""
    n = Ho.shape[0]
    Ho, Hd = np.tril(Ho), np.tril(Hd[:n, :n])
    dg = np.diag(Ho).copy()
    live = dg > 0
    si = np.where(live, 1.0 / np.sqrt(np.where(live, dg, 1.0)), 0.0)
    dead = int(np.count_nonzero(Hd[~live, :]) + np.count_nonzero(Hd[:, ~live]) + np.count_nonzero(bd[~live]))
    eh = float((np.abs(Hd - Ho) * si[:, None] * si[None, :]).max()) if n else 0.0
    P = n // 6
    tri = np.tril(np.ones((P, P), bool))
    zo = (Ho.reshape(P, 6, P, 6) == 0).all(axis=(1, 3)) & tri
    zd = (Hd.reshape(P, 6, P, 6) == 0).all(axis=(1, 3))
    bscale = max(float((np.abs(bo) * si).max()) if n else 0.0, 1e-300)
    eb = float((np.abs(bd - bo) * si).max()) / bscale if n else 0.0
    return dict(H=eh, b=eb, zero_blocks=int(zo.sum()), stray=int((zo & ~zd).sum()), dead=dead)


def assert_system_close(err, bars, tag=""):
    assert err["dead"] == 0 and err["stray"] == 0, (tag, err)
    assert err["H"] < bars["H"] and err["b"] < bars["b"], (tag, err, bars)


def damped_solve(H, b, lm, ep):
    """fp64 solve of a reduced system the way droid_ba_solve_update damps it (oracle/ba_oracle_impl.h solve_system:
    diag += ep + lm diag); lm, ep rounded to float32 like the C ABI's arguments.  H: lower triangle read."""
    lm, ep = float(np.float32(lm)), float(np.float32(ep))
    A = np.tril(H) + np.tril(H, -1).T
    A[np.diag_indices_from(A)] += ep + lm * np.diag(A)
    return np.linalg.solve(A, b)


def run_ba_stages(backends, p, torch, motion_only=False, packed=False, own=None, binding=None, fill="zero"):
    """One Gauss-Newton iteration through the phase ABI on a workspace of its own, with launch hints of its own (a
    BaBinding): droid_ba_prepare, droid_ba_build (its system copied before the solve factors it in place), optionally
    droid_ba_build_packed + droid_ba_unpack_system (copied too), droid_ba_solve_update.  Returns the copies, the
    state after the update, dx, dz, the header words and the hint words {tag, slots of Schur class 3}.
    own: the frame range handed to droid_ba_prepare (default: the whole buffer, a single GPU).
    binding: a BaBinding the caller owns (not closed here), already reserved to at least the bytes this problem needs,
    so that several runs share one workspace (tests/test_gpu_workspace_history.py); default: one of its own.
    fill: what happens to the workspace before droid_ba_prepare -- "zero": zeroed (the default), "ff": every byte 0xFF
    (NaN as fp32 and fp64, -1 as an int), "keep": left as the previous run through `binding` left it."""
    from droid_backends.ba_binding import BAProblemDev, BaBinding
    assert fill in ("zero", "ff", "keep"), fill
    d = BAProblemDev(**to_dev(p, torch))
    # default: a zeroed workspace of exactly the size asked for
    b = BaBinding(status_mirror=False, headroom=(1, 0)) if binding is None else binding
    E, nbuf, H, W, M, t0, t1 = b.begin(d, p.t0, p.t1, motion_only)
    if fill == "zero":
        b.buf.zero_()
    elif fill == "ff":
        b.buf.fill_(0xFF)
    n = 6 * (t1 - t0)
    dx = torch.zeros((t1 - t0, 6), dtype=torch.float32, device="cuda")
    dz = torch.zeros((max(M, 1), H * W), dtype=torch.float32, device="cuda")
    system = lambda: b.system().view(n + 1, -1)[:, :n].cpu().numpy().copy()
    try:
        b.prepare(d, (0, nbuf) if own is None else own, motion_only)
        b.build(d, motion_only)
        torch.cuda.synchronize()
        hw = b.HINT_WORD
        out = dict(system=system(), hdr=b.header(), hint=(int(b.mirror[hw]), int(b.mirror[hw + 1])))
        if packed:
            b.build(d, motion_only, packed=True)
            b.unpack_system(motion_only)
            torch.cuda.synchronize()
            out["system_packed"] = system()
        b.solve_update(d, p.lm, p.ep, motion_only, dx, dz)
        torch.cuda.synchronize()
        st, m = b.status()
    finally:
        if binding is None:
            b.close()
    out.update(status=st, M=m, dx=dx.cpu().numpy(), dz=dz.cpu().numpy()[:M], poses=d.poses.cpu().numpy(),
               disps=d.disps.cpu().numpy())
    return out


def shard_of(p, ranges, rank):
    """The arrays rank `rank` of `ranges` holds, as a problem of its own (ba_driver.shard_problem): its edges and eta
    rows, the replicated state; `.own` = its frame range."""
    import copy
    from droid_backends import ba_driver
    sh = ba_driver.shard_problem(p, ranges, rank)
    q = copy.copy(p)
    q.targets, q.weights, q.eta, q.ii, q.jj = sh["targets"], sh["weights"], sh["eta"], sh["ii"], sh["jj"]
    q.own = tuple(int(x) for x in sh["own"])
    return q


def run_shard_stages(backends, p, ranges, torch, motion_only=False):
    """One Gauss-Newton iteration of every shard of `p` (ranges: [(f0, f1)] per rank), the way the ranks of an
    edge-sharded call run it, in one process: per rank a zeroed workspace of its own (a BaBinding), droid_ba_prepare
    with its range, droid_ba_build and droid_ba_build_packed + droid_ba_unpack_system, each system copied before
    anything factors it; the packed tensors are summed on the device in rank order (what the all-reduce does); every
    rank copies the sum in, unpacks it (copied: the system it solves) and runs droid_ba_solve_update.
    Returns per rank: shard (shard_of), own, system, system_packed, packed, system_sum, hdr, hint, status, M, dx, dz,
    poses, disps."""
    from droid_backends.ba_binding import BAProblemDev, BaBinding
    n = 6 * (p.t1 - p.t0)
    ranks = []
    try:
        for r in range(len(ranges)):
            q = shard_of(p, ranges, r)
            d = BAProblemDev(**to_dev(q, torch))
            b = BaBinding(status_mirror=False, headroom=(1, 0))     # a zeroed workspace of exactly the size asked for
            ranks.append((q, d, b))
            E, nbuf, H, W, M, t0, t1 = b.begin(d, p.t0, p.t1, motion_only)
            b.buf.zero_()
        outs = []
        total = None
        for q, d, b in ranks:
            system = lambda b=b: b.system().view(n + 1, -1)[:, :n].cpu().numpy().copy()
            b.prepare(d, q.own, motion_only)
            b.build(d, motion_only)
            torch.cuda.synchronize()
            hw = b.HINT_WORD
            out = dict(shard=q, own=q.own, system=system(), hdr=b.header(),
                       hint=(int(b.mirror[hw]), int(b.mirror[hw + 1])))
            b.build(d, motion_only, packed=True)
            packed = b.packed().clone()
            b.unpack_system(motion_only)
            torch.cuda.synchronize()
            out.update(system_packed=system(), packed=packed.cpu().numpy())
            total = packed if total is None else total + packed
            outs.append(out)
        for (q, d, b), out in zip(ranks, outs):
            M, HW = b.dims[4], b.dims[2] * b.dims[3]
            dx = torch.zeros((p.t1 - p.t0, 6), dtype=torch.float32, device="cuda")
            dz = torch.zeros((max(M, 1), HW), dtype=torch.float32, device="cuda")
            b.packed().copy_(total)
            b.unpack_system(motion_only)
            torch.cuda.synchronize()
            out["system_sum"] = b.system().view(n + 1, -1)[:, :n].cpu().numpy().copy()
            b.solve_update(d, p.lm, p.ep, motion_only, dx, dz)
            torch.cuda.synchronize()
            st, m = b.status()
            out.update(status=st, M=m, dx=dx.cpu().numpy(), dz=dz.cpu().numpy()[:M], poses=d.poses.cpu().numpy(),
                       disps=d.disps.cpu().numpy())
    finally:
        for _, _, b in ranks:
            b.close()
    return outs


def slot_classes(stages, motion_only=False):
    """Schur classes the device served, from the header words and the hint words run_ba_stages read."""
    hdr, (tag, n3) = stages["hdr"], stages["hint"]
    if motion_only:
        return {"motion"} if hdr[HDR_M] == 0 else {"slots?"}
    assert tag != 0, "the launch hint of the prepare has not arrived after a synchronisation"
    counts = (hdr[HDR_M] - hdr[HDR_NC1] - hdr[HDR_NC2] - n3, hdr[HDR_NC1], hdr[HDR_NC2], n3)
    assert min(counts) >= 0, counts
    return {c for c, k in enumerate(counts) if k > 0}


def stage_errors(oracle, p, stages, motion_only=False, own=None, solved=None):
    """Errors of every stage of `stages` (run_ba_stages) against the oracle from the same inputs:
    build (scaled entry-wise, zero blocks), packed build vs build, solve (dx vs an fp64 solve of the device's own
    system) and back-substitution + retraction (the oracle's, applied to the device's own system).
    A shard (run_shard_stages): `p` holds the rank's own arrays, `own` its frame range -- the oracle then builds that
    rank's partial system and keeps that rank's depth slots -- and `solved` is the system the rank factored, the sum
    over the ranks ([n + 1, n], row n = rhs), which the solve and the back-substitution are judged on."""
    nbuf = p.disps.shape[0]
    own = (0, nbuf) if own is None else own
    ph = oracle.BAPhases()
    Ho, bo = ph.build(*ba_args(p), int(own[0]), int(own[1]), motion_only)
    sysd = stages["system"]
    n = Ho.shape[0]
    Hd, bd = sysd[:n], sysd[n]
    err = scaled_system_errors(Hd, bd, Ho, bo)
    if "system_packed" in stages:
        sp = stages["system_packed"]
        e = scaled_system_errors(sp[:n], sp[n], Hd, bd)
        err["packed"] = max(e["H"], e["b"])
        err["packed_stray"] = e["stray"] + e["dead"]
    if solved is not None:
        Hd, bd = solved[:n], solved[n]
    x = damped_solve(Hd, bd, p.lm, p.ep)
    err["dx"] = float(np.abs(stages["dx"].reshape(-1) - x).max() / max(np.abs(x).max(), 1e-300))
    lm, ep = float(np.float32(p.lm)), float(np.float32(p.ep))
    poses, disps, _ = ph.finish(np.tril(Hd) + np.tril(Hd, -1).T, bd, lm, ep)
    et = float(np.abs(stages["poses"][:, :3] - poses[:, :3]).max())
    er = float(quat_angle(stages["poses"][:, 3:].astype(np.float64), poses[:, 3:]).max())
    ed = float(np.abs(stages["disps"] - disps).max())
    err["state"] = max(et, er, ed)
    err["state_parts"] = (et, er, ed)
    return err


def relative_state_error(p, got, ref):
    """(translation, rotation, disparity) distance of the state `got` = (poses, disps) from `ref`, both one update of
    the state of `p`, for scenes whose update is not small (tests/hard_scenes.py: a disparity may move by 10, where
    the absolute |ddisp| of STAGE_BARS says nothing): per pixel |ddisp| / (|disp before| + |dz of ref|), per frame
    ||dt|| / (||t before|| + ||step of ref||), and the rotation angle as it is.  A pixel or frame that `ref` leaves at
    0 with a step of 0 has to be 0 in `got` as well (it counts as 1 otherwise)."""
    p0, d0 = np.asarray(p.poses, np.float64), np.asarray(p.disps, np.float64)
    gp, gd = (np.asarray(a, np.float64) for a in got)
    rp, rd = (np.asarray(a, np.float64) for a in ref)

    def rel(num, den):
        return float(np.where(num == 0, 0.0, np.where(den > 0, num / np.where(den > 0, den, 1.0), 1.0)).max())

    n = np.linalg.norm
    et = rel(n(gp[:, :3] - rp[:, :3], axis=1), n(p0[:, :3], axis=1) + n(rp[:, :3] - p0[:, :3], axis=1))
    er = float(quat_angle(gp[:, 3:], rp[:, 3:]).max())
    ed = rel(np.abs(gd - rd), np.abs(d0) + np.abs(rd - d0))
    return et, er, ed


def stage_state_relative(oracle, p, stages, motion_only=False):
    """relative_state_error of the state `stages` (run_ba_stages) ends in, against the oracle's fp64 solve,
    back-substitution and retraction of the device's own system -- the comparison of stage_errors, in the metric for
    scenes whose update is large."""
    nbuf = p.disps.shape[0]
    ph = oracle.BAPhases()
    ph.build(*ba_args(p), 0, nbuf, motion_only)
    n = 6 * (p.t1 - p.t0)
    Hd, bd = stages["system"][:n], stages["system"][n]
    lm, ep = float(np.float32(p.lm)), float(np.float32(p.ep))
    poses, disps, _ = ph.finish(np.tril(Hd) + np.tril(Hd, -1).T, bd, lm, ep)
    return relative_state_error(p, (stages["poses"], stages["disps"]), (poses, disps))
