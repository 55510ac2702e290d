"""Writes tests/golden/reference_{geom,ba,ba_blocks,corr,upsample}.npz: outputs of the reference's own Python programs
(geom/projective_ops.py, geom/ba.py with geom/chol.py, modules/corr.py, droid_net.py), run unchanged on the CPU in
float64, single-threaded, on the inputs of tests/reference_cases.py (float32 arrays widened to float64; quaternions
normalised there, see reference_cases.unit_poses).  Needs a
checkout of the reference (tests/reference_programs.py: DROID_REFERENCE_DIR); the fixtures are all the tests need.

    python tests/golden/make_reference_golden.py

Each file holds the reference's arrays and the SHA-256 of the inputs they were computed from.  Two runs write identical
files (fixed member order and time stamps).  tests/test_reference_pin.py recomputes everything below where the checkout
exists and compares it with the committed files.

What the reference is given that the device is not: `eta - 1e-7`, because geom/ba.py:92 adds 1e-7 itself where the CUDA
path's caller has added it already (factor_graph.py: `.2 * damping + 1e-7`).
"""
import io
import os
import sys
import zipfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
TESTS = os.path.dirname(HERE)
ROOT = os.path.dirname(TESTS)
for _p in (TESTS, ROOT, os.path.join(ROOT, "droid-slam_reserch_amd")):
    if _p not in sys.path:
        sys.path.insert(0, _p)

import cvx_upsample_ref as cu            # noqa: E402
import reference_cases as rc             # noqa: E402
import reference_programs as rp          # noqa: E402


CUDA_MIN_DEPTH = 0.25        # src/droid_kernels.cu:26


def _t(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(np.asarray(a, np.float64)))


def _ix(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(np.asarray(a, np.int64)))


def _sha(s):
    return np.array(s)


class _Depths:
    """wraps pops.actp for the time of a block: keeps Z of the transformed points (the quantity valid is decided on)"""

    def __init__(self, ref):
        self.ref, self.Z = ref, None

    def __enter__(self):
        self.actp0 = self.ref.pops.actp

        def actp(Gij, X0, jacobian=False):
            X1, Ja = self.actp0(Gij, X0, jacobian=jacobian)
            self.Z = X1[0, ..., 2].numpy().copy()
            return X1, Ja

        self.ref.pops.actp = actp
        return self

    def __exit__(self, *exc):
        self.ref.pops.actp = self.actp0


def project(ref, c, jacobian=False):
    """pops.projective_transform on a case of reference_cases.geom_cases: coords [E,H,W,2], valid [E,H,W], Z [E,H,W],
    and with `jacobian` Ji, Jj [E,H,W,2,6], Jz [E,H,W,2] (numpy float64)."""
    n = c["disps"].shape[0]
    K = _t(np.broadcast_to(c["K"], (n, 4)))[None]
    with _Depths(ref) as d:
        out = ref.pops.projective_transform(ref.SE3(_t(rc.unit_poses(c["poses"]))[None]), _t(c["disps"])[None], K, _ix(c["ii"]),
                                            _ix(c["jj"]), jacobian=jacobian)
    res = dict(coords=out[0][0].numpy(), valid=out[1][0, ..., 0].numpy(), Z=d.Z)
    if jacobian:
        Ji, Jj, Jz = out[2]
        res.update(Ji=Ji[0].numpy(), Jj=Jj[0].numpy(), Jz=Jz[0, ..., 0].numpy())
    return res


def compute_geom(ref):
    out = {}
    for name, c in rc.geom_cases().items():
        r = project(ref, c, jacobian=(name == "mono"))
        out[f"{name}_coords"] = r["coords"]
        out[f"{name}_valid"] = r["valid"].astype(np.uint8)
        out[f"{name}_Z"] = r["Z"]
        out[f"{name}_sha"] = _sha(rc.geom_digest(c))
        if name == "mono":
            E, H, W = r["Z"].shape
            s = rc.jac_sample(name, E, H * W)
            out["mono_Ji"] = r["Ji"].reshape(E * H * W, 2, 6)[s]
            out["mono_Jj"] = r["Jj"].reshape(E * H * W, 2, 6)[s]
            out["mono_Jz"] = r["Jz"].reshape(E * H * W, 2)[s]
    return out


def ba_inputs(ref, p):
    """a BAProblem as the arguments of geom.ba.BA / MoBA (batch of one, float64)"""
    n = p.disps.shape[0]
    return dict(target=_t(p.targets).permute(0, 2, 3, 1)[None].contiguous(),
                weight=_t(p.weights).permute(0, 2, 3, 1)[None].contiguous(),
                eta=_t(p.eta) - 1e-7, poses=ref.SE3(_t(rc.unit_poses(p.poses))[None]), disps=_t(p.disps)[None],
                intrinsics=_t(np.broadcast_to(p.intrinsics, (n, 4)))[None], ii=_ix(p.ii), jj=_ix(p.jj), fixedp=p.t0)


def _dense(H):
    """[1,P,Q,D,X] blocks -> [P*D, Q*X]"""
    _, P, Q, D, X = H.shape
    return H[0].permute(0, 2, 1, 3).reshape(P * D, Q * X).numpy()


def ba_system(ref, p, motion_only):
    """One linearisation of graph `p` by geom.ba.BA (MoBA): the per-edge blocks Hs [E,4,6,6] (Hii Hij Hji Hjj), vs
    [E,2,6], the scattered H [6P,6P], v, and for BA E [6P, M HW], C (eta included), w [M HW] and the reference's own
    undamped reduced system S, b; rule: how many observations with a weight lie behind the CUDA path's MIN_DEPTH, and the
    smallest distance of one from it."""
    a = ba_inputs(ref, p)
    # the CUDA path drops an observation whose depth is below 0.25 (dk:26), geom/ba.py one below 0.2: the rule is carried
    # over by handing the reference weights that are 0 where ITS depth is below 0.25
    Z = project(ref, dict(poses=p.poses, disps=p.disps, K=p.intrinsics, ii=p.ii, jj=p.jj))["Z"]
    live = (p.weights > 0).any(axis=1)
    a["weight"] = a["weight"] * _t(Z >= CUDA_MIN_DEPTH)[None, ..., None]
    rule = np.array([float((live & (Z < CUDA_MIN_DEPTH)).sum()), np.abs(Z - CUDA_MIN_DEPTH)[live].min()])
    with rp.spied(ref) as rec:
        if motion_only:
            ref.ba.MoBA(a["target"], a["weight"], a["eta"], a["poses"], a["disps"], a["intrinsics"], a["ii"], a["jj"],
                        fixedp=a["fixedp"])
        else:
            ref.ba.BA(a["target"], a["weight"], a["eta"], a["poses"], a["disps"], a["intrinsics"], a["ii"], a["jj"],
                      fixedp=a["fixedp"])
    out = dict(Hs=np.stack([rec.mat[k][0][0].numpy() for k in range(4)], axis=1),
               vs=np.stack([rec.vec[k][0][0].numpy() for k in range(2)], axis=1), rule=rule)
    if motion_only:
        out.update(H=_dense(rec.block["H"]), v=rec.block["v"][0].reshape(-1).numpy())
        return out
    s = rec.schur
    out.update(H=_dense(s["H"]), E=_dense(s["E"]), C=s["C"][0].reshape(-1).numpy(), v=s["v"][0].reshape(-1).numpy(),
               w=s["w"][0].reshape(-1).numpy(), S=s["S"][0].numpy(), b=s["b"][0, :, 0].numpy(),
               Ei=rec.mat[4][0][0].numpy(), Ej=rec.mat[5][0][0].numpy(), Ck=rec.vec[2][0][0].numpy(),
               wk=rec.vec[3][0][0].numpy())
    return out


def compute_ba(ref):
    """(reference_ba, reference_ba_blocks)"""
    out, blocks = {}, {}
    for name, (_, _, motion_only, _) in rc.BA_GRAPHS.items():
        p = rc.ba_problem(name)
        r = ba_system(ref, p, motion_only)
        sha = _sha(rc.ba_digest(p))
        out[f"{name}_sha"] = sha
        out[f"{name}_rule"] = r["rule"]
        S, b = (r["H"], r["v"]) if motion_only else (r["S"], r["b"])
        assert np.abs(S - S.T).max() <= 1e-12 * np.abs(S).max(), name
        out[f"{name}_S"] = rc.tril_pack(S)
        out[f"{name}_b"] = b
        if name in rc.EDGE_BLOCKS:
            out[f"{name}_Hs"], out[f"{name}_vs"] = r["Hs"], r["vs"]
        if name in rc.FULL_BLOCKS:
            blocks[f"{name}_sha"] = sha
            blocks[f"{name}_H"] = rc.tril_pack(r["H"])
            for k in ("E", "C", "v", "w"):
                blocks[f"{name}_{k}"] = r[k]
    return out, blocks


def compute_corr(ref):
    import torch
    s = rc.CORR_SHAPE
    f = torch.from_numpy(rc.corr_fmaps().astype(np.float64))
    ii, jj = (_ix(x) for x in rc.CORR_EDGES)
    f1, f2 = f[ii][None], f[jj][None]
    vol = ref.corr.CorrBlock.corr(f1, f2)
    blk = ref.corr.CorrBlock(f1, f2, num_levels=s["levels"])
    assert torch.equal(vol[0], blk.corr_pyramid[0])
    rows = _ix(rc.corr_rows())
    out = dict(sha=_sha(rc.digest(rc.corr_fmaps(), *rc.CORR_EDGES)))
    for l, lvl in enumerate(blk.corr_pyramid):
        E, h, w, h2, w2 = lvl.shape
        out[f"volume_l{l}"] = lvl.reshape(E, h * w, h2, w2)[:, rows].numpy()
    alt = ref.corr.AltCorrBlock(f[None], num_levels=s["levels"])
    for l, lvl in enumerate(alt.pyramid):
        out[f"alt_l{l}"] = lvl[0][_ix(rc.ALT_FRAMES)].numpy()
    return out


def compute_upsample(ref):
    import torch
    out = {}
    for case, sigma in rc.up_cases():
        p = cu.problem(case, sigma)
        n, H, W = p["data"].shape
        data, mask = _t(p["data"]), _t(p["mask16"])
        up = ref.droid_net.upsample_disp(data[None], mask[None])
        assert tuple(up.shape) == (1, n, 8 * H, 8 * W)
        key = rc.up_key(case, sigma)
        s = _ix(rc.up_sample(case, sigma))
        out[f"disp_{key}"] = up.reshape(-1)[s].numpy()
        out[f"sha_{key}"] = _sha(rc.digest(p["data"], p["mask16"]))
        if sigma == cu.SIGMAS[0] and n * H * W <= 256:
            cvx = ref.droid_net.cvx_upsample(data.view(n, H, W, 1), mask)
            assert tuple(cvx.shape) == (n, 8 * H, 8 * W, 1)
            out[f"cvx_{key}"] = cvx.reshape(-1)[s].numpy()
    return out


def compute_all():
    """name of the fixture -> dict of arrays; float64, one thread"""
    import torch
    threads = torch.get_num_threads()
    torch.set_num_threads(1)
    try:
        with rp.loaded() as ref, torch.no_grad():
            ba, blocks = compute_ba(ref)
            return dict(geom=compute_geom(ref), ba=ba, ba_blocks=blocks, corr=compute_corr(ref),
                        upsample=compute_upsample(ref))
    finally:
        torch.set_num_threads(threads)


def write_npz(path, arrays):
    """an .npz np.load reads, byte-identical for identical arrays: sorted members, a fixed time stamp"""
    with zipfile.ZipFile(path, "w", zipfile.ZIP_DEFLATED, compresslevel=9) as z:
        for k in sorted(arrays):
            buf = io.BytesIO()
            a = np.asarray(arrays[k])
            np.lib.format.write_array(buf, a if a.ndim == 0 else np.ascontiguousarray(a), allow_pickle=False)
            info = zipfile.ZipInfo(k + ".npy", date_time=(1980, 1, 1, 0, 0, 0))
            info.compress_type = zipfile.ZIP_DEFLATED
            info.external_attr = 0o644 << 16
            z.writestr(info, buf.getvalue(), compresslevel=9)


def main():
    if not rp.available():
        sys.exit(rp.SKIP_REASON)
    for name, arrays in compute_all().items():
        write_npz(rc.path(name), arrays)
        size = os.path.getsize(rc.path(name))
        print(f"{os.path.basename(rc.path(name))}: {len(arrays)} arrays, {size} bytes")
        assert size <= rc.MAX_BYTES, (name, size)


if __name__ == "__main__":
    main()
