"""Loads the reference's own Python programs -- droid_slam/geom/projective_ops.py, geom/ba.py, geom/chol.py,
modules/corr.py, droid_net.py -- unchanged, on the CPU, with the stand-ins of tests/refshim/ for the two packages they
need and this machine does not have (lietorch, torch_scatter).  Test infrastructure: the generator of the
tests/golden/reference_*.npz fixtures (tests/golden/make_reference_golden.py) and tests/test_reference_pin.py use it;
nothing that runs on the GPU does, the fixtures are all those tests read.

The checkout is found through the environment variable DROID_REFERENCE_DIR (default: /root/reference, where it lies on
the development machine).  Where it is absent `available()` is False and callers skip with `SKIP_REASON`.

    with reference_programs.loaded() as ref:
        coords, valid = ref.pops.projective_transform(ref.SE3(poses), disps, K, ii, jj)

Inside the block sys.path starts with the stand-ins and the checkout's droid_slam/, and torch.as_tensor ignores a
`device` argument (projective_ops.py:105 builds the stereo baseline on "cuda"; a Python list becomes float64 there, so
that the baseline is -0.1 and not float32(-0.1)).  On exit sys.path and torch.as_tensor are restored and the stand-ins
and every module imported from the checkout are removed from sys.modules: no other test sees a fake lietorch.
`modules/corr.py` imports `droid_backends`; that resolves to the product package, of which CorrBlock.corr and the two
pyramid builders call nothing.
"""
import contextlib
import importlib
import os
import sys
import types
import warnings

HERE = os.path.dirname(os.path.abspath(__file__))
SHIM_DIR = os.path.join(HERE, "refshim")
REFERENCE_DIR = os.environ.get("DROID_REFERENCE_DIR", "/root/reference")
PROGRAMS = ("geom.projective_ops", "geom.chol", "geom.ba", "modules.corr", "droid_net")
SKIP_REASON = f"no checkout of the reference under DROID_REFERENCE_DIR={REFERENCE_DIR}"
BA_SPIED = ("schur_solve", "block_solve", "safe_scatter_add_mat", "safe_scatter_add_vec")


def source_dir():
    return os.path.join(REFERENCE_DIR, "droid_slam")


def available():
    return all(os.path.isfile(os.path.join(source_dir(), *m.split(".")) + ".py") for m in PROGRAMS)


def _under(path, root):
    path, root = os.path.realpath(path), os.path.realpath(root)
    return path == root or path.startswith(root + os.sep)


def _foreign(mod):
    f = getattr(mod, "__file__", None)
    if f is not None:
        return _under(f, SHIM_DIR) or _under(f, REFERENCE_DIR)
    return any(_under(p, SHIM_DIR) or _under(p, REFERENCE_DIR) for p in list(getattr(mod, "__path__", [])))


@contextlib.contextmanager
def loaded():
    """The programs, imported for the time of the block: a namespace with pops, chol, ba, corr, droid_net, SE3."""
    import torch
    if not available():
        raise FileNotFoundError(SKIP_REASON)
    path0, as_tensor0 = list(sys.path), torch.as_tensor

    def as_tensor(data, dtype=None, device=None):
        if dtype is None and isinstance(data, (list, tuple)):
            dtype = torch.float64
        return as_tensor0(data, dtype=dtype)

    clash = [m for m in ("lietorch", "torch_scatter", "geom", "modules", "droid_net", "data_readers") if m in sys.modules]
    assert not clash, f"already imported, would shadow the reference's modules: {clash}"
    sys.path[:0] = [SHIM_DIR, source_dir()]
    torch.as_tensor = as_tensor
    try:
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")        # torch.meshgrid without `indexing`, as the reference calls it
            mods = {m: importlib.import_module(m) for m in PROGRAMS}
            import lietorch
            assert _under(lietorch.__file__, SHIM_DIR)
            yield types.SimpleNamespace(pops=mods["geom.projective_ops"], chol=mods["geom.chol"], ba=mods["geom.ba"],
                                        corr=mods["modules.corr"], droid_net=mods["droid_net"], SE3=lietorch.SE3)
    finally:
        torch.as_tensor = as_tensor0
        sys.path[:] = path0
        for name in [n for n, m in list(sys.modules.items()) if m is not None and _foreign(m)]:
            del sys.modules[name]
        importlib.invalidate_caches()


@contextlib.contextmanager
def spied(ref):
    """Rebinds the module-level names BA_SPIED of geom.ba (and CholeskySolver of geom.chol) for the time of the block.
    The yielded record collects, in call order:
      mat    (A, ii, jj, n, m) of every safe_scatter_add_mat: Hii, Hij, Hji, Hjj, then Ei, Ej (BA only)
      vec    (b, ii, n) of every safe_scatter_add_vec: vi, vj, then Ck, wk (BA only)
      schur  H, E, C, v, w as BA hands them to schur_solve, and S, b: what the reference's own schur_solve hands to its
             Cholesky solver when called with ep = lm = 0 (the undamped reduced system)
      block  H, v as MoBA hands them to block_solve
    The solves themselves return zeros: the programs run to their end, their updates are not used."""
    import torch
    ba, chol = ref.ba, ref.chol
    saved = {n: getattr(ba, n) for n in BA_SPIED}
    solver0 = chol.CholeskySolver
    rec = types.SimpleNamespace(mat=[], vec=[], schur=None, block=None)

    class Recorder:
        seen = None

        @staticmethod
        def apply(S, b):
            Recorder.seen = (S.clone(), b.clone())
            return torch.zeros_like(b)

    def mat(A, ii, jj, n, m):
        rec.mat.append((A.clone(), ii.clone(), jj.clone(), n, m))
        return saved["safe_scatter_add_mat"](A, ii, jj, n, m)

    def vec(b, ii, n):
        rec.vec.append((b.clone(), ii.clone(), n))
        return saved["safe_scatter_add_vec"](b, ii, n)

    def schur_solve(H, E, C, v, w, **kw):
        dx, dz = saved["schur_solve"](H, E, C, v, w, ep=0.0, lm=0.0)
        S, b = Recorder.seen
        rec.schur = dict(H=H.clone(), E=E.clone(), C=C.clone(), v=v.clone(), w=w.clone(), S=S, b=b)
        return dx, dz

    def block_solve(H, v, **kw):
        rec.block = dict(H=H.clone(), v=v.clone())
        return torch.zeros_like(v)

    ba.safe_scatter_add_mat, ba.safe_scatter_add_vec = mat, vec
    ba.schur_solve, ba.block_solve = schur_solve, block_solve
    chol.CholeskySolver = Recorder
    try:
        yield rec
    finally:
        for n, f in saved.items():
            setattr(ba, n, f)
        chol.CholeskySolver = solver0
