"""droid_backends.ba_binding.BaBinding against a recording stand-in for the library (no GPU): every integer dimension
reaches every BA function at the position include/droid_backends_hip.h declares for it -- both the `t0, t1, M` and the
`M, t0, t1` functions -- and a growing workspace keeps its pinned words."""
import os
import re
import types

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DIMS = dict(E=5, nbuf=7, H=11, W=13, M=3, t0=1, t1=4)   # pairwise distinct
STREAM = 77


def _header_params():
    """{function: [parameter names in declaration order]} of every droid_ba* function the header declares."""
    txt = open(os.path.join(ROOT, "include", "droid_backends_hip.h")).read()
    txt = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    return {name: [re.findall(r"\w+", a)[-1] for a in args.split(",")]
            for name, args in re.findall(r"\b(droid_ba\w*)\s*\(([^)]*)\)\s*;", txt)}


class Recorder:
    """Stands in for the ctypes library: droid_ba_* attributes append (name, args) to `calls` and return 0
    (droid_ba_workspace_bytes: `nbytes`, because 0 bytes means "bad sizes")."""

    def __init__(self, nbytes=1000):
        self.calls, self.nbytes = [], nbytes

    def __getattr__(self, name):
        if not name.startswith("droid_ba"):
            raise AttributeError(name)
        return lambda *args: self.calls.append((name, args)) or (self.nbytes if name == "droid_ba_workspace_bytes" else 0)


@pytest.fixture
def binding(backends, monkeypatch):
    from droid_backends import ba_binding
    monkeypatch.setattr(ba_binding, "_stream", lambda: STREAM)
    return ba_binding.BaBinding(lib=Recorder(), pinned=torch.zeros(8, dtype=torch.int32))


def _problem(d=DIMS):
    f = lambda *shape: torch.zeros(shape)
    return types.SimpleNamespace(poses=f(d["nbuf"], 7), disps=f(d["nbuf"], d["H"], d["W"]), intrinsics=f(4),
                                 disps_sens=f(d["nbuf"], d["H"], d["W"]), targets=f(d["E"], 2, d["H"], d["W"]),
                                 weights=f(d["E"], 2, d["H"], d["W"]), eta=f(d["M"], d["H"], d["W"]),
                                 ii=torch.zeros(d["E"], dtype=torch.int64), jj=torch.zeros(d["E"], dtype=torch.int64))


def test_dimensions_reach_every_function_in_the_header_s_order(binding):
    b, p = binding, _problem()
    assert b.begin(p, DIMS["t0"], DIMS["t1"], False, "cpu") == tuple(DIMS[k] for k in ("E", "nbuf", "H", "W", "M", "t0", "t1"))
    dx, dz = torch.zeros(3, 6), torch.zeros(DIMS["M"], DIMS["H"] * DIMS["W"])
    b.ba(p, 2, 0.25, 0.5, False, dx, dz)
    b.prepare(p, (17, 19), False)
    b.build(p, False)
    b.build(p, False, packed=True)
    b.unpack_system(False)
    b.solve_update(p, 0.25, 0.5, False, dx, dz)
    b.overlap_available()
    b.overlap_plan(6)
    b.unpack_chunk(2, 6, 0.25, 0.5, 9)
    b.solve_update_overlap(p, 9, False, dx, dz)
    b.profile_iteration(p, 0.25, 0.5, False)
    b.system()
    b.packed()
    b.status()
    ws = b.buf.data_ptr()
    b.close()
    params = _header_params()
    called = {name for name, _ in b.lib.calls}
    assert called == set(params), (sorted(called), sorted(params))   # every BA function of the header, no other
    ptrs = dict(poses=p.poses, disps=p.disps, intrinsics=p.intrinsics, disps_sens=p.disps_sens, targets=p.targets,
                weights=p.weights, eta=p.eta, ii=p.ii, jj=p.jj, dx_out=dx, dz_out=dz)
    for name, args in b.lib.calls:
        names = params[name]
        assert len(args) == len(names), (name, len(args), names)
        got = dict(zip(names, args))
        for k, v in DIMS.items():
            if k in got:
                assert got[k] == v, (name, k, got[k], names)
        for k, t in ptrs.items():
            if k in got:
                assert got[k] == t.data_ptr(), (name, k)
        if "stream" in got:
            assert got["stream"] == STREAM, name
        if "workspace_bytes" in got:
            assert got["workspace_bytes"] >= 1000, name
        # the scalars, each with a value of its own (pairwise distinct from the dimensions too)
        for k, v in dict(workspace=ws, own0=17, own1=19, lm=0.25, ep=0.5, iterations=2, chunk=2, max_chunks=6, epoch=9,
                         motion_only=0).items():
            if k in got:
                assert got[k] == v, (name, k, got[k])
    seen = {k for name, _ in b.lib.calls for k in params[name]}
    assert set(DIMS) <= seen and {"own0", "own1", "stream", "workspace", "lm", "ep", "iterations", "chunk", "epoch"} <= seen


def test_growth_keeps_the_pinned_words_and_detaches_the_old_buffer_first(binding):
    b = binding
    b.reserve(1000, "cpu")
    first = b.buf.data_ptr()
    b.reserve(500, "cpu")                    # fits: nothing happens
    assert b.buf.data_ptr() == first and len(b.lib.calls) == 2
    b.reserve(100000, "cpu")
    second = b.buf.data_ptr()
    assert second != first and b.buf.numel() >= 100000
    mirror, hints = b.mirror.data_ptr(), b.mirror.data_ptr() + 4 * b.HINT_WORD
    assert b.lib.calls == [("droid_ba_attach_status_mirror", (first, mirror)), ("droid_ba_attach_launch_hints", (first, hints)),
                           ("droid_ba_attach_status_mirror", (first, None)), ("droid_ba_attach_launch_hints", (first, None)),
                           ("droid_ba_attach_status_mirror", (second, mirror)), ("droid_ba_attach_launch_hints", (second, hints))]
    b.close()
    assert b.lib.calls[-2:] == [("droid_ba_attach_status_mirror", (second, None)), ("droid_ba_attach_launch_hints", (second, None))]
    assert b.buf is None


def test_without_a_status_mirror_only_the_hints_are_attached(backends):
    from droid_backends import ba_binding
    b = ba_binding.BaBinding(lib=Recorder(), status_mirror=False, pinned=torch.zeros(8, dtype=torch.int32), headroom=(1, 0))
    b.reserve(1000, "cpu")
    assert b.buf.numel() == 1000            # no headroom asked for: exactly the bytes
    b.close()
    assert [name for name, _ in b.lib.calls] == ["droid_ba_attach_launch_hints"] * 2
