"""The linearisation alone through the test hook droid_test_ba_lin (include/droid_test_hooks_hip.h), with either body of
ba_lin_kernel, and the host's choice of instantiation restated -- shared by tests/test_gpu_lin_pinned.py and
tests/test_gpu_lin_directed.py."""
import ctypes

from util import to_dev

LIN_CP, LIN_WAVES, LIN_WGS = 512, 4, 1536     # csrc/ba_internal.hpp
ARRAYS = ("Hpart", "Q", "w", "Ebuf")
FULL_INSTANTIATIONS = {(1, 0, 0), (1, 0, 1), (1, 1, 0), (1, 1, 1), (0, 0, 0)}


def instantiation(p, motion_only):
    """(depth, E rows, edge ranges) of the ba_lin_kernel the host launches (ba_internal.hpp::ba_carve, launch_build_stage),
    restated so that the table can be checked without a GPU; run_lin holds it against what the library reports."""
    _, H, W = p.disps.shape
    if motion_only:
        return (0, 0, 0)
    M, E, nch = p.eta.shape[0], len(p.ii), (H * W + LIN_CP - 1) // LIN_CP
    wide = M > 0 and E >= 12 * M and (H * W) % 32 == 0
    zsplit = min(max(LIN_WGS // (M * nch), 1), 8)
    return (1, int(wide), int(zsplit > 1))


def run_lin(backends, p, motion_only, ragged):
    """The linearisation of `p` on a zeroed workspace of its own after droid_ba_prepare, with the FULL (ragged = 0) or
    the ragged body; returns {name: int32 numpy view} of what the hook copies out."""
    import torch
    from droid_backends._args import _stream
    from droid_backends.ba_binding import BAProblemDev, BaBinding
    lib = backends._lib.load()
    d = BAProblemDev(**to_dev(p, torch))
    b = BaBinding(status_mirror=False, headroom=(1, 0))
    try:
        E, nbuf, H, W, M, t0, t1 = b.begin(d, p.t0, p.t1, motion_only)
        b.buf.zero_()
        b.prepare(d, (0, nbuf), motion_only)
        ws = (b.buf.data_ptr(), b.buf.numel())
        args = (*b._build_args(d), int(motion_only), int(ragged), *ws)
        words = (ctypes.c_size_t * 6)()
        backends._lib.check(lib.droid_test_ba_lin(*args, None, None, None, None, words, _stream()), "test_ba_lin (sizes)")
        nch = (H * W + LIN_CP - 1) // LIN_CP
        # the instantiation the HOST chooses (words 4, 5: E rows kept, edge ranges) is the one the table names
        assert (int(not motion_only), 0 if motion_only else int(words[4]), 0 if motion_only else int(words[5] > 1)) == \
            instantiation(p, motion_only), (int(words[4]), int(words[5]))
        words = list(words)[:4]
        assert words[0] == E * nch * LIN_WAVES * 32 and words[1] == words[2] == M * H * W
        assert words[3] in (0, 6 * (M + E) * H * W)
        out = [torch.full((max(int(n), 1),), float("nan"), dtype=torch.float32, device="cuda") for n in words]
        ptr = [o.data_ptr() if n else None for o, n in zip(out, words)]
        backends._lib.check(lib.droid_test_ba_lin(*args, *ptr, None, _stream()), "test_ba_lin")
        torch.cuda.synchronize()
        st, _ = b.status()
        assert st & 15 == 0, st
    finally:
        b.close()
    return {k: o[:int(n)].view(torch.int32).cpu().numpy() for k, o, n in zip(ARRAYS, out, words)}


def assert_bodies_equal(full, ragged, motion_only, inst, tag):
    """0 differing 32-bit words between what the two bodies left, and the arrays are live (the launch ran, wrote its
    sums and, where the instantiation keeps E rows, stored some).  Returns the counts of differing words."""
    diff = {k: int((full[k] != ragged[k]).sum()) for k in full}
    live = {k: int((ragged[k] != 0).sum()) for k in ragged}
    print(f"[{tag}] instantiation {inst}: differing words " + "  ".join(f"{k} {diff[k]} of {full[k].size}" for k in full)
          + f"   (non-zero words: {live})")
    assert live["Hpart"] > 0                       # the launch ran and wrote its sums
    if not motion_only:
        assert live["Q"] == full["Q"].size and live["w"] > 0
    assert (full["Ebuf"].size > 0) == bool(inst[1])
    if inst[1]:
        assert live["Ebuf"] > 0                    # some slot of the graph has its E rows stored
    assert diff == {k: 0 for k in diff}, diff
    return diff
