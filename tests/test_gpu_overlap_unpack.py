"""droid_ba_unpack_chunk and droid_ba_unpack_system on their own: no build, no solve launched.  The packed tensor is
filled with a known fp64 pattern, every chunk of droid_ba_overlap_plan is unpacked in turn, and the pitched system is
read back: each chunk writes its own block columns and nothing to the right of them, the lower triangle and the rhs row
carry the pattern bit for bit, and the diagonal is damped as the header says (diag += ep + lm diag, lm and ep the float32
arguments).  tests/test_gpu_sharded.py sees the same kernel only through a running overlap solve, at one size."""
from types import SimpleNamespace

import numpy as np
import pytest

from util import packed_column_bases as column_bases

NB = 64

pytestmark = pytest.mark.gpu

LM, EP = 1e-4, 0.1


def _binding(torch, P):
    """A BaBinding sized for a window of P poses and nothing else: no edges, 2x2 pixels, a zeroed workspace."""
    from droid_backends.ba_binding import BaBinding
    z = lambda *s: torch.zeros(s, dtype=torch.float32, device="cuda")
    p = SimpleNamespace(disps=z(P, 2, 2), eta=z(P, 2, 2), ii=torch.zeros(0, dtype=torch.int64, device="cuda"))
    b = BaBinding(status_mirror=False, headroom=(1, 0))
    b.begin(p, 0, P, False)
    b.buf.zero_()
    return b


def _expected(pattern, n):
    """Pitched [n + 1, n] image of the packed pattern (whole rows of every block column, as the kernel copies them)."""
    bases = column_bases(n)
    S = np.zeros((n + 1, n))
    for J in range(len(bases) - 1):
        w = min(NB, n - NB * J)
        S[NB * J:, NB * J:NB * J + w] = pattern[bases[J]:bases[J + 1]].reshape(n + 1 - NB * J, w)
    return S


@pytest.mark.parametrize("max_chunks", [1, 2, 4, 32])
@pytest.mark.parametrize("P", [10, 11, 22, 63])   # 1 block column; a last one of width 2; of width 4; 6 block columns
def test_unpack_chunk_places_and_damps_every_block_column(backends, P, max_chunks):
    import torch
    assert torch.cuda.is_available()
    n = 6 * P
    bases = column_bases(n)
    b = _binding(torch, P)
    try:
        packed = b.packed()
        assert packed.numel() == bases[-1]
        pattern = np.random.default_rng(P).standard_normal(bases[-1])
        pattern[np.random.default_rng(P + 1).random(bases[-1]) < 0.05] *= 1e6     # a few decades between entries
        packed.copy_(torch.from_numpy(pattern))
        system = lambda: b.system().view(n + 1, -1)[:, :n].cpu().numpy().copy()
        want = _expected(pattern, n)
        low = np.vstack([np.tril(np.ones((n, n), bool), -1), np.ones((1, n), bool)])   # strictly lower + the rhs row
        lm, ep = float(np.float32(LM)), float(np.float32(EP))
        d = np.diag(want[:n]).copy()
        damped = d + (ep + lm * d)
        plan = b.overlap_plan(max_chunks)
        assert plan[0][0] == 0 and plan[-1][1] == bases[-1]
        for c, (a, e) in enumerate(plan):
            b.unpack_chunk(c, max_chunks, LM, EP, 1)
            torch.cuda.synchronize()
            got = system()
            c1 = min(NB * bases.index(e), n)                 # columns delivered so far; nothing to their right yet
            assert np.array_equal(got[:, :c1][low[:, :c1]], want[:, :c1][low[:, :c1]]), (P, max_chunks, c)
            assert not got[:, c1:].any(), (P, max_chunks, c)
            ulp = np.spacing(np.abs(damped[:c1]))
            assert np.all(np.abs(np.diag(got[:n])[:c1] - damped[:c1]) <= 2 * ulp), (P, max_chunks, c)
        b.unpack_system(False)
        torch.cuda.synchronize()
        got = system()
        assert np.array_equal(got[low], want[low]) and np.array_equal(np.diag(got[:n]), d), (P, max_chunks)
    finally:
        b.close()
