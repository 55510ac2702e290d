"""droid_ba_overlap_plan on the CPU (host arithmetic, no GPU): the chunks of the packed system the ranks all-reduce one by
one while the factorisation is already running.  Swept over every window size up to 342 poses and every max_chunks the
ABI takes, against the layout include/droid_backends_hip.h documents: block column J = rows 64 J .. 6P (row 6P = rhs) as
rows of w_J doubles, w_J = 64, the last one 6P - 64 J."""
import ctypes

import pytest

from util import packed_column_bases as column_bases

P_MAX, CHUNKS_MAX = 342, 32


def plan(lib, P, max_chunks, t0=0):
    nc = ctypes.c_int(-1)
    offs = (ctypes.c_size_t * (CHUNKS_MAX + 1))()
    rc = lib.droid_ba_overlap_plan(t0, t0 + P, max_chunks, ctypes.byref(nc), offs)
    assert rc == 0, (P, max_chunks, rc)
    return [int(offs[c]) for c in range(nc.value + 1)]


def packed_elements(lib, P):
    """What droid_ba_packed_system reports for a window of P poses (host arithmetic on an address it never reads)."""
    dummy = ctypes.create_string_buffer(64)
    nel = ctypes.c_size_t(0)
    ptr = lib.droid_ba_packed_system(ctypes.addressof(dummy), 0, P, 8, 16, 0, P, 0, ctypes.byref(nel))
    assert ptr
    return int(nel.value)


def test_overlap_plan_cuts_at_block_columns(backends):
    lib = backends._lib.load()
    for P in range(1, P_MAX + 1):
        n = 6 * P
        bases = column_bases(n)
        nb = len(bases) - 1
        total = packed_elements(lib, P)
        assert total == bases[-1], (P, total, bases[-1])
        for mc in range(1, CHUNKS_MAX + 1):
            offs = plan(lib, P, mc)
            nc = len(offs) - 1
            assert 1 <= nc <= mc, (P, mc, nc)
            assert offs[0] == 0 and offs[-1] == total, (P, mc, offs)
            assert all(a < b for a, b in zip(offs, offs[1:])), (P, mc, offs)
            assert all(o in bases for o in offs), (P, mc, offs)
            cols = [bases.index(o) for o in offs]
            sizes = [b - a for a, b in zip(cols, cols[1:])]
            want = [1, 1] + list(range(2, CHUNKS_MAX + 2))
            # 1, 1, 2, 3, 4, ... block columns; the last chunk takes what is left: less when the columns run out, more
            # when max_chunks does
            assert sizes[:-1] == want[:nc - 1], (P, mc, sizes)
            if nc < mc:
                assert sizes[-1] <= want[nc - 1], (P, mc, sizes)
            assert sum(sizes) == nb


def test_overlap_plan_depends_on_the_window_size_only(backends):
    lib = backends._lib.load()
    for P, mc in ((10, 4), (63, 4), (342, 32)):
        assert plan(lib, P, mc, t0=0) == plan(lib, P, mc, t0=7)


@pytest.mark.parametrize("t0,t1,mc", [(5, 5, 4), (6, 5, 4), (0, 8, 0), (0, 8, -1), (0, 8, 33)])
def test_overlap_plan_refuses_bad_arguments(backends, t0, t1, mc):
    lib = backends._lib.load()
    nc = ctypes.c_int(0)
    offs = (ctypes.c_size_t * 40)()
    assert lib.droid_ba_overlap_plan(t0, t1, mc, ctypes.byref(nc), offs) == -1
    assert b"ba_overlap_plan" in lib.droid_last_error()


def test_overlap_plan_refuses_null_outputs(backends):
    lib = backends._lib.load()
    nc = ctypes.c_int(0)
    offs = (ctypes.c_size_t * 40)()
    assert lib.droid_ba_overlap_plan(0, 8, 4, None, offs) == -1
    assert lib.droid_ba_overlap_plan(0, 8, 4, ctypes.byref(nc), None) == -1
