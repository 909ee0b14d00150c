"""da_copy_nd_plan — the host-only validator / family selector of the N-D
selection copy.  dlopen needs no GPU and the function needs no da_init, so
every refusal that keeps a launch inside its two buffers is checked here."""
import ctypes

import numpy as np
import pytest

from distributedarrays_jl_amd import _ffi

U64, I64 = ctypes.c_uint64, ctypes.c_int64


def side(shape, start=None, step=None, idx=None):
    """(shape, start, step, idx) ctypes arrays for one side; idx is a list
    with a sequence or None per dimension."""
    nd = len(shape)
    keep = []
    c_idx = None
    if idx is not None:
        c_idx = (ctypes.c_void_p * nd)()
        for d, v in enumerate(idx):
            if v is not None:
                arr = np.ascontiguousarray(v, dtype=np.int64)
                keep.append(arr)
                c_idx[d] = arr.ctypes.data
    return ((U64 * nd)(*shape),
            (I64 * nd)(*start) if start is not None else None,
            (I64 * nd)(*step) if step is not None else None,
            c_idx, keep)


def plan_rc(dst, src, count, nd=None, dtype=0):
    nd = len(count) if nd is None else nd
    return _ffi.lib.da_copy_nd_plan(dst[0], dst[1], dst[2], dst[3],
                                    src[0], src[1], src[2], src[3],
                                    (U64 * max(len(count), 1))(*count), nd,
                                    dtype)


def refused(rc):
    msg = _ffi.lib.da_errstr(rc)
    return rc < 0 and msg is not None and b"da_copy_nd" in msg


def family(rc):
    assert rc >= 0, _ffi.lib.da_errstr(rc)
    return _ffi.COPY_FAMILIES[rc]


DENSE = lambda count: side(count)


def test_accepts_dense_and_reports_runs():
    assert family(plan_rc(DENSE((5, 4)), DENSE((5, 4)), (5, 4))) == "runs"


@pytest.mark.parametrize("start,step,count,ok", [
    (0, 3, 4, True),        # 0,3,6,9 in [0,10)
    (1, 3, 4, False),       # ..,10 is one past the end
    (9, -3, 4, True),       # 9,6,3,0
    (8, -3, 4, False),      # ..,-1
    (10, 1, 1, False),      # start itself outside
    (-1, 1, 2, False),
    (9, 1 << 62, 2, False),  # end far outside, no wrap-around
])
def test_affine_range_both_sides(start, step, count, ok):
    sel = side((10,), (start,), (step,))
    for rc in (plan_rc(sel, DENSE((count,)), (count,)),
               plan_rc(DENSE((count,)), sel, (count,))):
        assert (rc >= 0) if ok else refused(rc)


def test_vector_entry_out_of_range():
    for bad in ([0, 10], [-1, 3]):
        sel = side((10,), idx=[bad])
        assert refused(plan_rc(sel, DENSE((2,)), (2,)))
        assert refused(plan_rc(DENSE((2,)), sel, (2,)))
    ok = side((10,), idx=[[9, 0]])
    assert family(plan_rc(ok, DENSE((2,)), (2,))) == "general"


def test_duplicate_destination_vector_entry():
    dup = side((10, 4), idx=[None, [3, 1, 3]])
    assert refused(plan_rc(dup, DENSE((10, 3)), (10, 3)))
    # the same vector is fine on the source side (repeats allowed there)
    assert family(plan_rc(DENSE((10, 3)), dup, (10, 3))) == "runs"


def test_zero_step():
    zero = side((10, 4), (2, 1), (1, 0))
    assert refused(plan_rc(zero, DENSE((3, 2)), (3, 2)))      # dst: refused
    assert plan_rc(DENSE((3, 2)), zero, (3, 2)) >= 0          # src: broadcast
    assert plan_rc(zero, DENSE((3, 1)), (3, 1)) >= 0          # count 1 is fine
    scalar = side((1, 1), (0, 0), (0, 0))
    assert family(plan_rc(side((6, 5), (0, 1), (2, 3)), scalar,
                          (3, 2))) == "general"


@pytest.mark.parametrize("nd", [0, 7, -1])
def test_nd_out_of_range(nd):
    shape = (2,) * 7
    assert refused(plan_rc(DENSE(shape), DENSE(shape), shape, nd=nd))


def test_nd_six_accepted_and_bad_dtype():
    shape = (2,) * 6
    assert plan_rc(DENSE(shape), DENSE(shape), shape) >= 0
    assert refused(plan_rc(DENSE(shape), DENSE(shape), shape, dtype=3))
    assert refused(plan_rc(DENSE(shape), DENSE(shape), shape, dtype=-1))
    for dt in (0, 1, 2):
        assert plan_rc(DENSE(shape), DENSE(shape), shape, dtype=dt) >= 0


def test_zero_count_is_accepted():
    # nothing is touched, so even an out-of-range start passes
    far = side((10, 4), (50, 0), (1, 1))
    assert plan_rc(far, DENSE((0, 4)), (0, 4)) >= 0
    assert plan_rc(DENSE((3, 0)), side((10, 4), idx=[None, []]), (3, 0)) >= 0


@pytest.mark.parametrize("dstep,sstep,dvec,svec,want", [
    (1, 1, False, False, "runs"),
    (2, 1, False, False, "general"),
    (1, -1, False, False, "general"),
    (1, 0, False, False, "general"),
    (1, 1, True, False, "general"),
    (1, 1, False, True, "general"),
])
def test_family_rule(dstep, sstep, dvec, svec, want):
    """runs exactly when dimension 0 is affine with step 1 on both sides,
    whatever the outer dimensions do."""
    n = 4
    vec = [5, 0, 9, 2]
    for outer_vec in (False, True):
        dst = side((40, 6), (20, 5), (dstep, -2),
                   idx=[vec if dvec else None, None])
        src = side((40, 6), (20, 0), (sstep, 1),
                   idx=[vec if svec else None,
                        [3, 3, 0] if outer_vec else None])
        assert family(plan_rc(dst, src, (n, 3))) == want
