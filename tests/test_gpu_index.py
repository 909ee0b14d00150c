"""da_copy_nd on the GPU (kernel level, through _ffi.lib) and the indexing
API built on it (world 1), against numpy.

Kernel level: every case builds its own index arrays from Python
subscripts, so the expected result is dst0[np.ix_(..)] = src[np.ix_(..)]
computed by numpy alone.  Data are random BIT patterns (NaN payloads
included) compared as unsigned words: the copy must be bit-exact.  Scatter
hygiene is part of every case: the destination starts as a sentinel
pattern, both buffers carry 64 guard elements past their logical end, and
the whole destination (guards included) must equal the numpy result while
the whole source must be unchanged.  Each case also asserts the kernel
family the host validator reports before launching.

API level mirrors the reference's view / range-assignment tests
(test/darray.jl:182-221, :745-767) on (200, 200) and a small 3-D array.
"""
import ctypes
import zlib

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

GUARD = 64
NPDT = {"f64": np.float64, "f32": np.float32, "i64": np.int64}
WORD = {"f64": np.uint64, "f32": np.uint32, "i64": np.uint64}
DT = {"f64": 0, "f32": 1, "i64": 2}
U64, I64 = ctypes.c_uint64, ctypes.c_int64


@pytest.fixture(scope="module")
def lib():
    import distributedarrays_jl_amd as dja
    from distributedarrays_jl_amd import _ffi
    dja.comm.init()
    return _ffi.lib


class B:
    """Source-side broadcast of element k: start k, step 0."""

    def __init__(self, k, count):
        self.k, self.count = k, count


def resolve(sub, dim):
    """One subscript -> (index array, start, step, vector-or-None)."""
    if isinstance(sub, B):
        return np.full(sub.count, sub.k, dtype=np.int64), sub.k, 0, None
    if isinstance(sub, int):
        return np.array([sub], dtype=np.int64), sub, 1, None
    if isinstance(sub, slice):
        v = np.arange(dim, dtype=np.int64)[sub]
        return v, (int(v[0]) if v.size else 0), sub.indices(dim)[2], None
    v = np.asarray(sub, dtype=np.int64)
    return v, 0, 1, v


def side_args(shape, subs):
    nd = len(shape)
    ix, keep = [], []
    start, step = (I64 * nd)(), (I64 * nd)()
    idx = (ctypes.c_void_p * nd)()
    for d, (sub, dim) in enumerate(zip(subs, shape)):
        v, s0, st, vec = resolve(sub, dim)
        ix.append(v)
        start[d], step[d] = s0, st
        if vec is not None:
            vec = np.ascontiguousarray(vec)
            keep.append(vec)
            idx[d] = vec.ctypes.data
    return ix, ((U64 * nd)(*shape), start, step, idx), keep


def random_words(rng, n, dt):
    w = rng.integers(0, 2 ** 32, 2 * n, dtype=np.uint32)
    return (w.view(np.uint64)[:n] if WORD[dt] is np.uint64 else w[:n]).copy()


class Dev:
    def __init__(self, lib, words):
        from distributedarrays_jl_amd._ffi import check
        self.lib, self.n, self.wt = lib, words.size, words.dtype
        self.p = ctypes.c_void_p()
        check(lib.da_alloc(words.nbytes, 0, ctypes.byref(self.p)))
        check(lib.da_h2d(self.p, words.ctypes.data_as(ctypes.c_void_p),
                         words.nbytes))

    def read(self):
        from distributedarrays_jl_amd._ffi import check
        out = np.empty(self.n, dtype=self.wt)
        check(self.lib.da_d2h(self.p, out.ctypes.data_as(ctypes.c_void_p),
                              out.nbytes))
        return out

    def free(self):
        self.lib.da_free(self.p)


def run_case(lib, dt, dshape, dsubs, sshape, ssubs, family=None):
    """Launch one da_copy_nd and compare the WHOLE destination and source
    buffers (guards included) with numpy."""
    from distributedarrays_jl_amd import _ffi
    rng = np.random.default_rng(zlib.crc32(repr((dt, dshape, sshape))
                                           .encode()))
    dn, sn = int(np.prod(dshape)), int(np.prod(sshape))
    dst0 = random_words(rng, dn + GUARD, dt)
    dst0[:] = (dst0 & WORD[dt](0xFF)) | WORD[dt](0x5A5A5A00)   # sentinel
    src0 = random_words(rng, sn + GUARD, dt)
    dix, dargs, k1 = side_args(dshape, dsubs)
    six, sargs, k2 = side_args(sshape, ssubs)
    count = tuple(v.size for v in dix)
    assert count == tuple(v.size for v in six)
    cnt = (U64 * len(count))(*count)
    nd = len(count)
    rc_plan = lib.da_copy_nd_plan(*dargs, *sargs, cnt, nd, DT[dt])
    if family is not None:
        assert rc_plan >= 0, lib.da_errstr(rc_plan)
        assert _ffi.COPY_FAMILIES[rc_plan] == family
    d, s = Dev(lib, dst0), Dev(lib, src0)
    try:
        rc = lib.da_copy_nd(d.p, *dargs, s.p, *sargs, cnt, nd, DT[dt])
        _ffi.check(lib.da_synchronize())
        got, src_after = d.read(), s.read()
    finally:
        d.free()
        s.free()
    want = dst0.copy()
    assert rc == 0, lib.da_errstr(rc)
    if all(count):
        wv = want[:dn].reshape(dshape, order="F")
        sv = src0[:sn].reshape(sshape, order="F")
        wv[np.ix_(*dix)] = sv[np.ix_(*six)]
        assert np.shares_memory(wv, want)
    assert np.array_equal(got, want)
    assert np.array_equal(src_after, src0)


DTYPES = ("f64", "f32", "i64")
ALL = slice(None)


# ---- count_0 under, at and over one wavefront, off any vector width ------
@pytest.mark.parametrize("dt", DTYPES)
@pytest.mark.parametrize("c", [1, 63, 64, 65, 257])
def test_count0_runs(lib, dt, c):
    # outer: stepped on the destination, unsorted repeated vector on the
    # source (a vector on an outer dimension stays in the runs family)
    run_case(lib, dt, (300, 4), (slice(3, 3 + c), slice(None, None, 2)),
             (261, 3), (slice(1, 1 + c), [2, 0]), family="runs")


@pytest.mark.parametrize("dt", DTYPES)
@pytest.mark.parametrize("c", [1, 63, 64, 65, 257])
def test_count0_general(lib, dt, c):
    run_case(lib, dt, (2 * c + 5, 3), (slice(1, 1 + 2 * c, 2), [2, 0]),
             (c + 2, 2), (slice(c, 0, -1), ALL), family="general")


# ---- runs family: both sides of the 16-byte alignment gate ---------------
@pytest.mark.parametrize("dt", DTYPES)
@pytest.mark.parametrize("dstart,sstart,dshape0,sshape0,c", [
    (0, 1, 304, 304, 128),    # source start off by one word
    (0, 2, 304, 304, 128),    # f32: 8-byte aligned only; f64: aligned
    (3, 0, 304, 304, 128),    # destination start unaligned
    (1, 1, 304, 304, 128),    # both unaligned the same way
    (0, 0, 301, 304, 128),    # odd destination shape_0: columns drift
    (0, 0, 304, 301, 128),    # odd source shape_0
    (0, 0, 304, 304, 256),    # fully aligned: 16-byte lanes, no tail
    (4, 8, 304, 308, 130),    # aligned with a scalar tail
    (0, 0, 304, 304, 7),      # aligned but shorter than two vectors (f32)
    (0, 0, 4200, 4200, 4100),  # aligned, more than one tile per run
    (0, 1, 4200, 4200, 4100),  # unaligned, more than one tile per run
])
def test_runs_alignment(lib, dt, dstart, sstart, dshape0, sshape0, c):
    run_case(lib, dt, (dshape0, 3), (slice(dstart, dstart + c), ALL),
             (sshape0, 3), (slice(sstart, sstart + c), ALL), family="runs")


@pytest.mark.parametrize("dt", DTYPES)
def test_general_more_than_one_tile(lib, dt):
    run_case(lib, dt, (5003, 2), (slice(None, None, -2), ALL),
             (2502, 2), (ALL, [1, 1]), family="general")


# ---- nd = 1, 2, 3, 4, 6; negative steps on dimension 0 and outer ----------
ND_CASES = [
    ("general", (50,), (slice(None, None, -1),),
     (120,), (slice(10, 110, 2),)),
    ("runs", (50,), (slice(5, 45),), (120,), (slice(60, 100),)),
    ("general", (12, 6), (slice(1, None, 2), slice(None, None, -1)),
     (18, 9), (slice(None, None, 3), [8, 0, 3, 3, 5, 1])),     # both sides
    ("general", (9, 7, 5), (slice(1, 8), slice(None, None, -1), [4, 0, 2]),
     (20, 8, 6), (slice(2, 16, 2), slice(0, 7), slice(None, None, 2))),
    ("runs", (9, 7, 5), (slice(1, 8), slice(None, None, -1), [4, 0, 2]),
     (8, 9, 4), (slice(0, 7), slice(8, 1, -1), [3, 3, 1])),
    ("general", (6, 5, 4, 3),
     (slice(None, None, -1), ALL, slice(None, None, 2), [2, 0]),
     (7, 5, 3, 4),
     (slice(1, 7), slice(None, None, -1), slice(1, 3), slice(None, None, 3))),
    ("runs", (5, 3, 2, 3, 2, 4),
     (slice(0, 4), slice(None, None, -1), ALL, [2, 0], 1,
      slice(None, None, 3)),
     (4, 3, 3, 2, 2, 2),
     (ALL, ALL, slice(None, None, 2), slice(None, None, -1), 0, ALL)),
    ("general", (5, 3, 2, 3, 2, 4),
     (slice(4, 0, -1), slice(None, None, -1), ALL, [2, 0], 1,
      slice(None, None, 3)),
     (4, 3, 3, 2, 2, 2),
     (ALL, ALL, slice(None, None, 2), slice(None, None, -1), 0, ALL)),
    # unsorted, repeated source vector on dimension 0
    ("general", (8, 3), (ALL, ALL),
     (30, 5), ([7, 7, 0, 29, 3, 3, 1, 12], [4, 0, 4])),
    # distinct unsorted destination vector on dimension 0 (scatter)
    ("general", (30, 4), ([7, 29, 0, 3, 12], slice(None, None, -1)),
     (5, 4), (ALL, ALL)),
    # source step 0: one element broadcast into dst[::2, ::3]
    ("general", (9, 10), (slice(None, None, 2), slice(None, None, 3)),
     (1, 1), (B(0, 5), B(0, 4))),
    ("general", (9, 10), (slice(None, None, 2), slice(None, None, 3)),
     (4, 4), (B(2, 5), B(3, 4))),
    # step 0 on an outer dimension only: one column repeated (runs)
    ("runs", (9, 10), (slice(2, 7), slice(None, None, 3)),
     (5, 4), (ALL, B(3, 4))),
]


@pytest.mark.parametrize("dt", DTYPES)
@pytest.mark.parametrize("case", range(len(ND_CASES)))
def test_nd_cases(lib, dt, case):
    family, dshape, dsubs, sshape, ssubs = ND_CASES[case]
    run_case(lib, dt, dshape, dsubs, sshape, ssubs, family=family)


# ---- more outer runs than a grid y/z dimension holds ----------------------
@pytest.mark.parametrize("dt", DTYPES)
def test_many_runs(lib, dt):
    run_case(lib, dt, (3, 70001), (ALL, ALL),
             (3, 140001), (ALL, slice(None, None, 2)), family="runs")


@pytest.mark.parametrize("dt", DTYPES)
def test_many_runs_general(lib, dt):
    run_case(lib, dt, (3, 70001), (slice(None, None, -1), ALL),
             (3, 140001), (ALL, slice(None, None, 2)), family="general")


# ---- zero count and refusals leave the destination untouched -------------
@pytest.mark.parametrize("dt", DTYPES)
def test_zero_count(lib, dt):
    run_case(lib, dt, (10, 4), (slice(3, 3), ALL), (10, 4), (slice(0, 0), ALL))
    run_case(lib, dt, (10, 4), (ALL, []), (10, 4), (ALL, slice(4, 4)))


class Raw:
    """An affine entry passed as given (no numpy clipping), for refusals."""

    def __init__(self, start, step, count):
        self.start, self.step, self.count = start, step, count


def raw_side(shape, subs):
    nd = len(shape)
    start, step = (I64 * nd)(), (I64 * nd)()
    idx = (ctypes.c_void_p * nd)()
    keep, count = [], []
    for d, sub in enumerate(subs):
        if isinstance(sub, Raw):
            start[d], step[d] = sub.start, sub.step
            count.append(sub.count)
        else:
            v = np.ascontiguousarray(sub, dtype=np.int64)
            keep.append(v)
            idx[d] = v.ctypes.data
            step[d] = 1
            count.append(v.size)
    return ((U64 * nd)(*shape), start, step, idx), keep, tuple(count)


REFUSED = [
    # (dst subs over (10, 4), src subs over (10, 4), nd)
    ((Raw(1, 3, 4), Raw(0, 1, 2)), (Raw(0, 1, 4), Raw(0, 1, 2)), 2),
    ((Raw(8, -3, 4), Raw(0, 1, 2)), (Raw(0, 1, 4), Raw(0, 1, 2)), 2),
    ((Raw(0, 1, 4), Raw(0, 1, 2)), (Raw(1, 3, 4), Raw(0, 1, 2)), 2),
    ((Raw(0, 1, 4), Raw(0, 1, 2)), (Raw(8, -3, 4), Raw(0, 1, 2)), 2),
    ((Raw(0, 1, 4), Raw(0, 1, 2)), (Raw(0, 1, 4), [0, 4]), 2),
    (([0, 10, 3, 2], Raw(0, 1, 2)), (Raw(0, 1, 4), Raw(0, 1, 2)), 2),
    ((Raw(0, 1, 4), [3, 3]), (Raw(0, 1, 4), Raw(0, 1, 2)), 2),
    ((Raw(2, 0, 4), Raw(0, 1, 2)), (Raw(0, 1, 4), Raw(0, 1, 2)), 2),
    ((Raw(0, 1, 4), Raw(0, 1, 2)), (Raw(0, 1, 4), Raw(0, 1, 2)), 0),
    ((Raw(0, 1, 4), Raw(0, 1, 2)), (Raw(0, 1, 4), Raw(0, 1, 2)), 7),
]


@pytest.mark.parametrize("case", range(len(REFUSED)))
def test_refusals_leave_destination_untouched(lib, case):
    dsubs, ssubs, nd = REFUSED[case]
    rng = np.random.default_rng(case)
    dst0 = random_words(rng, 40 + GUARD, "f64")
    src0 = random_words(rng, 40 + GUARD, "f64")
    dargs, k1, count = raw_side((10, 4), dsubs)
    sargs, k2, _ = raw_side((10, 4), ssubs)
    cnt = (U64 * 7)(*(count + (1,) * 5))
    d, s = Dev(lib, dst0), Dev(lib, src0)
    try:
        rc = lib.da_copy_nd(d.p, *dargs, s.p, *sargs, cnt, nd, 0)
        assert rc < 0
        assert b"da_copy_nd" in lib.da_errstr(rc)
        from distributedarrays_jl_amd._ffi import check
        check(lib.da_synchronize())
        assert np.array_equal(d.read(), dst0)
    finally:
        d.free()
        s.free()


# ------------------------------------------------------------- API level
@pytest.fixture(scope="module")
def dja(lib):
    import distributedarrays_jl_amd as dja
    return dja


@pytest.fixture(scope="module")
def host():
    rng = np.random.default_rng(99)
    return (np.asfortranarray(rng.standard_normal((200, 200))),
            np.asfortranarray(rng.standard_normal((7, 9, 11))
                              .astype(np.float32)),
            np.asfortranarray(rng.integers(-2 ** 62, 2 ** 62, (33, 17),
                                           dtype=np.int64)))


def test_api_getindex(dja, host):
    m, t, i = host
    M, T, I = dja.distribute(m), dja.distribute(t), dja.distribute(i)
    try:
        assert np.array_equal(M[::2, 1::3], m[::2, 1::3])
        assert np.array_equal(M[::-1, 5:150:7], m[::-1, 5:150:7])
        cols = [199, 0, 17, 17, 64]
        assert np.array_equal(M[3:190:3, cols], m[3:190:3][:, cols])
        assert np.array_equal(M[[0, 2], [1, 3]], m[np.ix_([0, 2], [1, 3])])
        assert np.array_equal(M[cols, ::-5], m[cols][:, ::-5])
        assert np.array_equal(M[7, ::-2], m[7, ::-2])
        assert np.array_equal(M[::9, 199], m[::9, 199])
        assert M[150:10:3, :].shape == (0, 200)
        assert np.array_equal(T[::2, 1, ::-2], t[::2, 1, ::-2])
        assert np.array_equal(T[[6, 0, 6], ::4, [10, 1]],
                              t[np.ix_([6, 0, 6], range(0, 9, 4), [10, 1])])
        assert np.array_equal(I[::-3, [16, 16, 2]], i[::-3][:, [16, 16, 2]])
        # the pinned contiguous and scalar paths still answer
        assert np.array_equal(M[2:60, 10:30], m[2:60, 10:30])
        assert M[5, 6] == m[5, 6]
    finally:
        dja.d_closeall()


def test_api_views(dja, host):
    m, t, _ = host
    M, T = dja.distribute(m), dja.distribute(t)
    try:
        start = dja.bytes_in_use()
        v = dja.dview(M, slice(1, None, 2), [150, 0, 33, 33, 199, 8])
        ref = m[1::2][:, [150, 0, 33, 33, 199, 8]]
        assert dja.bytes_in_use() == start      # a view owns no memory
        assert v.shape == ref.shape
        assert np.array_equal(v.collect(), ref)
        C = v.copy()
        assert C.dims == ref.shape
        assert np.array_equal(C.collect(), ref)
        vv = v[::-3, 1:5]                       # view of a view
        assert np.array_equal(vv.collect(), ref[::-3, 1:5])
        row = dja.dview(v, 42, slice(None, None, -1))
        assert row.shape == (6,)
        assert np.array_equal(row.collect(), ref[42, ::-1])
        assert np.array_equal(row.copy().collect(), ref[42, ::-1])
        assert (v == ref) is True
        bad = ref.copy()
        bad[99, 5] = np.nextafter(bad[99, 5], np.inf)
        assert (v == bad) is False
        assert (v == C) is True and (C == v) is True
        assert (vv == dja.dview(C, slice(None, None, -3), slice(1, 5))) \
            is True
        assert (vv == dja.dview(C, slice(None, None, 3), slice(1, 5))) \
            is False
        tv = dja.dview(T, slice(None, None, 2), 1, slice(None, None, -2))
        assert np.array_equal(tv.collect(), t[::2, 1, ::-2])
        assert np.array_equal(tv.copy().collect(), t[::2, 1, ::-2])
    finally:
        dja.d_closeall()


def test_api_setindex(dja, host):
    from distributedarrays_jl_amd._ffi import DArrayError
    m, t, i = host
    start = dja.bytes_in_use()
    M, ref = dja.distribute(m), m.copy()
    try:
        M[::2, 1::3] = -4.5                                 # scalar
        ref[::2, 1::3] = -4.5
        M[3, ::-2] = 8.0
        ref[3, ::-2] = 8.0
        assert np.array_equal(M.collect(), ref)
        rng = np.random.default_rng(3)
        a = rng.standard_normal((4, 50))                    # ndarray
        M[[199, 0, 5, 6], ::4] = a
        ref[np.ix_([199, 0, 5, 6], range(0, 200, 4))] = a
        b = rng.standard_normal(100)
        M[::-2, 7] = b
        ref[::-2, 7] = b
        assert np.array_equal(M.collect(), ref)
        s = np.asfortranarray(rng.standard_normal((100, 3)))
        S = dja.distribute(s)                               # DArray
        M[1::2, [8, 0, 4]] = S
        ref[np.ix_(range(1, 200, 2), [8, 0, 4])] = s
        assert np.array_equal(M.collect(), ref)
        o = np.asfortranarray(rng.standard_normal((60, 90)))
        O = dja.distribute(o)                               # SubDArray
        M[::50, 20:23] = dja.dview(O, [59, 59, 0, 4], slice(89, 83, -2))
        ref[::50, 20:23] = o[[59, 59, 0, 4]][:, 89:83:-2]
        M[0:4, 0] = dja.dview(M, slice(199, 195, -1), 8)    # same array
        ref[0:4, 0] = ref[199:195:-1, 8].copy()
        v = dja.dview(M, slice(None, None, 2), ALL)         # through a view
        v[1:3, ::-4] = 1.5
        ref[::2][1:3, ::-4] = 1.5
        assert np.array_equal(M.collect(), ref)
        I, iref = dja.distribute(i), i.copy()
        big = (1 << 62) + 12345                             # exact i64
        I[::7, [16, 3]] = big
        iref[np.ix_(range(0, 33, 7), [16, 3])] = big
        assert np.array_equal(I.collect(), iref)
        T, tref = dja.distribute(t), t.copy()
        T[::3, 2, ::-5] = np.float32(0.1)
        tref[::3, 2, ::-5] = np.float32(0.1)
        assert np.array_equal(T.collect(), tref)
        # duplicate destination list: refused for every kind of source
        before = M.collect()
        D3 = dja.distribute(np.zeros((3, 200)))
        for value in (1.0, np.zeros((3, 200)), D3,
                      dja.dview(M, slice(0, 3), ALL)):
            with pytest.raises(DArrayError):
                M[[7, 0, 7], :] = value
        assert np.array_equal(M.collect(), before)
        with pytest.raises(DArrayError):
            M[::2, ::2] = np.zeros((3, 3))
    finally:
        dja.d_closeall()
    assert dja.bytes_in_use() == start
