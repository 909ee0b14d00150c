"""Strided / index-vector indexing, views and range assignment at world
sizes 2 and 4: the REAL orchestration code (plan.sel_plan, ops.gather_sel,
dsub, dsetindex_, SubDArray) over the fakelib ABI (numpy chunks + gloo,
see fakelib.py), with a numpy da_copy_nd built on np.ix_ added to the
installed FakeLib instance from this file.  Every expected value is numpy
indexing of the host array; every scenario ends with d_closeall() and a
zero-leak check."""
import ctypes
import os

import numpy as np
import pytest
import torch.multiprocessing as mp


# ------------------------------------------------ numpy da_copy_nd (fake)
def _fake_copy_nd(dst, dsh, dst0, dstp, didx, src, ssh, sst0, sstp, sidx,
                  count, nd, dtype):
    import fakelib
    nd = int(nd)
    dt = fakelib._NPDT[int(dtype)]

    def ints(p, ct):
        a = fakelib._addr(p)
        if a == 0:
            return None
        q = ctypes.cast(ctypes.c_void_p(a), ctypes.POINTER(ct))
        return [int(q[i]) for i in range(nd)]

    cnt = ints(count, ctypes.c_uint64)

    def side(shape, start, step, idx):
        shape = ints(shape, ctypes.c_uint64)
        start = ints(start, ctypes.c_int64) or [0] * nd
        step = ints(step, ctypes.c_int64) or [1] * nd
        vecs = ints(idx, ctypes.c_uint64) or [0] * nd
        ix = []
        for d in range(nd):
            if vecs[d]:
                q = ctypes.cast(ctypes.c_void_p(vecs[d]),
                                ctypes.POINTER(ctypes.c_int64))
                v = np.array([q[i] for i in range(cnt[d])], dtype=np.int64)
            else:
                v = start[d] + step[d] * np.arange(cnt[d], dtype=np.int64)
            assert v.size == 0 or (v.min() >= 0 and v.max() < shape[d]), \
                "da_copy_nd index outside its buffer"
            ix.append(v)
        return shape, ix

    dshape, dix = side(dsh, dst0, dstp, didx)
    sshape, six = side(ssh, sst0, sstp, sidx)
    if any(c == 0 for c in cnt):
        return 0
    for v in dix:
        assert np.unique(v).size == v.size, "duplicate destination index"
    dv = fakelib._tv(dst, int(np.prod(dshape)), dt).reshape(dshape,
                                                            order="F")
    sv = fakelib._tv(src, int(np.prod(sshape)), dt).reshape(sshape,
                                                            order="F")
    dv[np.ix_(*dix)] = sv[np.ix_(*six)]
    return 0


# ------------------------------------------------------- spawn plumbing
def _run_scenario(rank, tmpfile, q, world, name):
    try:
        os.environ["RANK"] = str(rank)
        os.environ["WORLD_SIZE"] = str(world)
        os.environ["MASTER_ADDR"] = "127.0.0.1"
        import torch.distributed as td
        td.init_process_group("gloo", init_method="file://%s" % tmpfile,
                              rank=rank, world_size=world)
        import fakelib
        fake = fakelib.install()
        fake.da_copy_nd = _fake_copy_nd
        import distributedarrays_jl_amd as dja
        dja.comm.init()
        globals()["_scenario_" + name](rank, world, dja)
        dja.d_closeall()
        assert fake.user_bytes == 0, \
            "leaked %d bytes of ABI allocations" % fake.user_bytes
        q.put((rank, True, None))
    except Exception:
        import traceback
        q.put((rank, False, traceback.format_exc()[-2000:]))
    finally:
        import torch.distributed as td
        if td.is_initialized():
            td.destroy_process_group()


def _spawn(tmp_path, world, name):
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    tmpfile = str(tmp_path / "rdv")
    procs = [ctx.Process(target=_run_scenario,
                         args=(r, tmpfile, q, world, name))
             for r in range(world)]
    for p in procs:
        p.start()
    results = [q.get(timeout=240) for _ in range(world)]
    for p in procs:
        p.join(timeout=60)
    for rank, ok, err in sorted(results):
        assert ok, "rank %d failed:\n%s" % (rank, err)


def _host(shape, seed, dtype=np.float64):
    rng = np.random.default_rng(seed)
    if np.dtype(dtype).kind == "i":
        return np.asfortranarray(
            rng.integers(-2 ** 62, 2 ** 62, shape, dtype=np.int64))
    return np.asfortranarray(rng.standard_normal(shape).astype(dtype))


# ------------------------------------------------------------ scenarios
def _scenario_getindex(rank, world, dja):
    g = _host((40,), 1)
    D = dja.distribute(g)
    assert np.array_equal(D[::3], g[::3])
    assert np.array_equal(D[::-1], g[::-1])
    assert np.array_equal(D[[7, 0, 7, 39]], g[[7, 0, 7, 39]])
    assert np.array_equal(D[5::-2], g[5::-2])
    assert D[30:2:5].shape == (0,)
    m = _host((9, 7), 2)
    M = dja.distribute(m)
    assert np.array_equal(M[1::2, [5, 0, 2]], m[1::2][:, [5, 0, 2]])
    # outer product, not numpy's zipped pairs
    assert np.array_equal(M[[0, 2], [1, 3]], m[np.ix_([0, 2], [1, 3])])
    # int + stepped slice squeezes the int dimension
    assert np.array_equal(M[4, ::-2], m[4, ::-2])
    assert np.array_equal(M[::4, 6], m[::4, 6])
    t = _host((6, 5, 7), 3, np.float32)
    T = dja.distribute(t)
    assert np.array_equal(T[::2, 1, ::-2], t[::2, 1, ::-2])
    i = _host((11, 6), 4, np.int64)
    I = dja.distribute(i, dist=(1, 2))
    assert np.array_equal(I[[10, 10, 3], ::-1], i[[10, 10, 3], ::-1])
    from distributedarrays_jl_amd._ffi import DArrayError
    for bad in ([40], [-1]):
        try:
            D[bad]
            assert False, "expected DArrayError"
        except DArrayError:
            pass


def _scenario_views(rank, world, dja):
    m = _host((13, 10), 5)
    # source split by columns, result default-distributed over its own
    # (smaller) shape: the result's cuts do not align with the source's
    M = dja.distribute(m, dist=(1, world))
    v = dja.dview(M, slice(1, None, 2), [9, 0, 2, 2, 7])
    ref = m[1::2][:, [9, 0, 2, 2, 7]]
    assert v.shape == ref.shape
    assert np.array_equal(v.collect(), ref)
    C = v.copy()
    assert C.dims == ref.shape
    assert [ix for ix in C.idxs] != [ix for ix in M.idxs]
    assert np.array_equal(C.collect(), ref)
    # view of a view, int squeeze, reversed
    vv = v[::-1, 1:4]
    assert np.array_equal(vv.collect(), ref[::-1, 1:4])
    row = dja.dview(v, 2, slice(None, None, -1))
    assert row.shape == (5,)
    assert np.array_equal(row.collect(), ref[2, ::-1])
    R = row.copy()
    assert R.dims == (5,) and np.array_equal(R.collect(), ref[2, ::-1])
    # == against ndarray / DArray / SubDArray
    assert (v == ref) is True
    assert (v == ref + 1.0) is False
    assert (v == C) is True
    assert (C == v) is True
    assert (v == dja.dview(C, slice(None), slice(None))) is True
    assert (vv == dja.dview(C, slice(None, None, -1), slice(1, 4))) is True
    assert (vv == dja.dview(C, slice(None), slice(1, 4))) is False
    # 3-D
    t = _host((5, 6, 4), 6, np.float32)
    T = dja.distribute(t)
    tv = dja.dview(T, slice(None, None, 2), 1, slice(None, None, -2))
    assert np.array_equal(tv.collect(), t[::2, 1, ::-2])
    TC = tv.copy()
    assert np.array_equal(TC.collect(), t[::2, 1, ::-2])
    # a view owns no device memory
    before = dja.bytes_in_use()
    dja.dview(M, slice(None, None, 3), slice(None))
    assert dja.bytes_in_use() == before


def _scenario_setindex(rank, world, dja):
    m = _host((12, 9), 7)
    M = dja.distribute(m)
    ref = m.copy()
    # scalar
    M[::2, 1::3] = -4.5
    ref[::2, 1::3] = -4.5
    assert np.array_equal(M.collect(), ref)
    M[3, ::-2] = 8.0
    ref[3, ::-2] = 8.0
    assert np.array_equal(M.collect(), ref)
    M[2:5, 1:3] = 0.25                       # plain ranges assign too
    ref[2:5, 1:3] = 0.25
    assert np.array_equal(M.collect(), ref)
    # ndarray
    a = _host((4, 3), 8)
    M[[11, 0, 5, 6], ::4] = a
    ref[np.ix_([11, 0, 5, 6], [0, 4, 8])] = a
    assert np.array_equal(M.collect(), ref)
    b = _host((6,), 9)
    M[::-2, 7] = b                           # squeezed shape
    ref[::-2, 7] = b
    assert np.array_equal(M.collect(), ref)
    # DArray with different cuts (source by rows, destination by default)
    s = _host((6, 3), 10)
    S = dja.distribute(s, dist=(world, 1))
    M[1::2, [8, 0, 4]] = S
    ref[np.ix_(np.arange(1, 12, 2), [8, 0, 4])] = s
    assert np.array_equal(M.collect(), ref)
    # view of another array (repeats allowed on the source side)
    o = _host((10, 14), 11)
    O = dja.distribute(o, dist=(1, world))
    M[::3, 2:5] = dja.dview(O, [9, 9, 0, 4], slice(13, 7, -2))
    ref[::3, 2:5] = o[[9, 9, 0, 4]][:, 13:7:-2]
    assert np.array_equal(M.collect(), ref)
    # a view of the SAME array (packed through a temporary)
    M[0:4, 0] = dja.dview(M, slice(11, 7, -1), 8)
    ref[0:4, 0] = ref[11:7:-1, 8].copy()
    assert np.array_equal(M.collect(), ref)
    # assignment through a view
    v = dja.dview(M, slice(None, None, 2), slice(None))
    v[1:3, ::-4] = 1.5
    ref[::2][1:3, ::-4] = 1.5
    assert np.array_equal(M.collect(), ref)
    # 1-D i64 beyond 2^53 stays exact
    g = _host((40,), 12, np.int64)
    D = dja.distribute(g)
    big = (1 << 62) + 12345
    D[::7] = big
    g[::7] = big
    assert np.array_equal(D.collect(), g)
    from distributedarrays_jl_amd._ffi import DArrayError
    for bad in (np.zeros((3, 3)), S):
        try:
            M[::2, ::2] = bad
            assert False, "expected DArrayError (shape mismatch)"
        except DArrayError:
            pass


def _scenario_dup_raises(rank, world, dja):
    """A repeated destination index raises on EVERY rank before any device
    or transport work (so nobody is left waiting in a collective), for
    all three kinds of source."""
    from distributedarrays_jl_amd._ffi import DArrayError
    g = _host((40,), 13)
    D = dja.distribute(g)
    S = dja.distribute(_host((3,), 14))
    for value in (1.0, np.zeros(3), S, dja.dview(D, slice(0, 3))):
        try:
            D[[7, 0, 7]] = value
            assert False, "expected DArrayError"
        except DArrayError:
            pass
    assert np.array_equal(D.collect(), g)    # untouched, still in step
    D[[7, 0, 8]] = S
    g[[7, 0, 8]] = S.collect()
    assert np.array_equal(D.collect(), g)


SCENARIOS = ["getindex", "views", "setindex", "dup_raises"]


@pytest.mark.timeout(420)
@pytest.mark.parametrize("name", SCENARIOS)
@pytest.mark.parametrize("world", [2, 4])
def test_index(tmp_path, world, name):
    _spawn(tmp_path, world, name)
