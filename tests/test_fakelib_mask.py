"""dfilter / dfindall / dsetmask_ and the D[M] sugar at world sizes 1, 2 and
4: the REAL orchestration code (ops._compact, ops.dsetmask_: mask
localisation, the shared counts, the redistribution fallback, the copy
back, the clean-up) over the fakelib ABI (numpy chunks + gloo, see
fakelib.py), with numpy da_compact / da_expand added to the installed
FakeLib instance from this file.  Masks are 0/1 DArrays distributed from
numpy (the fake da_expr predates comparisons).  Every expected value is
numpy boolean indexing on the Fortran-ordered host array, compared bit for
bit; every scenario ends with d_closeall() and a zero-leak check."""
import os

import numpy as np
import pytest
import torch.multiprocessing as mp


# ----------------------------------------- numpy da_compact / da_expand
def _fake_compact(dst, dst_cap, src, dtype, mask, mask_dtype, n,
                  index_base):
    import fakelib
    n, cap = int(n), int(dst_cap)
    if n == 0 or cap == 0:
        return 0
    assert fakelib._addr(dst) and fakelib._addr(mask)
    m = fakelib._tv(mask, n, fakelib._NPDT[int(mask_dtype)])
    keep = np.flatnonzero(m != 0)
    # the orchestration sizes dst from da_count: exactly the number kept
    assert cap == keep.size, (cap, keep.size)
    if fakelib._addr(src):
        dt = fakelib._NPDT[int(dtype)]
        fakelib._tv(dst, keep.size, dt)[:] = fakelib._tv(src, n, dt)[keep]
    else:
        fakelib._tv(dst, keep.size, np.dtype("int64"))[:] = \
            int(index_base) + keep
    return 0


def _fake_expand(dst, dtype, mask, mask_dtype, n, src, src_n, bcast):
    import fakelib
    n, src_n = int(n), int(src_n)
    if n == 0 or src_n == 0:
        return 0
    assert fakelib._addr(dst) and fakelib._addr(mask) and fakelib._addr(src)
    dt = fakelib._NPDT[int(dtype)]
    m = fakelib._tv(mask, n, fakelib._NPDT[int(mask_dtype)])
    keep = np.flatnonzero(m != 0)
    d = fakelib._tv(dst, n, dt)
    if int(bcast):
        d[keep] = fakelib._tv(src, 1, dt)[0]
    else:
        assert src_n == keep.size, (src_n, keep.size)
        d[keep] = fakelib._tv(src, src_n, dt)
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
        fake.da_compact = _fake_compact
        fake.da_expand = _fake_expand
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


# ----------------------------------------------------------------- data
_NP = {"f64": np.float64, "f32": np.float32, "i64": np.int64}


def _data(shape, seed, dtype):
    rng = np.random.default_rng(seed)
    if dtype == "i64":
        x = rng.integers(-2 ** 62, 2 ** 62, shape, dtype=np.int64)
    else:
        x = rng.standard_normal(shape).astype(_NP[dtype])
    return np.asfortranarray(x)


def _mask(shape, seed, dtype="f64", density=0.5):
    rng = np.random.default_rng(seed)
    return np.asfortranarray((rng.random(shape) < density)
                             .astype(_NP[dtype]))


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint64 if a.dtype.itemsize == 8 else np.uint32)


def _same(a, b):
    return (a.dtype == b.dtype and a.shape == b.shape
            and np.array_equal(_bits(a), _bits(b)))


def _kept(x, m):
    return x.ravel(order="F")[m.ravel(order="F") != 0]


def _assigned(x, m, v):
    flat = x.ravel(order="F").copy()
    flat[m.ravel(order="F") != 0] = v
    return np.asfortranarray(flat.reshape(x.shape, order="F"))


def _grids(world):
    """(shape, dist) pairs whose chunk count fits the world; the grids that
    cut another dimension than the last take the redistribution path."""
    allg = [((37,), (1,)), ((37,), (2,)), ((37,), (4,)),
            ((9, 7), (1, 1)), ((9, 7), (1, 2)), ((9, 7), (1, 4)),
            ((9, 7), (2, 1)), ((9, 7), (4, 1)), ((9, 7), (2, 2)),
            ((5, 4, 6), (2, 1, 2)), ((5, 4, 6), (1, 1, 4)),
            ((3,), (4,)),          # fewer elements than ranks: empty chunks
            ((3, 2), (4, 1))]
    return [(s, d) for s, d in allg if int(np.prod(d)) <= world]


def _check(dja, x, m, dist, mdist=None):
    """dfilter and dfindall of one (data, mask) pair; nothing leaks."""
    D = dja.distribute(x, dist=dist)
    M = dja.distribute(m, dist=mdist or dist)
    before = dja.bytes_in_use()
    R = dja.dfilter(M, D)
    exp = _kept(x, m)
    assert R.ndims == 1 and R.dims == (exp.size,) and R.dtype == D.dtype
    assert _same(R.collect(), exp), (x.shape, dist, mdist)
    I = dja.dfindall(M, D)
    idx = np.flatnonzero(m.ravel(order="F"))
    assert I.dtype == "i64" and I.dims == (idx.size,)
    assert np.array_equal(I.collect(), idx), (x.shape, dist, mdist)
    J = dja.dfindall(M)
    assert np.array_equal(J.collect(), idx)
    # the inputs are untouched
    assert _same(D.collect(), x) and _same(M.collect(), m)
    for t in (R, I, J):
        t.close()
    assert dja.bytes_in_use() == before
    D.close()
    M.close()


# ------------------------------------------------------------ scenarios
def _scenario_vector_even(rank, world, dja):
    seed = 0
    for n in (37, 8 * world, 3):
        for dtype in ("f64", "f32", "i64"):
            for mdtype in ("f64", "f32", "i64"):
                seed += 1
                _check(dja, _data((n,), seed, dtype),
                       _mask((n,), 100 + seed, mdtype), (world,))
    # rank r's chunk of the result is rank r's survivors: nothing moved
    x, m = _data((41,), 7, "f64"), _mask((41,), 8)
    D, M = dja.distribute(x), dja.distribute(m)
    R = dja.dfilter(M, D)
    (lo, hi), = D.lidx
    assert _same(R.localpart(), _kept(x[lo:hi], m[lo:hi]))
    assert dja.bytes_in_use() > 0
    for t in (D, M, R):
        t.close()
    assert dja.bytes_in_use() == 0


def _scenario_ragged(rank, world, dja):
    """The output of a dfilter (ragged cuts) filtered again with an evenly
    cut mask: the mask is localised onto the ragged boxes."""
    x, m = _data((61,), 1, "i64"), _mask((61,), 2, "i64", 0.6)
    D, M = dja.distribute(x), dja.distribute(m)
    R = dja.dfilter(M, D)
    y = _kept(x, m)
    m2 = _mask((y.size,), 3, "f64", 0.4)
    M2 = dja.distribute(m2)
    before = dja.bytes_in_use()
    R2 = dja.dfilter(M2, R)
    assert _same(R2.collect(), _kept(y, m2))
    I2 = dja.dfindall(M2, R)
    assert np.array_equal(I2.collect(), np.flatnonzero(m2))
    # a ragged mask over evenly cut data, too
    q = _mask((61,), 5, "f64", 0.5)
    Q = dja.distribute(q)
    Mr = dja.dfilter(M, Q)                      # q[m != 0], ragged cuts
    Y = dja.distribute(y)
    R3 = dja.dfilter(Mr, Y)
    assert _same(R3.collect(), _kept(y, _kept(q, m)))
    for t in (R2, I2, R3, Q):
        t.close()
    assert _same(R.collect(), y) and _same(Y.collect(), y)
    # assigning through a ragged destination, and with a ragged mask
    v = _data((int(np.count_nonzero(m2)),), 4, "i64")
    dja.dsetmask_(R, M2, v)
    assert _same(R.collect(), _assigned(y, m2, v))
    dja.dsetmask_(Y, Mr, 0)
    assert _same(Y.collect(), _assigned(y, _kept(q, m), 0))
    for t in (Mr, Y):
        t.close()
    assert dja.bytes_in_use() == before


def _scenario_grids(rank, world, dja):
    seed = 0
    for shape, dist in _grids(world):
        for dtype in ("f64", "i64"):
            seed += 1
            _check(dja, _data(shape, seed, dtype),
                   _mask(shape, 50 + seed, "f64"), dist)
    assert dja.bytes_in_use() == 0


def _scenario_mask_other_layout(rank, world, dja):
    x, m = _data((9, 7), 1, "f64"), _mask((9, 7), 2, "i64")
    _check(dja, x, m, (1, world), (world, 1))
    _check(dja, x, m, (world, 1), (1, world))
    _check(dja, x, m, (1, 1), (1, world))
    if world == 4:
        _check(dja, x, m, (2, 2), (1, 4))
        _check(dja, x, m, (1, 4), (2, 2))
    v, mv = _data((29,), 3, "f32"), _mask((29,), 4, "f32")
    _check(dja, v, mv, (world,), (1,))
    _check(dja, v, mv, (1,), (world,))
    # mismatched dims raise on every rank, before anything moves
    from distributedarrays_jl_amd._ffi import DArrayError
    D, M = dja.distribute(x), dja.distribute(m[:, :6].copy())
    before = dja.bytes_in_use()
    for f in (lambda: dja.dfilter(M, D), lambda: dja.dfindall(M, D),
              lambda: dja.dsetmask_(D, M, 1.0), lambda: D[M],
              lambda: dja.dfilter(np.ones((9, 7)), D)):
        try:
            f()
            assert False, "expected DArrayError"
        except DArrayError:
            pass
    assert dja.bytes_in_use() == before
    assert _same(D.collect(), x)


def _scenario_empty(rank, world, dja):
    n = 10 * world
    x = _data((n,), 1, "f64")
    m = _mask((n,), 2)
    m[:10] = 0                      # rank 0 keeps nothing
    _check(dja, x, m, (world,))
    m[:] = 0                        # nobody keeps anything
    _check(dja, x, m, (world,))
    m[:] = 1                        # everybody keeps everything
    _check(dja, x, m, (world,))
    for shape, dist in _grids(world):
        x = _data(shape, 3, "i64")
        _check(dja, x, np.zeros(shape, order="F"), dist)
        m = np.zeros(shape, order="F")
        m[(-1,) * len(shape)] = 1   # the very last element only
        _check(dja, x, m, dist)
    # an empty array
    _check(dja, np.zeros((0,)), np.zeros((0,)), (world,))
    # assigning where nothing is true changes nothing
    D = dja.distribute(_data((n,), 5, "f64"))
    Z = dja.distribute(np.zeros(n))
    dja.dsetmask_(D, Z, 3.0)
    dja.dsetmask_(D, Z, np.zeros(0))
    assert _same(D.collect(), _data((n,), 5, "f64"))


def _vector_forms(dja, v, world, rank):
    """v as a numpy array, an evenly cut DVector, and DVectors with all of
    it on the last / the first rank."""
    yield v
    yield dja.distribute(v)
    for sizes in ([0] * (world - 1) + [v.size], [v.size] + [0] * (world - 1)):
        V = dja.DArray.from_chunk_sizes(sizes, {np.dtype("float64"): "f64",
                                                np.dtype("int64"): "i64"}[
                                                    v.dtype])
        lo = sum(sizes[:rank])
        V.set_localpart(v[lo:lo + sizes[rank]])
        yield V


def _scenario_setmask(rank, world, dja):
    seed = 0
    for shape, dist in _grids(world):
        for dtype in ("f64", "i64"):
            seed += 1
            x = _data(shape, seed, dtype)
            m = _mask(shape, 70 + seed, "f64" if seed % 2 else "i64")
            M = dja.distribute(m, dist=dist)
            k = int(np.count_nonzero(m))
            # a scalar
            D = dja.distribute(x, dist=dist)
            before = dja.bytes_in_use()
            c = -7 if dtype == "i64" else -0.0
            assert dja.dsetmask_(D, M, c) is D
            assert _same(D.collect(), _assigned(x, m, c)), (shape, dist)
            assert dja.bytes_in_use() == before
            D.close()
            # a vector in every form
            v = _data((k,), 200 + seed, dtype)
            for V in _vector_forms(dja, v, world, rank):
                D = dja.distribute(x, dist=dist)
                before = dja.bytes_in_use()
                dja.dsetmask_(D, M, V)
                assert _same(D.collect(), _assigned(x, m, v)), \
                    (shape, dist, type(V))
                assert dja.bytes_in_use() == before
                assert list(D.idxs) == list(
                    dja.DArray(shape, dtype, dist, _alloc=False).idxs)
                D.close()
                if not isinstance(V, np.ndarray):
                    assert _same(V.collect(), v)
                    V.close()
            # the mask in another layout than the data
            if len(shape) == 2:
                D = dja.distribute(x, dist=dist)
                M2 = dja.distribute(m, dist=dist[::-1])
                dja.dsetmask_(D, M2, v)
                assert _same(D.collect(), _assigned(x, m, v))
                D.close()
                M2.close()
            assert _same(M.collect(), m)
            M.close()
    assert dja.bytes_in_use() == 0
    # D[D] = c: the array is its own mask (in place on the device)
    x = _data((23,), 9, "i64")
    x[::3] = 0
    D = dja.distribute(x)
    dja.dsetmask_(D, D, 5)
    assert _same(D.collect(), _assigned(x, x, 5))
    # i64 scalars beyond 2^53 do not fit the double parameter
    from distributedarrays_jl_amd._ffi import DArrayError
    for bad in ((1 << 53) + 1, 1.5):
        try:
            dja.dsetmask_(D, D, bad)
            assert False, "expected DArrayError"
        except DArrayError:
            pass
    dja.dsetmask_(D, D, 1 << 53)
    assert _same(D.collect(), _assigned(x, x, 1 << 53))


def _scenario_wrong_length(rank, world, dja):
    from distributedarrays_jl_amd._ffi import DArrayError
    for shape, dist in _grids(world):
        x, m = _data(shape, 1, "f64"), _mask(shape, 2)
        k = int(np.count_nonzero(m))
        D, M = dja.distribute(x, dist=dist), dja.distribute(m, dist=dist)
        before = dja.bytes_in_use()
        bad = [np.zeros(k + 1), np.zeros(max(k - 1, 0)) if k else
               np.zeros(2), dja.distribute(np.zeros(k + 2)),
               np.zeros((k, 1)), dja.distribute(np.zeros(k, np.int64)),
               "abc", [1.0] * k]
        for v in bad:
            try:
                dja.dsetmask_(D, M, v)
                assert False, "expected DArrayError for %r" % (v,)
            except DArrayError:
                pass
            if isinstance(v, dja.DArray):
                v.close()
        assert dja.bytes_in_use() == before
        assert _same(D.collect(), x), (shape, dist)
        D.close()
        M.close()
    assert dja.bytes_in_use() == 0


def _scenario_sugar(rank, world, dja):
    from distributedarrays_jl_amd import expr as E
    from distributedarrays_jl_amd._ffi import DArrayError
    for shape, dist in _grids(world):
        x, m = _data(shape, 1, "f64"), _mask(shape, 2)
        k = int(np.count_nonzero(m))
        D, M = dja.distribute(x, dist=dist), dja.distribute(m, dist=dist)
        before = dja.bytes_in_use()
        got = D[M]
        assert isinstance(got, np.ndarray) and _same(got, _kept(x, m))
        assert _same(D[M, ], _kept(x, m))
        # an Expr mask (materialised, then freed) and a predicate; the
        # fake da_expr has no comparisons, so the trees are arithmetic
        assert _same(D[E.ref(M) * E.ref(M)], _kept(x, m))
        R = dja.dfilter(lambda t: t * 0.0 + 1.0, D)
        assert _same(R.collect(), x.ravel(order="F"))
        R.close()
        I = dja.dfindall(E.ref(M) + 0.0)
        assert np.array_equal(I.collect(),
                              np.flatnonzero(m.ravel(order="F")))
        I.close()
        assert dja.bytes_in_use() == before
        D[M] = 2.5
        assert _same(D.collect(), _assigned(x, m, 2.5))
        v = _data((k,), 3, "f64")
        D[M] = v
        assert _same(D.collect(), _assigned(x, m, v))
        V = dja.distribute(v[::-1].copy())
        D[E.ref(M) * 2.0] = V
        assert _same(D.collect(), _assigned(x, m, v[::-1]))
        V.close()
        assert dja.bytes_in_use() == before
        # numpy bool arrays are still not masks
        try:
            D[m != 0]
            assert False, "expected DArrayError"
        except DArrayError:
            pass
        D.close()
        M.close()
    assert dja.bytes_in_use() == 0


SCENARIOS = ["vector_even", "ragged", "grids", "mask_other_layout", "empty",
             "setmask", "wrong_length", "sugar"]


@pytest.mark.timeout(420)
@pytest.mark.parametrize("name", SCENARIOS)
@pytest.mark.parametrize("world", [1, 2, 4])
def test_mask(tmp_path, world, name):
    _spawn(tmp_path, world, name)
