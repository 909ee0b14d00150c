"""expr.reduce / expr.count with dims, mapreduce(callable, dims=), dvar_dims,
dstd_dims and dcount_dims at world sizes 1, 2 and 4: the REAL orchestration
(domain, localisation, the one da_expr_reduce_dims call per rank, result
placement, the slab exchange and ascending-rank fold shared with
dreduce_dims) over the fakelib ABI, with a numpy da_expr_reduce_dims added
to the installed instance from this file.  Numerics are numpy's, so float
sums are compared within a few roundings and everything else exactly;
expected values are numpy on the collected host arrays.  Every scenario ends
with d_closeall() and a zero-leak check."""
import ctypes
import os

import numpy as np
import pytest
import torch.multiprocessing as mp


# ------------------------------------------- numpy da_expr_reduce_dims
def _make_fake_reduce_dims(fake):
    import fakelib
    from expr_dims_ref import evaluate as _evaluate

    def da_expr_reduce_dims(prog, plen, dims, nd, srcs, src_strides, nsrcs,
                            consts, nconsts, dtype, mask, redop, dst):
        fake.calls.append("da_expr_reduce_dims")
        dt = fakelib._NPDT[int(dtype)]
        nd, mask, redop = int(nd), int(mask), int(redop)
        nsrcs, nconsts = int(nsrcs), int(nconsts)
        dv = ctypes.cast(dims, ctypes.POINTER(ctypes.c_uint64))
        shape = tuple(int(dv[d]) for d in range(nd))
        assert 1 <= nd <= 4 and mask >> nd == 0
        axes = tuple(d for d in range(nd) if (mask >> d) & 1)
        kshape = tuple(1 if d in axes else shape[d] for d in range(nd))
        K = int(np.prod(kshape))
        if K == 0:
            return 0
        assert fakelib._addr(dst)
        n = int(np.prod(shape))
        if n:
            pv = ctypes.cast(prog, ctypes.POINTER(ctypes.c_int32))
            program = [int(pv[i]) for i in range(int(plen))]
            cv = ctypes.cast(consts, ctypes.POINTER(ctypes.c_double))
            cc = [float(cv[i]) for i in range(nconsts)]
            sv = ctypes.cast(srcs, ctypes.POINTER(ctypes.c_void_p))
            if fakelib._addr(src_strides):
                stv = ctypes.cast(src_strides,
                                  ctypes.POINTER(ctypes.c_uint64))
                strides = [[int(stv[i * nd + d]) for d in range(nd)]
                           for i in range(nsrcs)]
            else:
                dense = [int(np.prod(shape[:d])) for d in range(nd)]
                strides = [dense] * nsrcs
            args = [np.lib.stride_tricks.as_strided(
                fakelib._tv(sv[i], 1, dt), shape=shape,
                strides=tuple(s * dt.itemsize for s in ss))
                for i, ss in enumerate(strides)]
            t = np.broadcast_to(_evaluate(program, args, cc, dt), shape)
        else:
            t = np.zeros(shape, dtype=dt)
        if redop == -1:
            res = np.count_nonzero(t, axis=axes, keepdims=True).astype(
                np.int64)
        else:
            op = fakelib._REDOP_NAMES[redop]
            if dt.kind == "i":
                info = np.iinfo(np.int64)
                ident = {"add": 0, "mul": 1, "min": info.max,
                         "max": info.min}[op]
            else:
                ident = {"add": 0.0, "mul": 1.0, "min": np.inf,
                         "max": -np.inf}[op]
            f = {"add": np.add, "mul": np.multiply, "min": np.minimum,
                 "max": np.maximum}[op]
            with np.errstate(over="ignore"):
                res = f.reduce(t, axis=axes, keepdims=True, dtype=dt,
                               initial=dt.type(ident))
        assert res.shape == kshape
        fakelib._tv(dst, K, res.dtype)[:] = res.ravel(order="F")
        return 0

    return da_expr_reduce_dims


# ------------------------------------------------------- spawn plumbing
def _run_scenario(rank, tmpfile, q, world, name):
    try:
        os.environ["RANK"] = str(rank)
        os.environ["WORLD_SIZE"] = str(world)
        os.environ["MASTER_ADDR"] = "127.0.0.1"
        import torch.distributed as td
        td.init_process_group("gloo", init_method="file://%s" % tmpfile,
                              rank=rank, world_size=world)
        import fakelib_reduce
        fake = fakelib_reduce.install()
        fake.da_expr_reduce_dims = _make_fake_reduce_dims(fake)
        import distributedarrays_jl_amd as dja
        dja.comm.init()
        globals()["_scenario_" + name](rank, world, dja, fake)
        dja.d_closeall()
        assert fake.user_bytes == 0, \
            "leaked %d bytes of ABI allocations" % fake.user_bytes
        q.put((rank, True, None))
    except Exception:
        import traceback
        q.put((rank, False, traceback.format_exc()[-3000:]))
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
def _data(shape, seed, dtype="f64"):
    rng = np.random.default_rng(seed)
    if dtype == "i64":
        x = rng.integers(-9, 10, shape, dtype=np.int64)
    else:
        x = (rng.random(shape) - 0.5).astype(
            {"f64": np.float64, "f32": np.float32}[dtype])
    return np.asfortranarray(x)


def _grid2(world):
    """2-D grids of exactly `world` chunks."""
    return {1: [(1, 1)], 2: [(2, 1), (1, 2)],
            4: [(4, 1), (1, 4), (2, 2)]}[world]


def _owners(dja, dist, dims):
    """Ranks that own a result chunk: reduced grid coordinates 0."""
    out = []
    for r in range(int(np.prod(dist))):
        pos = dja.geometry.grid_pos(r, dist)
        if all(pos[a] == 0 for a in dims):
            out.append(r)
    return out


def _check_result(dja, R, want, dist, dims, rank, exact):
    nd = len(dist)
    assert R.dims == want.shape, (R.dims, want.shape)
    assert R.dist == tuple(1 if a in dims else dist[a] for a in range(nd))
    assert list(R.ranks) == _owners(dja, dist, dims)
    # a rank that is no owner holds no result chunk
    assert (R.lchunk is not None) == (rank in R.ranks)
    got = R.collect()
    assert got.dtype == want.dtype
    if exact:
        assert np.array_equal(got, want), (got, want)
    else:
        assert np.allclose(got, want, rtol=1e-12, atol=1e-13), (got, want)


def _closing(dja, before, *ds):
    for d in ds:
        d.close()
    assert dja.bytes_in_use() == before


# ------------------------------------------------------------ scenarios
def _scenario_grid2d(rank, world, dja, fake):
    """Every 2-D grid of the world: the reduced dim split across ranks
    (slabs exchanged), not split, and both dims reduced."""
    from distributedarrays_jl_amd import expr as E
    x, y = _data((9, 7), 1), _data((9, 7), 2)
    for dist in _grid2(world):
        X, Y = dja.distribute(x, dist=dist), dja.distribute(y, dist=dist)
        before = dja.bytes_in_use()
        for dims in ((0,), (1,), (0, 1), 0, [1, 1, 0]):
            nd = dja.ops._norm_dims("t", dims, 2)
            fake.calls.clear()
            R = E.reduce("add", E.abs2(E.ref(X) - E.ref(Y)) + 0.25,
                         dims=dims)
            # one fused call per rank with a chunk, no per-axis kernel
            assert fake.calls.count("da_expr_reduce_dims") == 1
            assert "da_reduce" not in fake.calls
            want = ((x - y) ** 2 + 0.25).sum(axis=nd, keepdims=True)
            _check_result(dja, R, want, dist, nd, rank, False)
            Rm = E.reduce("max", E.ref(X) * E.ref(Y), dims=dims)
            _check_result(dja, Rm, (x * y).max(axis=nd, keepdims=True),
                          dist, nd, rank, True)
            _closing(dja, before, R, Rm)
        X.close()
        Y.close()
    assert dja.bytes_in_use() == 0


def _scenario_three_d(rank, world, dja, fake):
    """A 3-D array reduced over two dims, with a singleton-dim operand."""
    from distributedarrays_jl_amd import expr as E
    dist = {1: (1, 1, 1), 2: (2, 1, 1), 4: (2, 1, 2)}[world]
    a, s = _data((5, 4, 6), 3), _data((5, 1, 6), 4)
    A, S = dja.distribute(a, dist=dist), dja.distribute(
        s, dist=(dist[0], 1, dist[2]))
    before = dja.bytes_in_use()
    for dims in ((0, 2), (1, 2), (1,), (0, 1, 2)):
        R = E.reduce("add", E.abs2(E.ref(A) - E.ref(S)), dims=dims)
        _check_result(dja, R, ((a - s) ** 2).sum(axis=dims, keepdims=True),
                      dist, dims, rank, False)
        R.close()
    ai = _data((5, 4, 6), 5, "i64")
    AI = dja.distribute(ai, dist=dist)
    for op, f in (("add", np.add), ("mul", np.multiply),
                  ("min", np.minimum), ("max", np.maximum)):
        R = E.reduce(op, abs(E.ref(AI)) * 3 + E.ref(AI), dims=(0, 2))
        with np.errstate(over="ignore"):
            want = f.reduce(np.abs(ai) * 3 + ai, axis=(0, 2), keepdims=True)
        _check_result(dja, R, want, dist, (0, 2), rank, True)
        R.close()
    AI.close()
    assert dja.bytes_in_use() == before


def _scenario_mismatched_cuts(rank, world, dja, fake):
    """An operand cut differently from the domain goes through gather_box,
    for floats and (its own index decode) for i64."""
    from distributedarrays_jl_amd import expr as E
    for dtype in ("f64", "i64"):
        x, y = _data((9, 7), 6, dtype), _data((9, 7), 7, dtype)
        r = _data((1, 7), 8, dtype)
        X = dja.distribute(x, dist=(world, 1))
        Y = dja.distribute(y, dist=(1, world))
        Rw = dja.distribute(r, dist=(1, 1))
        before = dja.bytes_in_use()
        for dims in ((0,), (1,)):
            R = E.reduce("add", E.ref(X) * E.ref(Y) + E.ref(Rw), dims=dims)
            _check_result(dja, R, (x * y + r).sum(axis=dims, keepdims=True),
                          (world, 1), dims, rank, dtype == "i64")
            R.close()
        assert dja.bytes_in_use() == before
        # row .* column: no operand has the domain's shape
        c = _data((9, 1), 9, dtype)
        C = dja.distribute(c, dist=(1, 1))
        R = E.reduce("max", E.ref(Rw) * E.ref(C), dims=(0,))
        assert np.array_equal(R.collect(), (r * c).max(axis=0,
                                                       keepdims=True))
        for t in (R, C, X, Y, Rw):
            t.close()
    assert dja.bytes_in_use() == 0


def _scenario_few_chunks(rank, world, dja, fake):
    """Fewer chunks than ranks, empty chunks and empty extents: ranks that
    own no chunk of the domain or of the result take part all the same."""
    from distributedarrays_jl_amd import expr as E
    x = _data((3, 2), 10)
    X = dja.distribute(x, dist=(1, 1))            # rank 0 only
    R = E.reduce("add", E.ref(X) * 2.0, dims=(0,))
    assert np.allclose(R.collect(), (2 * x).sum(axis=0, keepdims=True))
    assert (R.lchunk is not None) == (rank == 0)
    R.close()
    X.close()
    x = _data((3, 5), 11)
    X = dja.distribute(x, dist=(world, 1))        # world 4: an empty chunk
    for dims in ((0,), (1,)):
        R = E.reduce("min", E.ref(X), dims=dims)
        assert np.array_equal(R.collect(), x.min(axis=dims, keepdims=True))
        C = E.count(E.ref(X) > 0.0, dims=dims)
        assert C.dtype == "i64"
        assert np.array_equal(C.collect(),
                              (x > 0).sum(axis=dims, keepdims=True))
        R.close()
        C.close()
    X.close()
    # a reduced extent of 0: the identity / zero counts; no outputs: empty
    z = np.zeros((0, 4), order="F")
    Z = dja.distribute(z, dist=(1, 1))
    R = E.reduce("max", E.ref(Z), dims=(0,))
    assert np.array_equal(R.collect(), np.full((1, 4), -np.inf))
    C = E.count(E.ref(Z), dims=0)
    assert np.array_equal(C.collect(), np.zeros((1, 4), np.int64))
    E0 = E.reduce("add", E.ref(Z), dims=(1,))
    assert E0.dims == (0, 1) and E0.collect().shape == (0, 1)
    for t in (R, C, E0, Z):
        t.close()
    assert dja.bytes_in_use() == 0


def _scenario_public_names(rank, world, dja, fake):
    """dvar_dims / dstd_dims / dcount_dims / mapreduce(callable, dims=)."""
    from distributedarrays_jl_amd._ffi import DArrayError
    x = _data((9, 7), 12)
    for dist in _grid2(world):
        X = dja.distribute(x, dist=dist)
        before = dja.bytes_in_use()
        for dims in ((0,), (1,), (0, 1)):
            for corrected in (True, False):
                V = dja.dvar_dims(X, dims, corrected)
                want = x.var(axis=dims, keepdims=True,
                             ddof=1 if corrected else 0)
                _check_result(dja, V, want, dist, dims, rank, False)
                V.close()
            S = dja.dstd_dims(X, dims)
            assert np.allclose(S.collect(),
                               x.std(axis=dims, keepdims=True, ddof=1),
                               rtol=1e-12)
            C = dja.dcount_dims(lambda t: t > 0.1, X, dims)
            _check_result(dja, C, (x > 0.1).sum(axis=dims, keepdims=True)
                          .astype(np.int64), dist, dims, rank, True)
            N = dja.dcount_dims("nonzero", X, dims)
            assert np.array_equal(N.collect(), np.count_nonzero(
                x, axis=dims, keepdims=True))
            M = dja.mapreduce(lambda t: t * t, "add", X, dims=dims)
            _check_result(dja, M, (x * x).sum(axis=dims, keepdims=True),
                          dist, dims, rank, False)
            fake.calls.clear()
            P = dja.mapreduce("abs2", "add", X, dims=dims)   # a name:
            assert "da_expr_reduce_dims" not in fake.calls   # dreduce_dims
            assert np.allclose(P.collect(), M.collect(), rtol=1e-12)
            _closing(dja, before, S, C, N, M, P)
        # one sample, corrected: the denominator is 0
        one = dja.distribute(x[:1, :].copy(), dist=(1, 1))
        V = dja.dvar_dims(one, (0,))
        assert np.isnan(V.collect()).all() and V.dims == (1, 7)
        V.close()
        one.close()
        for bad in ((2,), (-1,), (0, 5)):
            for f in (lambda: dja.dvar_dims(X, bad),
                      lambda: dja.dcount_dims("nonzero", X, bad),
                      lambda: dja.mapreduce(lambda t: t, "add", X, dims=bad)):
                try:
                    f()
                    assert False, "expected DArrayError"
                except DArrayError:
                    pass
        assert dja.bytes_in_use() == before
        XI = dja.distribute(_data((9, 7), 13, "i64"), dist=dist)
        try:
            dja.dvar_dims(XI, 0)
            assert False, "expected DArrayError"
        except DArrayError:
            pass
        XI.close()
        X.close()
    assert dja.bytes_in_use() == 0


SCENARIOS = ["grid2d", "three_d", "mismatched_cuts", "few_chunks",
             "public_names"]


@pytest.mark.timeout(420)
@pytest.mark.parametrize("name", SCENARIOS)
@pytest.mark.parametrize("world", [1, 2, 4])
def test_expr_dims(tmp_path, world, name):
    _spawn(tmp_path, world, name)
