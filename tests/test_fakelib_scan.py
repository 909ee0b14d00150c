"""daccumulate / dcumsum / dcumprod / dcummax / dcummin at world sizes 1, 2
and 4: the REAL orchestration code (ops.daccumulate_: line totals, the
grouped exchange along a grid line, the ascending left fold into the
carry) over the fakelib ABI (numpy chunks + gloo, see fakelib.py), with a
numpy da_scan added to the installed FakeLib instance from this file.
Every expected value is numpy's ufunc.accumulate along the axis of the
Fortran-ordered host array; all data is exact under any bracketing (i64
wraps, f64 holds integers / powers of two), so every comparison is
array_equal.  Every scenario ends with d_closeall() and a zero-leak
check."""
import os

import numpy as np
import pytest
import torch.multiprocessing as mp

_UFUNC = {"add": np.add, "mul": np.multiply, "min": np.minimum,
          "max": np.maximum}


# ---------------------------------------------------- numpy da_scan (fake)
def _fake_scan(redop, dst, src, inner, axis, outer, dtype, carry):
    import fakelib
    dt = fakelib._NPDT[int(dtype)]
    inner, axis, outer = int(inner), int(axis), int(outer)
    n = inner * axis * outer
    if n == 0:
        return 0
    assert fakelib._addr(dst) and fakelib._addr(src)
    f = _UFUNC[fakelib._REDOP_NAMES[int(redop)]]
    x = fakelib._tv(src, n, dt).reshape((inner, axis, outer),
                                        order="F").copy()
    with np.errstate(over="ignore"):
        r = f.accumulate(x, axis=1)
        if fakelib._addr(carry):
            c = fakelib._tv(carry, inner * outer, dt).reshape(
                (inner, 1, outer), order="F")
            r = f(c, r)
    fakelib._tv(dst, n, dt)[:] = np.asfortranarray(r).ravel(order="F")
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
        fake.da_scan = _fake_scan
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
def _host(shape, seed, dtype, op):
    """Data whose scan is exact in any bracketing."""
    rng = np.random.default_rng(seed)
    if dtype == "i64":
        # any bits: add and mul wrap mod 2^64 on both sides
        return np.asfortranarray(
            rng.integers(-2 ** 62, 2 ** 62, shape, dtype=np.int64))
    if op == "mul":
        # +-2^e, e in {-1, 0, 1}: every prefix is a power of two far
        # inside the exponent range at these sizes
        e = rng.integers(-1, 2, shape)
        s = rng.integers(0, 2, shape) * 2 - 1
        return np.asfortranarray(s * np.exp2(e))
    return np.asfortranarray(rng.integers(-8, 9, shape).astype(np.float64))


def _expect(op, g, dims, init=None):
    with np.errstate(over="ignore"):
        r = _UFUNC[op].accumulate(g, axis=dims)
        if init is not None:
            r = _UFUNC[op](g.dtype.type(init), r)
    return r


def _grids(world):
    """(shape, dist) pairs whose chunk count fits the world."""
    allg = [((23,), (1,)), ((23,), (2,)), ((23,), (4,)),
            ((9, 7), (2, 2)), ((9, 7), (1, 4)), ((9, 7), (4, 1)),
            ((9, 7), (1, 2)), ((9, 7), (2, 1)), ((9, 7), (1, 1)),
            ((5, 4, 6), (2, 1, 2)), ((5, 4, 6), (1, 2, 1)),
            ((3,), (4,)),          # fewer elements than ranks: empty chunks
            ((3, 2), (4, 1)), ((2, 3), (1, 4))]
    return [(s, d) for s, d in allg if int(np.prod(d)) <= world]


# ------------------------------------------------------------ scenarios
def _scenario_all_ops(rank, world, dja):
    wrap = {"add": dja.dcumsum, "mul": dja.dcumprod, "max": dja.dcummax,
            "min": dja.dcummin}
    seed = 0
    for shape, dist in _grids(world):
        for dtype in ("i64", "f64"):
            for op in ("add", "mul", "min", "max"):
                seed += 1
                g = _host(shape, seed, dtype, op)
                D = dja.distribute(g, dist=dist)
                for dims in range(len(shape)):
                    R = wrap[op](D, dims)
                    assert R.dims == D.dims and R.dist == D.dist
                    assert R.ranks == D.ranks and R.dtype == D.dtype
                    assert list(R.idxs) == list(D.idxs)
                    got = R.collect()
                    assert np.array_equal(got, _expect(op, g, dims)), \
                        (shape, dist, dtype, op, dims)
                    R.close()
                # the source is untouched
                assert np.array_equal(D.collect(), g)
                D.close()
    assert dja.bytes_in_use() == 0


def _scenario_default_dist_and_1d(rank, world, dja):
    # default distribution; dims may be omitted for a vector only
    g = _host((41,), 101, "i64", "add")
    D = dja.distribute(g)
    R = dja.dcumsum(D)
    assert np.array_equal(R.collect(), _expect("add", g, 0))
    R2 = dja.daccumulate("max", D, dims=(0,))
    assert np.array_equal(R2.collect(), _expect("max", g, 0))
    m = _host((10, 12), 102, "f64", "add")
    M = dja.distribute(m)
    for dims in (0, 1):
        R3 = dja.daccumulate("add", M, dims)
        assert np.array_equal(R3.collect(), _expect("add", m, dims))
        R3.close()


def _scenario_init(rank, world, dja):
    big = (1 << 53)
    for shape, dist in _grids(world):
        for dtype, op, init in (("i64", "add", -7), ("i64", "max", 5),
                                ("i64", "add", big), ("f64", "add", 3.0),
                                ("f64", "mul", -2.0), ("f64", "min", -1.0)):
            g = _host(shape, 7 + len(shape), dtype, op)
            D = dja.distribute(g, dist=dist)
            for dims in range(len(shape)):
                R = dja.daccumulate(op, D, dims, init=init)
                assert np.array_equal(R.collect(),
                                      _expect(op, g, dims, init)), \
                    (shape, dist, dtype, op, dims, init)
                R.close()
            D.close()
    assert dja.bytes_in_use() == 0
    from distributedarrays_jl_amd._ffi import DArrayError
    D = dja.distribute(_host((8,), 1, "i64", "add"))
    for bad in ((1 << 53) + 1, 1.5):
        try:
            dja.daccumulate("add", D, init=bad)
            assert False, "expected DArrayError (i64 init)"
        except DArrayError:
            pass
    D.close()
    assert dja.bytes_in_use() == 0


def _scenario_inplace(rank, world, dja):
    for shape, dist in _grids(world):
        g = _host(shape, 31, "i64", "mul")
        for dims in range(len(shape)):
            D = dja.distribute(g, dist=dist)
            before = dja.bytes_in_use()
            out = dja.daccumulate_("mul", D, D, dims)       # dest is src
            assert out is D
            assert dja.bytes_in_use() == before
            assert np.array_equal(D.collect(), _expect("mul", g, dims))
            # accumulate! into another array of the same layout, with init
            E = D.similar()
            dja.daccumulate_("min", E, D, dims, init=0)
            assert np.array_equal(E.collect(),
                                  _expect("min", _expect("mul", g, dims),
                                          dims, 0))
            E.close()
            D.close()
    assert dja.bytes_in_use() == 0


def _scenario_errors(rank, world, dja):
    from distributedarrays_jl_amd._ffi import DArrayError
    m = _host((8, 6), 5, "f64", "add")
    M = dja.distribute(m, dist=(1, world))
    N = dja.distribute(m, dist=(world, 1))
    F = dja.distribute(m.astype(np.float32), dist=(1, world))
    S = dja.distribute(m[:, :5].copy(), dist=(1, world))
    before = dja.bytes_in_use()

    def raises(f):
        try:
            f()
        except DArrayError:
            return True
        return False

    # N-D without dims (Julia: accumulate of a matrix needs dims)
    assert raises(lambda: dja.dcumsum(M))
    assert raises(lambda: dja.daccumulate("add", M))
    assert raises(lambda: dja.daccumulate_("add", M, M))
    # layout / dtype / shape mismatch between dest and src
    if world > 1:
        assert raises(lambda: dja.daccumulate_("add", N, M, 0))
    assert raises(lambda: dja.daccumulate_("add", F, M, 0))
    assert raises(lambda: dja.daccumulate_("add", S, M, 0))
    # bad op / dims
    assert raises(lambda: dja.daccumulate("sub", M, 0))
    assert raises(lambda: dja.daccumulate("add", M, 2))
    assert raises(lambda: dja.daccumulate("add", M, -1))
    assert raises(lambda: dja.daccumulate("add", M, (0, 1)))
    # nothing leaked by the failures
    assert dja.bytes_in_use() == before
    # non-identity owners (a dims-reduction's result lives on the
    # lowest-coordinate slab owners)
    if world > 1:
        R = dja.dsum_dims(dja.distribute(m, dist=(1, world)), (0,))
        Q = dja.DArray((world,), "f64", (world,),
                       ranks=list(range(world))[::-1])
        assert raises(lambda: dja.dcumsum(Q))
        assert np.array_equal(dja.dcumsum(R, 1).collect(),
                              _expect("add", m.sum(axis=0, keepdims=True),
                                      1))
    # and everything is still in step
    assert np.array_equal(dja.dcumsum(M, 1).collect(), _expect("add", m, 1))


SCENARIOS = ["all_ops", "default_dist_and_1d", "init", "inplace", "errors"]


@pytest.mark.timeout(420)
@pytest.mark.parametrize("name", SCENARIOS)
@pytest.mark.parametrize("world", [1, 2, 4])
def test_scan(tmp_path, world, name):
    _spawn(tmp_path, world, name)
