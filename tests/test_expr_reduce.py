"""Fused mapreduce over broadcast trees (expr.reduce / expr.count and the
callable forms of ops.mapreduce / dcount / dall / dany, dvar, dstd) on the
CPU: the hipRTC codegen of every dtype x layout x fold compiles, and the
Python orchestration runs at world sizes 2 and 3 over the fake ABI of
fakelib_reduce.py (numpy numerics; the kernels' bits are the GPU suite's
business)."""
import ctypes
import os

import numpy as np
import pytest
import torch.multiprocessing as mp

from distributedarrays_jl_amd._opcodes import MAP_OP, MAP2_OP


# ------------------------------------------------------------------ codegen
def _dbg():
    from distributedarrays_jl_amd._ffi import lib
    dbg = lib.dbg_expr_reduce_jit_compile
    dbg.argtypes = [ctypes.POINTER(ctypes.c_int32)] + [ctypes.c_int] * 6 + \
        [ctypes.c_char_p, ctypes.c_int]
    dbg.restype = ctypes.c_int
    lib.da_expr_jit_errstr.restype = ctypes.c_char_p
    return lib, dbg


PROG = [(1 << 8) | 0, (0 << 8) | MAP_OP["sin"], (1 << 8) | 1,
        (2 << 8) | 0, (3 << 8) | MAP2_OP["mul"], (3 << 8) | MAP2_OP["add"]]
IPROG = [(1 << 8) | 0, (0 << 8) | MAP_OP["abs"], (1 << 8) | 1,
         (2 << 8) | 0, (3 << 8) | MAP2_OP["mul"], (3 << 8) | MAP2_OP["add"]]
COUNT = -1


@pytest.mark.parametrize("dtype,nd,strided", [(0, 1, 0), (1, 1, 0), (2, 1, 0),
                                              (0, 2, 1), (1, 3, 1), (0, 4, 1)])
def test_reduce_codegen_compiles(dtype, nd, strided):
    """hipRTC is a pure compiler: every fold and the count of each dtype x
    layout row generate source it accepts, with no GPU."""
    lib, dbg = _dbg()
    p = IPROG if dtype == 2 else PROG
    arr = (ctypes.c_int32 * len(p))(*p)
    src = ctypes.create_string_buffer(32768)
    seen = set()
    for rop in (0, 1, 2, 3, COUNT):
        rc = dbg(arr, len(p), dtype, nd, 2, strided, rop, src, 32768)
        assert rc == 0, "dtype %d nd %d strided %d redop %d: %r\n%s" % (
            dtype, nd, strided, rop, lib.da_expr_jit_errstr(),
            src.value.decode()[-1200:])
        text = src.value
        # the fold is a compile-time constant of the source: the JIT cache
        # is keyed by source, so every fold and the count are distinct
        assert text not in seen
        seen.add(text)
        assert b'#include "reduce_core.hpp"' in text
        assert b"da::fanin_finish(" in text and b"da::block_reduce_in(" in text
        if rop == COUNT:
            assert b"int64_t acc" in text
        else:
            assert b"da::red_comb(%d," % rop in text
    # the evaluator is the one of da_expr: shared functor tables by constant
    assert (b"da::apply_map<double>(%d," % MAP_OP["sin"] in text
            or b"da::apply_map<float>(%d," % MAP_OP["sin"] in text
            or b"da::apply_map_i64(%d," % MAP_OP["abs"] in text)


def test_reduce_codegen_rejects_bad_arguments():
    lib, dbg = _dbg()
    arr = (ctypes.c_int32 * len(PROG))(*PROG)
    src = ctypes.create_string_buffer(4096)
    assert dbg(arr, len(PROG), 0, 1, 2, 0, 4, src, 4096) != 0    # redop
    assert dbg(arr, len(PROG), 0, 1, 2, 0, -2, src, 4096) != 0
    assert dbg(arr, len(PROG), 0, 5, 2, 1, 0, src, 4096) != 0    # nd
    assert dbg(arr, len(PROG), 3, 1, 2, 0, 0, src, 4096) != 0    # dtype
    assert dbg(arr, len(PROG), 0, 1, 1, 0, 0, src, 4096) != 0    # arg 1 oob
    assert dbg(arr, len(PROG) - 1, 0, 1, 2, 0, 0, src, 4096) != 0  # 2 left


def test_entry_points_need_init():
    from distributedarrays_jl_amd._ffi import lib
    out = ctypes.c_double()
    cnt = ctypes.c_int64()
    arr = (ctypes.c_int32 * 1)((1 << 8) | 0)
    assert lib.da_expr_reduce(arr, 1, None, 1, None, None, 1, None, 0, 0, 0,
                              0, ctypes.byref(out)) < 0
    assert lib.da_expr_count(arr, 1, None, 1, None, None, 1, None, 0, 0, 0,
                             ctypes.byref(cnt)) < 0


# --------------------------------------------------------------- multi-rank
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
        import distributedarrays_jl_amd as dja
        dja.comm.init()
        globals()["_scenario_" + name](rank, world, dja, fake)
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


def _g(n, seed):
    from oracle import philox
    return philox.fill_uniform_f64(n, seed)


def _set(d, full):
    sl = tuple(slice(lo, hi) for lo, hi in d.lidx)
    d.set_localpart(np.asfortranarray(np.asarray(full)[sl]))
    return d


def _close(a, b, rel=1e-12):
    return abs(a - b) <= rel * max(abs(b), 1e-300)


class _NoLeak:
    """Temporaries of a fused reduction are freed before it returns."""

    def __init__(self, fake):
        self.fake = fake

    def __enter__(self):
        self.before = self.fake.user_bytes

    def __exit__(self, *exc):
        if exc[0] is None:
            assert self.fake.user_bytes == self.before


def _ragged(world, n):
    sizes = [n // world] * world
    sizes[0] += n - sum(sizes) + 3
    sizes[-1] -= 3
    return sizes


def _scenario_vectors(rank, world, dja, fake):
    from distributedarrays_jl_amd import expr as E
    n = 1000
    ga, gb = _g(n, 1) - 0.5, _g(n, 2) + 0.5
    A = _set(dja.DArray((n,), "f64"), ga)
    B = _set(dja.DArray((n,), "f64"), gb)
    with _NoLeak(fake):
        # aligned operands
        assert _close(E.reduce("add", E.ref(A) * E.ref(B)), float(ga @ gb))
        assert E.reduce("max", E.ref(A) - E.ref(B)) == (ga - gb).max()
        assert E.reduce("min", E.abs(E.ref(A))) == np.abs(ga).min()
        assert _close(E.reduce("mul", E.ref(B) * 0.0 + 1.001), 1.001 ** n,
                      1e-10)
        assert E.count(E.ref(A)) == n
        assert E.count(E.sign(E.max2(E.ref(A), 0.0))) == int((ga > 0).sum())
        # aliasing: one operand slot, one read
        prog, args, _ = E.compile_expr(E.ref(A) * E.ref(A))
        assert len(args) == 1
        assert _close(E.reduce("add", E.ref(A) * E.ref(A)), float(ga @ ga))
    # operands with mismatched cuts: localised through the gather
    R = dja.DArray.from_chunk_sizes(_ragged(world, n), "f64")
    _set(R, gb)
    assert not A.samedist(R)
    with _NoLeak(fake):
        assert _close(E.reduce("add", E.ref(A) * E.ref(R)), float(ga @ gb))
        # the ragged array first: its layout is the reduction's
        assert _close(E.reduce("add", E.ref(R) * E.ref(A)), float(ga @ gb))
        assert E.count(E.ref(R) - E.ref(B)) == 0
    # a vector shorter than the world: some ranks hold an empty chunk and
    # contribute the fold identity / a zero count
    short = np.array([3.0, -1.0, 2.0][:max(world - 1, 1)])
    sizes = [0] * world
    sizes[0] = short.size - (1 if short.size > 1 else 0)
    sizes[-1] += short.size - sizes[0]
    S = dja.DArray.from_chunk_sizes(sizes, "f64")
    _set(S, short)
    assert 0 in sizes or world == 1
    with _NoLeak(fake):
        assert E.reduce("min", E.ref(S) * 2.0) == 2.0 * short.min()
        assert E.reduce("max", E.ref(S) * 2.0) == 2.0 * short.max()
        assert E.reduce("add", E.ref(S) * 2.0) == 2.0 * short.sum()
        assert E.reduce("mul", E.ref(S) * 2.0) == np.prod(2.0 * short)
        assert E.count(E.ref(S)) == short.size
    T = _set(dja.DArray((world - 1,), "f64"), short[:world - 1])
    assert E.reduce("add", E.ref(T)) == short[:world - 1].sum()
    assert E.count(E.ref(T) - 5.0) == world - 1
    for d in (A, B, R, S, T):
        d.close()


def _scenario_matrices(rank, world, dja, fake):
    from distributedarrays_jl_amd import expr as E
    nr, nc = 12, 4 * world
    g = _g(nr * nc, 20).reshape((nr, nc), order="F")
    X = _set(dja.DArray((nr, nc), "f64", (1, world)), g)
    # a (1, n) and an (m, 1) singleton operand against the full shape
    M = dja.dmean_dims(X, (0,))                       # (1, nc)
    gcol = _g(nr, 21).reshape((nr, 1), order="F")
    C = _set(dja.DArray((nr, 1), "f64", (1, 1)), gcol)
    mean0 = g.mean(axis=0, keepdims=True)
    with _NoLeak(fake):
        got = E.reduce("add", E.abs2(E.ref(X) - E.ref(M)))
        assert _close(got, float(((g - mean0) ** 2).sum()))
        got = E.reduce("max", E.ref(X) * E.ref(C) - E.ref(M))
        assert _close(got, float((g * gcol - mean0).max()))
        assert E.count(E.sign(E.max2(E.ref(X) - E.ref(C), 0.0))) == \
            int((g > gcol).sum())
    # a full-shape operand cut the other way (row split vs column split)
    Y = _set(dja.DArray((nr, nc), "f64", (world, 1)), g)
    with _NoLeak(fake):
        assert _close(E.reduce("add", E.ref(X) * E.ref(Y)),
                      float((g * g).sum()))
    # row .+ column: no operand has the full shape, the domain is the
    # default grid for (nr, nc) and nothing of that shape is allocated
    grow = _g(nc, 22).reshape((1, nc), order="F")
    R = _set(dja.DArray((1, nc), "f64", (1, world)), grow)
    with _NoLeak(fake):
        before = set(fake.bufs)
        got = E.reduce("add", E.ref(C) * E.ref(R) + 1.0)
        assert _close(got, float((gcol * grow + 1.0).sum()))
        assert E.reduce("min", E.ref(R) + E.ref(C)) == (grow + gcol).min()
        assert E.count(E.ref(R) + E.ref(C)) == nr * nc
        assert set(fake.bufs) == before
    # 3-D with a (n0, 1, n2) operand
    g3 = _g(5 * 4 * 3 * world, 23).reshape((5, 4, 3 * world), order="F")
    A3 = _set(dja.DArray((5, 4, 3 * world), "f64", (1, 1, world)), g3)
    gs = _g(5 * 3 * world, 24).reshape((5, 1, 3 * world), order="F")
    S3 = _set(dja.DArray((5, 1, 3 * world), "f64", (1, 1, world)), gs)
    with _NoLeak(fake):
        assert _close(E.reduce("add", E.ref(A3) * E.ref(S3)),
                      float((g3 * gs).sum()))
    for d in (X, M, C, Y, R, A3, S3):
        d.close()


def _scenario_ops(rank, world, dja, fake):
    from distributedarrays_jl_amd import expr as E
    from distributedarrays_jl_amd._ffi import DArrayError
    n = 501
    ga, gb = _g(n, 30) - 0.25, _g(n, 31)
    A = _set(dja.DArray((n,), "f64"), ga)
    B = _set(dja.DArray((n,), "f64"), gb)
    # callable f: mapreduce(t -> t*t, +, D) and mapreduce(f, op, A, B)
    fake.calls.clear()
    assert _close(dja.mapreduce(lambda t: t * t, "add", A), float(ga @ ga))
    assert _close(dja.mapreduce(lambda a, b: a * b, "add", A, B),
                  float(ga @ gb))
    assert dja.mapreduce(lambda a, b: E.max2(a, b), "min", A, B) == \
        np.maximum(ga, gb).min()
    assert fake.calls == ["da_expr_reduce"] * 3
    # a string f keeps today's path
    fake.calls.clear()
    assert _close(dja.mapreduce("abs2", "add", A), float(ga @ ga))
    assert fake.calls == ["da_reduce"]
    fake.calls.clear()
    assert dja.dcount("nonzero", A) == n
    assert fake.calls == ["da_count"]
    with pytest.raises(DArrayError):
        dja.mapreduce("abs2", "add", A, B)
    with pytest.raises(DArrayError):
        dja.mapreduce(lambda t: 1.0, "add", A)
    # callable predicates, composed from the op tables: x > 0
    pos = lambda x: E.sign(E.max2(x, 0.0))
    fake.calls.clear()
    assert dja.dcount(pos, A) == int((ga > 0).sum())
    assert fake.calls == ["da_expr_count"]
    assert dja.dall(pos, A) is False and dja.dany(pos, A) is True
    assert dja.dall(pos, B) is bool((gb > 0).all())
    assert dja.dany(lambda x: E.sign(E.max2(x - 2.0, 0.0)), B) is False
    empty = dja.DArray((0,), "f64")
    assert dja.dall(pos, empty) is True and dja.dany(pos, empty) is False
    assert dja.dall("nonzero", A) == bool(np.all(ga != 0))
    # dvar / dstd: two passes, no temporary
    with _NoLeak(fake):
        assert _close(dja.dvar(A), float(np.var(ga, ddof=1)))
        assert _close(dja.dvar(A, corrected=False), float(np.var(ga)))
        assert _close(dja.dstd(A), float(np.std(ga, ddof=1)))
        assert _close(dja.dstd(A, corrected=False), float(np.std(ga)))
    g32 = ga.astype(np.float32)
    A32 = _set(dja.DArray((n,), "f32"), g32)
    assert _close(dja.dvar(A32), float(np.var(g32.astype(np.float64),
                                              ddof=1)), 1e-4)
    # i64: exact folds; float-only ops and non-integer constants raise
    gi = np.rint(ga * 100).astype(np.int64)
    I = _set(dja.DArray((n,), "i64"), gi)
    assert E.reduce("add", E.ref(I) * E.ref(I) + 3) == int((gi * gi + 3).sum())
    assert E.reduce("max", E.abs(E.ref(I))) == int(np.abs(gi).max())
    assert E.count(E.ref(I)) == int(np.count_nonzero(gi))
    assert isinstance(E.reduce("add", E.ref(I)), int)
    with pytest.raises(DArrayError):
        E.reduce("add", E.sin(E.ref(I)))
    with pytest.raises(DArrayError):
        E.reduce("add", E.ref(I) * 0.5)
    with pytest.raises(DArrayError):
        dja.dvar(I)
    # no DArray operand; unknown fold; mixed dtypes; shape mismatch
    with pytest.raises(DArrayError):
        E.reduce("add", E.lit(1.0) + 2.0)
    with pytest.raises(DArrayError):
        E.count(3.0)
    with pytest.raises(DArrayError):
        E.reduce("sub", E.ref(A))
    with pytest.raises(DArrayError):
        E.reduce("add", E.ref(A) * E.ref(A32))
    bad = dja.DArray((n - 1,), "f64")
    with pytest.raises(DArrayError):
        E.reduce("add", E.ref(A) + E.ref(bad))
    # seven distinct operands
    many = [dja.DArray((8,), "f64") for _ in range(7)]
    e = E.ref(many[0])
    for d in many[1:]:
        e = e + E.ref(d)
    with pytest.raises(DArrayError):
        E.reduce("add", e)
    for d in [A, B, empty, A32, I, bad] + many:
        d.close()


@pytest.mark.timeout(420)
@pytest.mark.parametrize("name", ["vectors", "matrices", "ops"])
@pytest.mark.parametrize("world", [2, 3])
def test_multirank(tmp_path, world, name):
    _spawn(tmp_path, world, name)
