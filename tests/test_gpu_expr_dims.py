"""The fused dims-reductions over broadcast trees on the GPU
(da_expr_reduce_dims behind expr.reduce / expr.count with dims, dvar_dims,
dcount_dims, dall_dims, dany_dims), one rank.

Expected values: the program's terms from the oracle on the host copies
(expr_dims_ref.evaluate), reduced along the axes; per output element min,
max, every i64 fold and every count are exact, a float sum obeys
|got - fsum(t)| <= 1.01 (N-1) u sum|t| (true of any summation order, so it
needs no knowledge of the schedule) and a float product
|got/exact - 1| <= 1.01 N u (expr_dims_ref.check_fold).

Shapes are the smallest at which each piece can go wrong: (33, 7) — a
leading extent that is a multiple of nothing — with row and column
operands, (5, 4, 3) and (3, 2, 5, 4) with interleaved kept and reduced
dims, 257 terms across a wave and a 256-thread block with a tail under both
schedules, and one shape at each side of every selector threshold
(schedule, wave/block, split on/off, grid cap), asserted through
dbg_expr_dims_variant before the launch."""
import ctypes
import os

import numpy as np
import pytest

import expr_dims_ref as ref
import kernel_ref as kr
from distributedarrays_jl_amd import expr as E

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dja():
    import distributedarrays_jl_amd as dja
    dja.comm.init()
    return dja


@pytest.fixture(autouse=True)
def no_leak(dja):
    before = dja.bytes_in_use()
    yield
    assert dja.bytes_in_use() == before, "HBM leak"


class Pool:
    """DArrays of a test with their host copies; closes them all."""

    def __init__(self, dja):
        self.dja, self.ds, self.host = dja, [], {}

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        for d in self.ds:
            d.close()

    def mk(self, arr):
        d = self.dja.distribute(np.asfortranarray(arr))
        self.ds.append(d)
        self.host[id(d)] = np.asarray(arr)
        return d

    def own(self, d, host=None):
        self.ds.append(d)
        if host is not None:
            self.host[id(d)] = host
        return d

    def terms(self, e, dt):
        """The oracle's values of the tree, in the broadcast shape."""
        prog, args, consts = E.compile_expr(e)
        hs = [self.host[id(a)] for a in args]
        t = ref.evaluate(prog, hs, consts, kr.NP[dt])
        return np.broadcast_to(t, np.broadcast_shapes(*[h.shape
                                                        for h in hs]))

    def fold(self, op, e, dims, dt, tag, integral=False):
        """One fused fold (op None: count) checked against the oracle;
        returns the device's values."""
        R = E.count(e, dims=dims) if op is None else \
            E.reduce(op, e, dims=dims)
        try:
            got = R.localpart()
            assert R.dtype == ("i64" if op is None else dt)
        finally:
            R.close()
        axes = (dims,) if isinstance(dims, int) else tuple(dims)
        ref.check_fold(got, self.terms(e, dt), axes, op, (tag, op, dims),
                       integral)
        return got


def inputs(shape, dt, seed):
    """Both signs for floats; small integers for i64."""
    n = int(np.prod(shape))
    x = kr.uniform(n, dt, seed)
    if dt != "i64":
        x = x - kr.NP[dt].type(0.5)
    return x.reshape(shape, order="F")


def ints(shape, dt, seed, bound=8):
    """Integer-valued data of any dtype: every sum of them is exact."""
    n = int(np.prod(shape))
    return kr.small_ints(n, seed, bound).astype(kr.NP[dt]).reshape(
        shape, order="F")


def variant(shape, dims):
    from distributedarrays_jl_amd import _ffi
    arr = (ctypes.c_uint64 * len(shape))(*shape)
    nb, gx = ctypes.c_uint32(), ctypes.c_uint32()
    rc = _ffi.lib.dbg_expr_dims_variant(arr, len(shape),
                                        sum(1 << a for a in dims),
                                        ctypes.byref(nb), ctypes.byref(gx))
    assert rc >= 0
    return _ffi.EXPR_DIMS_VARIANTS[rc], nb.value, gx.value


def p_near_one(x):          # values in [0.98, 1.02): a product that stays put
    return (E.ref(x) + 0.5) * 0.04 + 0.98


def p_i64(x, y):
    return abs(E.ref(x)) * 3 + E.ref(y)


# ------------------------------------------------------------- (33, 7)
@pytest.mark.parametrize("dims", [(0,), (1,), (0, 1)])
@pytest.mark.parametrize("dt", ["f64", "f32"])
def test_33x7_row_and_column_operands(dja, dt, dims):
    with Pool(dja) as p:
        X = p.mk(inputs((33, 7), dt, 21))
        M = p.mk(inputs((1, 7), dt, 22))
        C = p.mk(inputs((33, 1), dt, 23))
        demean = E.abs2(E.ref(X) - E.ref(M))
        rowcol = E.ref(X) * E.ref(M) + E.ref(C)
        for op in ("add", "min", "max", None):
            p.fold(op, demean, dims, dt, "demean " + dt)
            p.fold(op, rowcol, dims, dt, "row*col " + dt)
        p.fold("mul", p_near_one(X), dims, dt, "near one " + dt)
        # no operand has the domain's shape
        p.fold("add", E.ref(M) * E.ref(C), dims, dt, "outer " + dt)


# ------------------------------------------------- (5, 4, 3), (3, 2, 5, 4)
@pytest.mark.parametrize("dims", [(1,), (0, 2), (1, 2), (0, 1, 2)])
def test_5x4x3_with_a_singleton_dim_operand(dja, dims):
    with Pool(dja) as p:
        A = p.mk(inputs((5, 4, 3), "f64", 24))
        S = p.mk(inputs((5, 1, 3), "f64", 25))
        e = E.abs2(E.ref(A) - E.ref(S))
        for op in ("add", "max", None):
            p.fold(op, e, dims, "f64", "(5,4,3)")
        p.fold("mul", p_near_one(A), dims, "f64", "(5,4,3) near one")
        AI, SI = p.mk(inputs((5, 4, 3), "i64", 26)), \
            p.mk(inputs((5, 1, 3), "i64", 27))
        for op in ("add", "mul", "min", "max"):
            p.fold(op, p_i64(AI, SI), dims, "i64", "(5,4,3) i64")


def test_4d_interleaved_kept_and_reduced(dja):
    with Pool(dja) as p:
        A = p.mk(inputs((3, 2, 5, 4), "f64", 28))
        S = p.mk(inputs((3, 1, 5, 1), "f64", 29))
        e = E.ref(A) * E.ref(S) + 0.25
        for dims in ((1, 3), (0, 2), (0, 1, 2, 3), (3,)):
            for op in ("add", "min", None):
                p.fold(op, e, dims, "f64", "(3,2,5,4)")
        A32 = p.mk(inputs((3, 2, 5, 4), "f32", 30))
        p.fold("add", E.abs2(E.ref(A32)), (1, 3), "f32", "(3,2,5,4) f32")


# ---------------------------------------- 257 terms under both schedules
@pytest.mark.parametrize("shape,dims,sched", [
    ((257, 3), (0,), "wave"), ((3, 257), (1,), "lanes")])
@pytest.mark.parametrize("dt", ["f64", "f32", "i64"])
def test_257_terms_cross_a_wave_and_a_block(dja, dt, shape, dims, sched):
    assert variant(shape, dims)[0] == sched
    with Pool(dja) as p:
        X, Y = p.mk(inputs(shape, dt, 31)), p.mk(inputs(shape, dt, 32))
        if dt == "i64":
            e = p_i64(X, Y)
            for op in ("add", "mul", "min", "max", None):
                p.fold(op, e, dims, dt, "257 i64")
        else:
            e = (E.ref(X) - 0.25) * E.ref(Y) + abs(E.ref(X))
            for op in ("add", "min", "max", None):
                p.fold(op, e, dims, dt, "257 " + dt)
            p.fold("mul", p_near_one(X), dims, dt, "257 near one " + dt)


# ----------------------------------------------------- selector thresholds
# (shape, dims, expected (schedule, slices, gridDim.x)): one shape at each
# side of every threshold, the smallest that crosses it
THRESHOLDS = [
    # wave | block at 512 terms
    ((511, 3), (0,), ("wave", 1, 1)),
    ((512, 3), (0,), ("block", 1, 3)),
    # lanes: split from 16 terms (2 slices of 8) ...
    ((256, 15), (1,), ("lanes", 1, 1)),
    ((256, 16), (1,), ("lanes", 2, 1)),
    # ... while the outputs fill at most 512 workgroups
    ((131072, 16), (1,), ("lanes", 2, 512)),
    ((131073, 16), (1,), ("lanes", 1, 513)),
    # block: split from 2048 terms (2 slices of 1024) ...
    ((2047, 2), (0,), ("block", 1, 2)),
    ((2048, 2), (0,), ("block", 2, 2)),
    # ... while there are at most 512 outputs
    ((2048, 512), (0,), ("block", 2, 512)),
    ((2048, 513), (0,), ("block", 1, 513)),
    # many slices (8191 // 8 = 1023 wanted, 9 terms each make 911), the
    # last one ragged
    ((3, 8191), (1,), ("lanes", 911, 1)),
    # grid cap of 4096 workgroups, each schedule
    ((1 << 20, 2), (1,), ("lanes", 1, 4096)),
    (((1 << 20) + 1, 2), (1,), ("lanes", 1, 4096)),
    ((2, 16384), (0,), ("wave", 1, 4096)),
    ((2, 16385), (0,), ("wave", 1, 4096)),
    ((512, 4096), (0,), ("block", 1, 4096)),
    ((512, 4097), (0,), ("block", 1, 4096)),
]


@pytest.mark.parametrize("shape,dims,want", THRESHOLDS,
                         ids=["%s-%s" % ("x".join(map(str, s)), d[0])
                              for s, d, _ in THRESHOLDS])
def test_selector_thresholds(dja, shape, dims, want):
    assert variant(shape, dims) == want
    with Pool(dja) as p:
        # integer-valued f64: every partial sum is exact, so the sum is
        # checked to the bit for any number of outputs
        X = p.mk(ints(shape, "f64", 41))
        kept = tuple(1 if a in dims else s for a, s in enumerate(shape))
        V = p.mk(ints(kept, "f64", 42))
        e = E.ref(X) * E.ref(V) + E.ref(X)
        p.fold("add", e, dims, "f64", ("thr", shape), integral=True)
        p.fold("max", e, dims, "f64", ("thr", shape))
        p.fold(None, e, dims, "f64", ("thr", shape))


def test_split_fold_with_real_valued_terms(dja):
    """The split path (partial rows, second kernel) under the fsum bound
    and the product bound, f64 and f32."""
    for shape, dims in (((2048, 2), (0,)), ((3, 257), (1,))):
        assert variant(shape, dims)[1] > 1
        for dt in ("f64", "f32"):
            with Pool(dja) as p:
                X = p.mk(inputs(shape, dt, 43))
                p.fold("add", E.abs2(E.ref(X)) - 0.05, dims, dt,
                       ("split", shape, dt))
                if shape[0] == 3:
                    p.fold("mul", p_near_one(X), dims, dt,
                           ("split", shape, dt))
                p.fold("min", E.ref(X), dims, dt, ("split", shape, dt))


# ------------------------------------------------ other dtypes and cases
@pytest.mark.parametrize("dims", [(0,), (1,), (0, 1)])
def test_i64_all_folds_with_strided_operands(dja, dims):
    with Pool(dja) as p:
        X, Y = p.mk(inputs((33, 7), "i64", 51)), \
            p.mk(inputs((33, 7), "i64", 52))
        Rw, Cl = p.mk(inputs((1, 7), "i64", 53)), \
            p.mk(inputs((33, 1), "i64", 54))
        for e in (p_i64(X, Y), p_i64(X, Rw), p_i64(Cl, X)):
            for op in ("add", "mul", "min", "max", None):
                p.fold(op, e, dims, "i64", "i64 (33,7)")
        # wrap-around is exact
        big = np.full((33, 7), (1 << 62) + 12345, dtype=np.int64)
        B = p.mk(big)
        p.fold("add", E.ref(B) + E.ref(X), dims, "i64", "i64 wrap")
        p.fold("mul", E.ref(B) * 3 + E.ref(Rw), dims, "i64", "i64 wrap")


def test_count_of_a_comparison_tree(dja):
    for dt, c in (("f64", 0.1), ("f32", 0.125), ("i64", 2)):
        with Pool(dja) as p:
            x = inputs((33, 7), dt, 55)
            X, Rw = p.mk(x), p.mk(inputs((1, 7), dt, 56))
            for dims in ((0,), (1,), (0, 1)):
                got = p.fold(None, E.ref(X) > c, dims, dt, "x > c")
                assert np.array_equal(
                    got, (x > c).sum(axis=dims, keepdims=True))
                p.fold(None, E.le(E.ref(X), E.ref(Rw)), dims, dt, "x <= r")
                C = dja.dcount_dims(lambda t: t > c, X, dims)
                assert C.dtype == "i64" and np.array_equal(C.localpart(),
                                                           got)
                C.close()
                N = dja.dcount_dims("nonzero", X, dims)
                assert np.array_equal(N.localpart(), np.count_nonzero(
                    x, axis=dims, keepdims=True))
                N.close()


def test_all_and_any_along_dims(dja):
    with Pool(dja) as p:
        x = inputs((33, 7), "f64", 57)
        x[:, 2] = np.abs(x[:, 2]) + 0.01         # one column all positive
        x[:, 4] = -np.abs(x[:, 4]) - 0.01        # one column all negative
        X = p.mk(x)
        pos = lambda t: t > 0.0
        for dims in ((0,), (1,), (0, 1)):
            A, Y = dja.dall_dims(pos, X, dims), dja.dany_dims(pos, X, dims)
            assert A.dtype == "i64" and Y.dtype == "i64"
            assert np.array_equal(A.localpart(), (x > 0).all(
                axis=dims, keepdims=True).astype(np.int64)), dims
            assert np.array_equal(Y.localpart(), (x > 0).any(
                axis=dims, keepdims=True).astype(np.int64)), dims
            A.close()
            Y.close()
        F = dja.dall_dims("isfinite", X, 0)
        assert np.array_equal(F.localpart(), np.ones((1, 7), np.int64))
        F.close()
        # an empty reduced extent: all is 1, any is 0
        Z = p.own(dja.DArray((0, 4), "f64"))
        A, Y = dja.dall_dims(pos, Z, 0), dja.dany_dims(pos, Z, 0)
        assert np.array_equal(A.localpart(), np.ones((1, 4), np.int64))
        assert np.array_equal(Y.localpart(), np.zeros((1, 4), np.int64))
        A.close()
        Y.close()


def test_empty_reduced_extent_and_no_outputs(dja):
    with Pool(dja) as p:
        for dt in ("f64", "f32", "i64"):
            Z = p.own(dja.DArray((0, 4), dt))
            for op in ("add", "mul", "min", "max"):
                R = E.reduce(op, E.ref(Z) + 1, dims=0)
                got = R.localpart()
                R.close()
                want = np.full((1, 4), kr.fold_identity(op, dt),
                               dtype=kr.NP[dt])
                assert ref.same_bits(got, want), (dt, op)
            C = E.count(E.ref(Z), dims=(0,))
            assert np.array_equal(C.localpart(), np.zeros((1, 4), np.int64))
            C.close()
            # K == 0: nothing is launched, the result is empty
            R = E.reduce("add", E.ref(Z), dims=1)
            assert R.dims == (0, 1) and R.localpart().size == 0
            R.close()
            R = E.count(E.ref(Z), dims=(0, 1))
            assert R.dims == (1, 1) and int(R.localpart()[0, 0]) == 0
            R.close()


def test_errors_raise_and_leak_nothing(dja):
    from distributedarrays_jl_amd._ffi import DArrayError
    with Pool(dja) as p:
        ds = [p.mk(inputs((4, 2), "f64", 60 + k)) for k in range(7)]
        e = E.ref(ds[0])
        for d in ds[1:]:
            e = e + E.ref(d)
        with pytest.raises(DArrayError):
            E.reduce("add", e, dims=0)
        with pytest.raises(DArrayError):
            E.count(e, dims=0)
        with pytest.raises(DArrayError):
            E.reduce("add", E.lit(2.0) * 3.0, dims=0)
        for bad in ((2,), (-1,), (0, 7)):
            with pytest.raises(DArrayError):
                E.reduce("add", E.ref(ds[0]), dims=bad)
        with pytest.raises(DArrayError):
            E.reduce("sub", E.ref(ds[0]), dims=0)
        with pytest.raises(DArrayError):
            dja.dvar_dims(p.mk(inputs((4, 2), "i64", 70)), 0)


# ---------------------------------------------------------------------- NaN
@pytest.mark.parametrize("shape,dims", [((33, 7), (0,)), ((33, 7), (1,)),
                                        ((2048, 2), (0,)), ((3, 257), (1,))])
def test_one_nan_poisons_its_own_output_only(dja, shape, dims):
    """log of one negative element: that output's min and max are NaN, the
    others' are not (every other term is log(x), x in [1.5, 2.5)); the
    count counts it."""
    with Pool(dja) as p:
        x = (kr.uniform(int(np.prod(shape)), "f64", 61) + 1.5).reshape(
            shape, order="F")
        at = (shape[0] - 2, 1)
        x[at] = -1.0
        X = p.mk(x)
        e = E.log(E.ref(X))
        kept = at[1 - dims[0]]
        for op in ("min", "max"):
            R = E.reduce(op, e, dims=dims)
            got = R.localpart().ravel()
            R.close()
            assert np.isnan(got[kept])
            assert not np.isnan(np.delete(got, kept)).any()
            want = (np.min if op == "min" else np.max)(
                np.log(np.where(x > 0, x, 2.0)), axis=dims).ravel()
            # log is not IEEE-exact: a few ulps from numpy's
            assert np.allclose(np.delete(got, kept), np.delete(want, kept),
                               rtol=1e-14)
        C = E.count(e, dims=dims)
        assert np.array_equal(C.localpart().ravel(),
                              np.count_nonzero(x != 1.0, axis=dims))
        C.close()


# ------------------------------------------- JIT / interpreter, determinism
def test_jit_and_interpreter_give_the_same_bits_twice(dja):
    """DA_EXPR_JIT is read per call, so both paths run in this process;
    each runs twice: the bits depend on nothing but the shape."""
    from distributedarrays_jl_amd._ffi import lib
    lib.da_expr_jit_errstr.restype = ctypes.c_char_p
    with Pool(dja) as p:
        # every schedule, the split path, each dtype; few distinct kernels
        cases = []
        for shape, dimsets, dts in (
                ((33, 7), ((0,), (1,), (0, 1)), ("f64", "f32", "i64")),
                ((257, 3), ((0,),), ("f64",)),
                ((3, 257), ((1,),), ("f64", "i64")),
                ((2048, 2), ((0,),), ("f64", "f32")),
                ((5, 4, 3), ((0, 2),), ("f64",))):
            for dt in dts:
                X, Y = p.mk(inputs(shape, dt, 71)), \
                    p.mk(inputs(shape, dt, 72))
                kept = tuple(s if a else 1 for a, s in enumerate(shape))
                V = p.mk(inputs(kept, dt, 73))
                if dt == "i64":
                    e, ops = p_i64(X, V), ("mul",)
                elif dt == "f32":
                    e, ops = E.ref(X) * E.ref(V) + E.abs2(E.ref(Y)), ("add",)
                else:
                    e = E.sin(E.ref(X)) * E.ref(V) + E.abs2(E.ref(Y))
                    ops = ("add",)
                for dims in dimsets:
                    cases.append((e, dims, ops))

        def run():
            out = []
            for e, dims, ops in cases:
                for op in ops + (None,):
                    R = E.count(e, dims=dims) if op is None else \
                        E.reduce(op, e, dims=dims)
                    out.append(ref.bits(R.localpart()).tolist())
                    R.close()
            return out

        jit = run()
        assert run() == jit
        state = int(lib.da_expr_jit_state())
        os.environ["DA_EXPR_JIT"] = "0"
        try:
            interp = run()
            assert run() == interp
        finally:
            del os.environ["DA_EXPR_JIT"]
        assert jit == interp
        assert state == 2, "expr JIT not active: state %d, err %r" % (
            state, lib.da_expr_jit_errstr())


# ------------------------------------------------------ against dreduce_dims
@pytest.mark.parametrize("shape,dims", [((33, 7), (0,)), ((33, 7), (1,)),
                                        ((33, 7), (0, 1)), ((5, 4, 3), (0, 2)),
                                        ((257, 3), (0,)), ((3, 257), (1,))])
def test_plain_ref_equals_dreduce_dims(dja, shape, dims):
    """E.ref(D) alone: i64 folds, min and max do not depend on the order,
    so the fused kernel and the per-axis kernels agree to the bit."""
    with Pool(dja) as p:
        for dt, ops in (("i64", ("add", "mul", "min", "max")),
                        ("f64", ("min", "max")), ("f32", ("min", "max"))):
            D = p.mk(inputs(shape, dt, 81))
            for op in ops:
                F = E.reduce(op, E.ref(D), dims=dims)
                G = dja.dreduce_dims("identity", op, D, dims)
                M = dja.mapreduce(lambda t: t, op, D, dims=dims)
                try:
                    assert F.dims == G.dims and F.dist == G.dist
                    assert list(F.ranks) == list(G.ranks)
                    assert ref.same_bits(F.localpart(), G.localpart()), \
                        (dt, op)
                    assert ref.same_bits(M.localpart(), G.localpart())
                finally:
                    F.close()
                    G.close()
                    M.close()


# ------------------------------------------------------------------ dvar_dims
@pytest.mark.parametrize("shape,dims", [((33, 7), (0,)), ((33, 7), (1,)),
                                        ((257, 3), (0,)), ((3, 257), (1,)),
                                        ((5, 4, 3), (0, 2))])
def test_dvar_dims(dja, shape, dims):
    with Pool(dja) as p:
        x = inputs(shape, "f64", 91)
        X = p.mk(x)
        # the fused sum against oracle terms built with the device's own
        # mean row, under the add bound
        M = p.own(dja.dmean_dims(X, dims))
        p.host[id(M)] = M.localpart()
        p.fold("add", E.abs2(E.ref(X) - E.ref(M)), dims, "f64", "dvar sum")
        xl = x.astype(np.longdouble)
        for corrected in (True, False):
            V = dja.dvar_dims(X, dims, corrected)
            S = dja.dstd_dims(X, dims, corrected)
            try:
                want = np.var(xl, axis=dims, keepdims=True,
                              ddof=1 if corrected else 0)
                got = V.localpart()
                assert got.shape == want.shape
                rel = np.abs(got - want) / want
                print("dvar_dims %s %s worst rel %.3e" % (shape, dims,
                                                          float(rel.max())))
                assert (rel <= 1e-12).all(), float(rel.max())
                assert np.allclose(S.localpart(), np.sqrt(got), rtol=1e-15)
            finally:
                V.close()
                S.close()
        # one sample, corrected: NaN
        one = p.mk(x[(slice(0, 1),) * len(shape)])
        V = dja.dvar_dims(one, tuple(range(len(shape))))
        assert np.isnan(V.localpart()).all()
        V.close()


# --------------------------------------------------------------------- example
def test_zscore_fused_example(dja):
    """examples/zscore_fused.py at a small size with a 1e6 offset, where the
    E[X^2] - mu^2 form of examples/zscore.py keeps 4 digits: the two-pass
    std is good to 1e-12 relative (the dvar tolerance; N = 257)."""
    from examples.zscore_fused import zscore
    X, mu, sig, Z = zscore(257, 33, offset=1.0e6)
    try:
        hX = X.localpart().astype(np.longdouble)
        want = np.std(hX, axis=0, keepdims=True)
        assert sig.dims == (1, 33) and list(sig.ranks) == list(mu.ranks)
        rel = np.abs(sig.localpart() - want) / want
        assert (rel <= 1e-12).all(), float(rel.max())
        z = (hX - hX.mean(axis=0, keepdims=True)) / want
        assert np.max(np.abs(Z.localpart() - z)) < 1e-8
    finally:
        for d in (X, mu, sig, Z):
            d.close()
