"""The fused mapreduce over broadcast trees on the GPU (da_expr_reduce /
da_expr_count behind expr.reduce / expr.count).

Contract under test: the fused result has EXACTLY the bits of materialising
the tree and reducing the temporary with da_reduce / da_count — for every
program, layout, fold and size, through the hipRTC kernel and through the
interpreter, in one launch and under DA_RED_FUSED=0.

Sizes are the smallest at which the kernel can go wrong: 0 (no launch), 1
and 2 (tail only / one pair), 257 (block boundary), 513 (just past one
block of pairs), 2^20+1 (grid cap of 2048 blocks reached, a second
grid-stride iteration, and a tail).  Strided shapes (33, 7) — pairs cross
column ends — and (5, 4, 3).

Bounds against the oracle (terms t from oracle.expr.evaluate, bit-identical
to the device's for IEEE-exact programs): min / max / i64 / count are exact.
A float sum obeys |got - fsum(t)| <= 1.01 * D * u * sum|t|, D the longest
chain of dependent roundings in the fold order: the per-thread serial
length, 6 shuffle steps, 2 LDS steps, ceil(g/256) partials per thread of
the last block, and that block's own 6 + 2.  A float product obeys
|got/exact - 1| <= 1.01 * n * u.  Derived from the fold order, not
measured."""
import ctypes
import math
import os
import subprocess
import sys

import numpy as np
import pytest

import kernel_ref as kr
import oracle.expr as oexpr
from distributedarrays_jl_amd import expr as E

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
SIZES = [0, 1, 2, 257, 513, (1 << 20) + 1]
CHILD_TIMEOUT = 120
_faulted = []


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

    def own(self, d):
        self.ds.append(d)
        return d

    def terms(self, e, dt):
        """The oracle's values of the tree, flat in column-major order."""
        prog, args, consts = E.compile_expr(e)
        t = oexpr.evaluate(prog, [self.host[id(a)] for a in args], consts,
                           kr.NP[dt])
        shape = np.broadcast_shapes(*[self.host[id(a)].shape for a in args])
        return np.broadcast_to(t, shape).ravel(order="F")


def bits_of(v, dt):
    return int(kr.bits(np.array([v], dtype=kr.NP[dt]))[0])


def inputs(n, dt, seed, shape=None):
    """Both signs for floats; small integers for i64."""
    x = kr.uniform(n, dt, seed)
    if dt != "i64":
        x = x - kr.NP[dt].type(0.5)
    return x if shape is None else x.reshape(shape, order="F")


def check_against_materialised(dja, e, dt, ops, tag, count=True):
    """Contract of the fused reduce: bits of materialise-then-reduce."""
    tmp = E.materialize(e)
    try:
        for op in ops:
            got = E.reduce(op, e)
            want = dja.mapreduce("identity", op, tmp)
            assert bits_of(got, dt) == bits_of(want, dt), (tag, op, got, want)
        if count:
            assert E.count(e) == dja.dcount("nonzero", tmp), tag
    finally:
        tmp.close()


# four programs of the contract: an IEEE-exact chain, a sin chain, a
# two-operand product, (strided) a de-meaned square
def p_exact(x, y):
    return (E.ref(x) - 0.25) * E.ref(y) + abs(E.ref(x))


def p_sin(x, y):
    return E.sin(E.ref(x)) + E.ref(y) * 0.5


def p_prod(x, y):
    return E.ref(x) * E.ref(y)


def p_near_one(x):          # values in [0.98, 1.02): a product that stays put
    return (E.ref(x) + 0.5) * 0.04 + 0.98


def grid_of(n):
    return min(2048, max(1, (n // 2 + 255) // 256))


def chain_length(n):
    """D of the module docstring."""
    g = grid_of(n)
    stride = g * 256
    serial = 2 * -(-(n // 2) // stride) + (n & 1)
    return serial + 6 + 2 + -(-g // 256) + 8


def check_against_oracle(got, t, op, dt, n, tag):
    if op in ("min", "max"):
        want = t.min() if op == "min" else t.max()
        assert bits_of(got, dt) == bits_of(want, dt), (tag, op, got, want)
    elif dt == "i64":
        with np.errstate(over="ignore"):
            want = t.sum(dtype=np.int64) if op == "add" \
                else t.prod(dtype=np.int64)
        assert got == int(want), (tag, op, got, want)
    elif op == "add":
        tl = [float(v) for v in t]
        err = abs(float(got) - math.fsum(tl))
        bound = 1.01 * chain_length(n) * kr.UNIT[dt] * \
            math.fsum(abs(v) for v in tl)
        print("%s add err %.3e bound %.3e" % (tag, err, bound))
        assert err <= bound, (tag, got, err, bound)
    else:
        exact = np.prod(t.astype(np.longdouble))
        rel = abs(np.longdouble(got) / exact - 1)
        bound = 1.01 * n * kr.UNIT[dt]
        print("%s mul rel %.3e bound %.3e" % (tag, float(rel), bound))
        assert rel <= bound, (tag, got, float(rel), bound)


# ------------------------------------------------------ bit identity, flat
@pytest.mark.parametrize("n", SIZES)
def test_flat_f64_bits(dja, n):
    with Pool(dja) as p:
        x, y = p.mk(inputs(n, "f64", 11)), p.mk(inputs(n, "f64", 12))
        for name, e in (("exact", p_exact(x, y)), ("sin", p_sin(x, y)),
                        ("prod", p_prod(x, y))):
            check_against_materialised(dja, e, "f64", ("add", "max", "min"),
                                       (name, n))
        check_against_materialised(dja, p_near_one(x), "f64", ("mul",),
                                   ("near_one", n), count=False)


@pytest.mark.parametrize("n", SIZES)
def test_flat_f32_bits(dja, n):
    with Pool(dja) as p:
        x, y = p.mk(inputs(n, "f32", 13)), p.mk(inputs(n, "f32", 14))
        check_against_materialised(dja, p_exact(x, y), "f32",
                                   ("add", "max"), ("exact", n))
        check_against_materialised(dja, p_prod(x, y), "f32", ("add",),
                                   ("prod", n), count=False)
        check_against_materialised(dja, p_near_one(x), "f32", ("mul",),
                                   ("near_one", n), count=False)


def p_i64(x, y):
    return abs(E.ref(x)) * 3 + E.ref(y)


@pytest.mark.parametrize("n", SIZES)
def test_flat_i64_bits_and_values(dja, n):
    with Pool(dja) as p:
        x, y = p.mk(inputs(n, "i64", 15)), p.mk(inputs(n, "i64", 16))
        e = p_i64(x, y)
        check_against_materialised(dja, e, "i64",
                                   ("add", "mul", "min", "max"), ("i64", n))
        t = p.terms(e, "i64")
        for op in ("add", "mul"):
            check_against_oracle(E.reduce(op, e), t, op, "i64", n, ("i64", n))
        if n:
            assert E.reduce("min", e) == int(t.min())
            assert E.reduce("max", e) == int(t.max())
        else:
            assert E.reduce("min", e) == kr.I64_MAX
            assert E.reduce("max", e) == kr.I64_MIN
        assert E.count(e) == int(np.count_nonzero(t))


@pytest.mark.parametrize("n", SIZES)
def test_special_cases_share_bits_with_existing_paths(dja, n):
    with Pool(dja) as p:
        x, y = p.mk(inputs(n, "f64", 17)), p.mk(inputs(n, "f64", 18))
        for op in ("add", "max"):
            assert bits_of(E.reduce(op, E.ref(x)), "f64") == \
                bits_of(dja.mapreduce("identity", op, x), "f64"), (n, op)
        want = bits_of(dja.mapreduce("abs2", "add", x), "f64")
        assert bits_of(E.reduce("add", E.abs2(E.ref(x))), "f64") == want, n
        # aliasing: x * x is one operand slot, and abs2's value
        prog, args, _ = E.compile_expr(E.ref(x) * E.ref(x))
        assert len(args) == 1
        assert bits_of(E.reduce("add", E.ref(x) * E.ref(x)), "f64") == want
        assert bits_of(E.reduce("add", E.ref(x) * E.ref(y)), "f64") == \
            bits_of(dja.ddot(x, y), "f64"), n
        assert bits_of(dja.mapreduce(lambda a, b: a * b, "add", x, y),
                       "f64") == bits_of(dja.ddot(x, y), "f64"), n


def test_empty_chunk_returns_identity_without_launch(dja):
    from distributedarrays_jl_amd._ffi import lib
    with Pool(dja) as p:
        x = p.mk(np.zeros(0))
        for dt in ("f64", "f32"):
            d = p.own(dja.DArray((0,), dt))
            for op in ("add", "mul", "min", "max"):
                assert bits_of(E.reduce(op, E.ref(d) + 1.0), dt) == \
                    bits_of(kr.fold_identity(op, dt), dt), (dt, op)
            assert E.count(E.ref(d) + 1.0) == 0
        assert E.reduce("add", E.ref(x)) == 0.0


def test_seven_operands_raise(dja):
    from distributedarrays_jl_amd._ffi import DArrayError
    with Pool(dja) as p:
        ds = [p.mk(inputs(8, "f64", 40 + k)) for k in range(7)]
        e = E.ref(ds[0])
        for d in ds[1:]:
            e = e + E.ref(d)
        with pytest.raises(DArrayError):
            E.reduce("add", e)
        with pytest.raises(DArrayError):
            E.count(e)
        with pytest.raises(DArrayError):
            E.reduce("add", E.lit(2.0) * 3.0)


# --------------------------------------------------- bit identity, strided
def strided_operands(p, dt, seed):
    X = p.mk(inputs(33 * 7, dt, seed, (33, 7)))
    R = p.mk(inputs(7, dt, seed + 1, (1, 7)))
    C = p.mk(inputs(33, dt, seed + 2, (33, 1)))
    return X, R, C


def test_strided_f64_bits(dja):
    with Pool(dja) as p:
        X, R, C = strided_operands(p, "f64", 21)
        M = p.own(dja.dmean_dims(X, (0,)))
        check_against_materialised(dja, E.abs2(E.ref(X) - E.ref(M)), "f64",
                                   ("add", "max", "min"), "demean (33,7)")
        check_against_materialised(dja, E.ref(X) * E.ref(R) + E.ref(C),
                                   "f64", ("add",), "row+col (33,7)",
                                   count=False)
        # no full-shape operand: the domain is the default grid
        check_against_materialised(dja, E.ref(R) * E.ref(C), "f64",
                                   ("max",), "outer (33,7)", count=False)
        A3 = p.mk(inputs(60, "f64", 24, (5, 4, 3)))
        S3 = p.mk(inputs(15, "f64", 25, (5, 1, 3)))
        check_against_materialised(dja, E.abs2(E.ref(A3) - E.ref(S3)),
                                   "f64", ("add",), "(5,4,3)", count=False)


def test_strided_f32_bits(dja):
    with Pool(dja) as p:
        X, R, C = strided_operands(p, "f32", 26)
        check_against_materialised(dja, E.abs2(E.ref(X) - E.ref(R)), "f32",
                                   ("add",), "demean f32 (33,7)", count=False)


# ----------------------------------------------------- parity with oracle
@pytest.mark.parametrize("dt", ["f64", "f32"])
@pytest.mark.parametrize("n", SIZES[1:])
def test_oracle_parity_flat(dja, n, dt):
    """Same programs and folds as the bit-identity tests (no new kernels)."""
    with Pool(dja) as p:
        x, y = p.mk(inputs(n, dt, 31)), p.mk(inputs(n, dt, 32))
        e = p_exact(x, y)
        t = p.terms(e, dt)
        for op in ("add", "max"):
            check_against_oracle(E.reduce(op, e), t, op, dt, n,
                                 ("exact", dt, n))
        assert E.count(e) == int(np.count_nonzero(t))
        e = p_near_one(x)
        check_against_oracle(E.reduce("mul", e), p.terms(e, dt), "mul", dt,
                             n, ("near_one", dt, n))
        if dt == "f64":
            check_against_oracle(E.reduce("min", p_exact(x, y)), t, "min",
                                 dt, n, ("exact", dt, n))


def test_oracle_parity_strided(dja):
    with Pool(dja) as p:
        X, R, C = strided_operands(p, "f64", 33)
        e = E.ref(X) * E.ref(R) + E.ref(C)
        check_against_oracle(E.reduce("add", e), p.terms(e, "f64"), "add",
                             "f64", 33 * 7, "row+col")
        M = p.own(dja.dmean_dims(X, (0,)))
        p.host[id(M)] = M.localpart()
        e = E.abs2(E.ref(X) - E.ref(M))
        t = p.terms(e, "f64")
        for op in ("add", "max", "min"):
            check_against_oracle(E.reduce(op, e), t, op, "f64", 33 * 7,
                                 "demean")
        assert E.count(e) == int(np.count_nonzero(t))


@pytest.mark.parametrize("n", [513, (1 << 20) + 1])
def test_nan_propagates_and_counts(dja, n):
    """log of one negative element: min and max return NaN, count counts
    it (every other term is log(x) > 0, x in [1.5, 2.5))."""
    with Pool(dja) as p:
        x = kr.uniform(n, "f64", 34) + 1.5
        x[300] = -1.0
        d = p.mk(x)
        e = E.log(E.ref(d))
        assert math.isnan(E.reduce("min", e))
        assert math.isnan(E.reduce("max", e))
        assert E.count(e) == n


# ------------------------------------------------------------------ fuzzer
F_UN = ["neg", "abs", "abs2", "floor", "sign"]
F_BIN = ["add", "sub", "mul", "min2", "max2"]
I_UN = ["neg", "abs", "abs2", "sign"]
I_BIN = ["add", "sub", "mul", "min2", "max2", "xor"]


def random_tree(rng, leaves, un, bin_, depth, integer):
    if depth == 0 or rng.random() < 0.2:
        if rng.random() < 0.75:
            return E.ref(leaves[int(rng.integers(len(leaves)))])
        c = int(rng.integers(-3, 4))
        return E.lit(c if integer else c * 0.375)
    if rng.random() < 0.35:
        return E.Unary(un[int(rng.integers(len(un)))],
                       random_tree(rng, leaves, un, bin_, depth - 1, integer))
    return E.Binary(bin_[int(rng.integers(len(bin_)))],
                    random_tree(rng, leaves, un, bin_, depth - 1, integer),
                    random_tree(rng, leaves, un, bin_, depth - 1, integer))


def test_random_programs_keep_the_contract(dja):
    from distributedarrays_jl_amd._ffi import DArrayError
    rng = np.random.default_rng(20260)
    n = 100003
    done = 0
    with Pool(dja) as p:
        leaves = {dt: [p.mk(inputs(n, dt, 50 + k + 10 * kr.DT[dt]))
                       for k in range(3)] for dt in ("f64", "i64")}
        ops = ("add", "max", "min", "add")
        for k in range(4):
            dt = "i64" if k >= 3 else "f64"
            un, bin_ = (I_UN, I_BIN) if dt == "i64" else (F_UN, F_BIN)
            while True:
                e = random_tree(rng, leaves[dt], un, bin_, 3, dt == "i64")
                try:
                    if E.compile_expr(e)[1]:
                        break
                except DArrayError:
                    pass
            check_against_materialised(dja, e, dt, (ops[k],), ("fuzz", k),
                                       count=(k % 3 == 0))
            done += 1
    assert done == 4


# ------------------------------------------------------- JIT / interpreter
def test_jit_and_interpreter_give_the_same_bits(dja):
    """DA_EXPR_JIT is read per call, so both paths run in this process."""
    from distributedarrays_jl_amd._ffi import lib
    lib.da_expr_jit_errstr.restype = ctypes.c_char_p
    with Pool(dja) as p:
        cases = []
        for n in SIZES:
            x, y = p.mk(inputs(n, "f64", 61)), p.mk(inputs(n, "f64", 62))
            cases.append((("sin", n), p_sin(x, y), "f64", ("add", "max")))
            cases.append((("exact", n), p_exact(x, y), "f64", ("min",)))
            xi, yi = p.mk(inputs(n, "i64", 63)), p.mk(inputs(n, "i64", 64))
            cases.append((("i64", n), p_i64(xi, yi), "i64", ("add", "mul")))
            x32, y32 = p.mk(inputs(n, "f32", 65)), p.mk(inputs(n, "f32", 66))
            cases.append((("f32", n), p_exact(x32, y32), "f32", ("add",)))
        X, R, C = strided_operands(p, "f64", 67)
        M = p.own(dja.dmean_dims(X, (0,)))
        cases.append(("demean", E.abs2(E.ref(X) - E.ref(M)), "f64",
                      ("add", "max")))
        cases.append(("row+col", E.ref(X) * E.ref(R) + E.ref(C), "f64",
                      ("add",)))

        def run():
            out = []
            for tag, e, dt, ops in cases:
                out += [(tag, op, bits_of(E.reduce(op, e), dt)) for op in ops]
                out.append((tag, "count", E.count(e)))
            return out

        jit = run()
        state = int(lib.da_expr_jit_state())
        os.environ["DA_EXPR_JIT"] = "0"
        try:
            interp = run()
        finally:
            del os.environ["DA_EXPR_JIT"]
        assert jit == interp
        assert state == 2, "expr JIT not active: state %d, err %r" % (
            state, lib.da_expr_jit_errstr())


# ------------------------------------------------- one launch / two kernels
def run_child(script, env_extra, tag):
    """One child at a time under its own timeout; none after one that died."""
    if _faulted:
        pytest.fail("an earlier child faulted (%s); not starting further "
                    "GPU processes" % _faulted[0])
    env = dict(os.environ)
    env.pop("DA_RED_FUSED", None)
    env.update(env_extra)
    try:
        r = subprocess.run([sys.executable, os.path.join(HERE, script)],
                           env=env, capture_output=True, text=True,
                           timeout=CHILD_TIMEOUT)
    except subprocess.TimeoutExpired:
        _faulted.append(tag)
        pytest.fail("%s: child exceeded %d s" % (tag, CHILD_TIMEOUT))
    if r.returncode < 0 or r.returncode in (134, 139):
        _faulted.append(tag)
    assert r.returncode == 0, "%s: child exit %d\n%s" % (
        tag, r.returncode, r.stderr[-2000:])
    return r.stdout


def test_single_launch_and_two_kernel_bits_agree():
    one = run_child("expr_reduce_bits_child.py", {}, "bits default")
    two = run_child("expr_reduce_bits_child.py", {"DA_RED_FUSED": "0"},
                    "bits DA_RED_FUSED=0")
    assert one.endswith("bits done\n") and one.count("\n") == 19, one
    assert one == two


# ---------------------------------------------------------- ticket sequence
def test_ticket_sequence_across_all_single_launch_kernels(dja):
    """The fused expression reduce shares the ticket counter with da_reduce
    and da_count: three rounds of interleaved launches with changing grids.
    A launch that does not advance red_base by its grid makes the next one
    miss (or double) its last arriver.  Integer-valued data: every sum is
    exact."""
    big = (1 << 20) + 1
    with Pool(dja) as p:
        a = kr.small_ints(257, 71, 8).astype(np.float64)
        b = kr.small_ints(big, 72, 8).astype(np.float64)
        c = kr.small_ints(513, 73, 8).astype(np.float64)
        hx = kr.small_ints(33 * 7, 74, 8).astype(np.float64).reshape(
            (33, 7), order="F")
        hr = kr.small_ints(7, 75, 8).astype(np.float64).reshape((1, 7))
        hc = kr.small_ints(33, 76, 8).astype(np.float64).reshape((33, 1))
        A, B, C, X, R = p.mk(a), p.mk(b), p.mk(c), p.mk(hx), p.mk(hr)
        K = p.mk(hc)
        for rnd in range(3):
            tag = "round %d" % rnd
            assert E.reduce("add", E.ref(A)) == a.sum(), tag
            assert dja.dsum(B) == b.sum(), tag
            assert E.count(E.ref(C)) == int(np.count_nonzero(c)), tag
            assert dja.dcount("nonzero", A) == int(np.count_nonzero(a)), tag
            assert E.reduce("add", E.ref(X) * E.ref(R) + E.ref(K)) == \
                (hx * hr + hc).sum(), tag
            assert dja.dmaximum(B) == b.max(), tag


def test_var_and_std(dja):
    with Pool(dja) as p:
        x = inputs(100003, "f64", 81)
        d = p.mk(x)
        v = float(np.var(x.astype(np.longdouble), ddof=1))
        assert abs(dja.dvar(d) - v) <= 1e-12 * v
        assert abs(dja.dstd(d, corrected=False)
                   - float(np.std(x.astype(np.longdouble)))) <= 1e-12
        pos = lambda t: E.sign(E.max2(t, 0.0))
        assert dja.dcount(pos, d) == int((x > 0).sum())
        assert dja.dany(pos, d) is True and dja.dall(pos, d) is False
