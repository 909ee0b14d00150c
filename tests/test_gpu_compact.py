"""Comparisons, stream compaction and masks on the GPU (world 1).

ABI level: da_compact / da_expand for all nine (dtype, mask_dtype) pairs
over sizes around every wave / workgroup / tile edge, up to more tiles than
one scan tile holds, and mask patterns from all-false to a float mask of
NaN, -0.0 and denormals.  Comparison numerics: all six ops on f64 / f32 /
i64 through the JIT (this process) and the interpreters (a child with
DA_EXPR_JIT=0), same bits.  Python API: dfilter, dfindall, D[M], D[M] = v,
dcount / dany / dall with comparison lambdas.

Every expectation is numpy boolean indexing on the host array (Fortran
order for N-D) and every data comparison is array_equal on the raw bits:
no tolerance appears anywhere."""
import functools
import os
import subprocess
import sys

import numpy as np
import pytest

import kernel_ref as kr
import cmp_bits_child

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
TILE = 2048
SIZES = [0, 1, 63, 64, 65, 255, 256, 257, 2047, 2048, 2049, 3 * TILE,
         TILE * TILE + 3]
NMAX = SIZES[-1]
DTYPES = ("f64", "f32", "i64")
CHILD_TIMEOUT = 240
SENT = 0xA5


@pytest.fixture(scope="module")
def dja():
    import distributedarrays_jl_amd as dja
    dja.comm.init()
    return dja


@pytest.fixture(autouse=True)
def no_leak(dja):
    before = dja.bytes_in_use()
    yield
    assert dja.bytes_in_use() == before


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint64 if a.dtype.itemsize == 8 else np.uint32)


def same(a, b):
    return a.shape == b.shape and np.array_equal(bits(a), bits(b))


# ------------------------------------------------- shared host references
@functools.lru_cache(maxsize=None)
def _uniform(seed):
    u = kr.uniform(NMAX, "f64", seed)
    u.setflags(write=False)
    return u


@functools.lru_cache(maxsize=None)
def data(dt, seed):
    """NMAX elements of dtype dt, computed once: philox noise with -0.0,
    a NaN with a payload and an infinity planted near the front."""
    if dt == "i64":
        x = kr.philox.fill_int64(NMAX, 500 + seed)
    else:
        x = (_uniform(500 + seed) - 0.5).astype(kr.NP[dt])
        x[0::97] = -0.0
        x[1::89] = np.inf
        nan = bits(x[:1]).dtype.type(0x7FF8000000000123 if dt == "f64"
                                     else 0x7FC00123)
        bits(x)[2::83] = nan
    x.setflags(write=False)
    return x


def patterns(n, mdt):
    """(name, mask) pairs for one size, the mask in dtype mdt."""
    t = kr.NP[mdt].type
    out = [("none", np.zeros(n, kr.NP[mdt])), ("all", np.ones(n, kr.NP[mdt]))]
    if n == 0:
        return out[:1]

    def only(*idx):
        m = np.zeros(n, kr.NP[mdt])
        m[list(idx)] = t(-3)
        return m

    out.append(("first", only(0)))
    out.append(("last", only(n - 1)))
    out.append(("alternating", (np.arange(n) % 2).astype(kr.NP[mdt])))
    out.append(("half", (_uniform(1)[:n] < 0.5).astype(kr.NP[mdt])))
    out.append(("sparse", (_uniform(2)[:n] < 1 / 64).astype(kr.NP[mdt])))
    if n >= TILE + 4:
        out.append(("straddle", only(*range(TILE - 3, TILE + 4))))
    if mdt != "i64":
        tiny = np.finfo(kr.NP[mdt]).smallest_subnormal
        cyc = np.array([np.nan, -0.0, tiny, 0.0, -tiny, 2.0, -0.0],
                       kr.NP[mdt])
        m = np.resize(cyc, n)
        assert (m != 0).tolist()[:7][:n] == [True, False, True, False, True,
                                              True, False][:n]
        out.append(("nan -0 denormal", m))
    return out


# ------------------------------------------------------- device plumbing
class Dev:
    """A device buffer holding `host` at an offset of `off` elements."""

    def __init__(self, ops, lib, host, off=0):
        self.ops, self.lib = ops, lib
        self.host = np.ascontiguousarray(host)
        self.esz = self.host.dtype.itemsize
        self.buf = ops._Buf((self.host.size + off) * self.esz)
        self.p = self.buf.p.value + off * self.esz
        if self.host.size:
            rc = lib.da_h2d(self.p, self.host.ctypes.data, self.host.nbytes)
            assert rc == 0

    def get(self):
        out = np.empty_like(self.host)
        if out.size:
            assert self.lib.da_d2h(self.p, out.ctypes.data, out.nbytes) == 0
        else:
            assert self.lib.da_synchronize() == 0
        return out

    def free(self):
        self.buf.free()


def sentinel(n, npdt):
    return np.frombuffer(bytes([SENT]) * (n * npdt.itemsize), npdt).copy()


def _abi_case(dja, dt, mdt, n, name, m, off):
    """Every da_compact / da_expand check of one (size, mask pattern)."""
    from distributedarrays_jl_amd import ops
    from distributedarrays_jl_amd._ffi import lib
    tag = (dt, mdt, n, name, off)
    npdt = kr.NP[dt]
    x = data(dt, 0)[:n]
    keep = np.flatnonzero(m != 0)
    K = keep.size
    devs = []

    def dev(host):
        d = Dev(ops, lib, host, off)
        devs.append(d)
        return d

    try:
        X, M = dev(x), dev(m)
        # -- compact with src; dst_cap = K, and K - 3 to test the guard: dst
        # really has K + 8 elements, so a broken guard fails, not faults
        for cap in sorted({K, max(K - 3, 0)}):
            Dst = dev(sentinel(K + 8, npdt))
            rc = lib.da_compact(Dst.p, cap, X.p, kr.DT[dt], M.p, kr.DT[mdt],
                                n, 0)
            assert rc == 0, (tag, lib.da_errstr(rc))
            got = Dst.get()
            assert same(got[:cap], x[keep][:cap]), (tag, cap)
            assert same(got[cap:], sentinel(K + 8 - cap, npdt)), (tag, cap)
            if cap == K:
                Kept = Dst
        # -- findall with a base beyond 32 bits
        base = (1 << 40) + 12345
        Idx = dev(sentinel(K + 8, kr.NP["i64"]))
        rc = lib.da_compact(Idx.p, K, None, kr.DT["i64"], M.p, kr.DT[mdt],
                            n, base)
        assert rc == 0, (tag, lib.da_errstr(rc))
        got = Idx.get()
        assert np.array_equal(got[:K], keep + base), tag
        assert same(got[K:], sentinel(8, kr.NP["i64"])), tag
        # -- src == mask
        if dt == mdt:
            Dst = dev(sentinel(K + 8, npdt))
            rc = lib.da_compact(Dst.p, K, M.p, kr.DT[dt], M.p, kr.DT[mdt],
                                n, 0)
            assert rc == 0, (tag, lib.da_errstr(rc))
            got = Dst.get()
            assert same(got[:K], m[keep]) and same(
                got[K:], sentinel(8, npdt)), tag
        # -- expand: the inverse, into other data
        prior = data(dt, 1)[:n]
        vals = data(dt, 2)[:K]
        V = dev(vals)
        for src_n in sorted({K, max(K - 3, 0)}):
            Dst = dev(prior)
            rc = lib.da_expand(Dst.p, kr.DT[dt], M.p, kr.DT[mdt], n, V.p,
                               src_n, 0)
            assert rc == 0, (tag, lib.da_errstr(rc))
            exp = prior.copy()
            exp[keep[:src_n]] = vals[:src_n]   # the tail stays untouched
            assert same(Dst.get(), exp), (tag, src_n)
        # -- expand a broadcast element
        Dst = dev(prior)
        rc = lib.da_expand(Dst.p, kr.DT[dt], M.p, kr.DT[mdt], n, V.p,
                           min(K, 1), 1)
        assert rc == 0, (tag, lib.da_errstr(rc))
        exp = prior.copy()
        if K:
            exp[keep] = vals[0]
        assert same(Dst.get(), exp), tag
        # -- expand with dst == mask
        if dt == mdt:
            Dst = dev(m)
            rc = lib.da_expand(Dst.p, kr.DT[dt], Dst.p, kr.DT[mdt], n, V.p,
                               K, 0)
            assert rc == 0, (tag, lib.da_errstr(rc))
            exp = m.copy()
            exp[keep] = vals
            assert same(Dst.get(), exp), tag
        # -- round trip: expand(compact(x)) into a copy of x is x
        Dst = dev(x)
        rc = lib.da_expand(Dst.p, kr.DT[dt], M.p, kr.DT[mdt], n, Kept.p, K,
                           0)
        assert rc == 0, (tag, lib.da_errstr(rc))
        assert same(Dst.get(), x), tag
        # the inputs are untouched
        assert same(X.get(), x) and same(M.get(), m), tag
    finally:
        assert lib.da_synchronize() == 0
        for d in devs:
            d.free()


@pytest.mark.parametrize("mdt", DTYPES)
@pytest.mark.parametrize("dt", DTYPES)
def test_abi_compact_expand(dja, dt, mdt):
    for n in SIZES:
        for k, (name, m) in enumerate(patterns(n, mdt)):
            # pointers offset by one element on every other case
            _abi_case(dja, dt, mdt, n, name, m, off=(k + (n & 1)) % 2)


# ------------------------------------------------- comparison numerics
_faulted = []


def run_child(script, env_extra, tag):
    """One child under its own timeout; none after one that died."""
    if _faulted:
        pytest.fail("an earlier child faulted (%s); not starting further "
                    "GPU processes" % _faulted[0])
    env = dict(os.environ)
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
    assert r.returncode == 0, "%s: child exit %d\n%s\n%s" % (
        tag, r.returncode, r.stdout[-2000:], r.stderr[-2000:])
    return r.stdout


@pytest.fixture(scope="module")
def interpreter_lines():
    """The child's lines (DA_EXPR_JIT=0: the interpreters), by group of
    cases; the child checks each against numpy itself."""
    out = run_child("cmp_bits_child.py", {"DA_EXPR_JIT": "0"},
                    "comparisons DA_EXPR_JIT=0")
    assert out.endswith("cmp done\n"), out[-500:]
    groups = {}
    for ln in out.splitlines()[:-1]:
        key, line = ln.split("|", 1)
        groups.setdefault(key, []).append(line)
    return groups


@pytest.mark.parametrize("dt,part", [(dt, part)
                                     for dt, parts in
                                     cmp_bits_child.PARTS.items()
                                     for part in parts])
def test_comparisons_jit_and_interpreter(dja, interpreter_lines, dt, part):
    """Both evaluators against numpy (inside lines()), and the same bits
    from both."""
    from distributedarrays_jl_amd._ffi import lib
    assert os.environ.get("DA_EXPR_JIT", "1") != "0"
    mine = cmp_bits_child.lines(dja, dt, part)
    assert lib.da_expr_jit_state() == 2, lib.da_expr_jit_errstr()
    # all six ops; "arr" and "const" add one Python operator each
    nconst = 3 if dt == "i64" else 2
    assert len(mine) == {"arr": 7, "const": 6 * nconst + 1,
                         "strided": 6}[part]
    assert interpreter_lines["%s %s" % (dt, part)] == mine


# ------------------------------------------------------------ Python API
def _kept(x, m):
    return x.ravel(order="F")[m.ravel(order="F") != 0]


def _assigned(x, m, v):
    flat = x.ravel(order="F").copy()
    flat[m.ravel(order="F") != 0] = v
    return np.asfortranarray(flat.reshape(x.shape, order="F"))


@pytest.mark.parametrize("shape", [(2049,), ((1 << 20) + 3,), (257, 33)])
@pytest.mark.parametrize("dt", DTYPES)
def test_python_api(dja, dt, shape):
    from distributedarrays_jl_amd import expr as E
    n = int(np.prod(shape))
    x = np.asfortranarray(data(dt, 3)[:n].reshape(shape, order="F"))
    c = 0 if dt == "i64" else 0.25
    with np.errstate(invalid="ignore"):
        m = (x > c)
    mh = np.asfortranarray(m.astype(kr.NP[dt]))
    D = dja.distribute(x)
    M = dja.distribute(mh)
    exp = _kept(x, mh)
    idx = np.flatnonzero(m.ravel(order="F"))
    for mask in (lambda t: t > c, E.ref(D) > c, E.gt(E.ref(D), c), M):
        R = dja.dfilter(mask, D)
        assert R.dtype == dt and R.dims == (exp.size,)
        assert same(R.collect(), exp)
        R.close()
        I = dja.dfindall(mask, D)
        assert I.dtype == "i64" and np.array_equal(I.collect(), idx)
        I.close()
    I = dja.dfindall(E.ref(D) > c)
    assert np.array_equal(I.collect(), idx)
    I.close()
    assert same(D[M], exp) and same(D[E.ref(D) > c], exp)
    # counts and quantifiers with comparison lambdas
    assert dja.dcount(lambda t: t > c, D) == idx.size
    assert dja.dany(lambda t: t > c, D) == bool(m.any())
    assert dja.dall(lambda t: t > c, D) == bool(m.all())
    assert dja.dall(lambda t: E.eq(t, t), D) == bool((x == x).all())
    assert dja.dany(lambda t: E.ne(t, t), D) == bool((x != x).any())
    lo = -(1 << 53) if dt == "i64" else -np.inf   # exact as a constant
    assert dja.dall(lambda t: t >= lo, D) == bool((x >= lo).all())
    assert dja.dany(lambda t: t <= lo, D) == bool((x <= lo).any())
    y = np.asfortranarray(data(dt, 4)[:n].reshape(shape, order="F"))
    Y = dja.distribute(y)
    with np.errstate(invalid="ignore"):
        assert dja.mapreduce(lambda a, b: E.lt(a, b), "add", D, Y) == \
            np.count_nonzero(x < y)
    # D[M] = scalar / ndarray / DVector; the mask as DArray and as a tree
    s = -7 if dt == "i64" else -0.0
    T = D.copy()
    T[M] = s
    assert same(T.collect(), _assigned(x, mh, s))
    v = data(dt, 5)[:exp.size].copy()
    T[M] = v
    assert same(T.collect(), _assigned(x, mh, v))
    V = dja.distribute(v[::-1].copy())
    T[E.ref(D) > c] = V
    assert same(T.collect(), _assigned(x, mh, v[::-1]))
    # the array as its own mask, in place on the device
    T[T] = s
    z = _assigned(x, mh, v[::-1])
    assert same(T.collect(), _assigned(z, z, s))
    from distributedarrays_jl_amd._ffi import DArrayError
    with pytest.raises(DArrayError):
        T[M] = v[:-1]
    assert same(T.collect(), _assigned(z, z, s))
    for t in (D, M, Y, T, V):
        t.close()


def test_nothing_left_allocated(dja):
    dja.d_closeall()
    assert dja.bytes_in_use() == 0
