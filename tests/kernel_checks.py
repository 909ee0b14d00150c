"""GPU check routines shared by test_gpu_reduce_tree, test_gpu_gemm_exact
and variant_child (which reruns a reduced set of them in a fresh process
per env-gated kernel variant).  Each routine asserts; none tunes a
tolerance — see kernel_ref for the bounds."""
import ctypes
import functools

import numpy as np

import kernel_ref as kr

TREE_N = (1 << 20) + 1     # 2048 blocks, odd length, one-element scalar tail


# ------------------------------------------------------------- flat reduce
def tree_positions(n):
    """Planting sites: first/last element, wave and block edges of the
    vector-of-2 grid-stride loop, the last block's last pair (n-3, n-2 for
    odd n), the scalar tail (n-1) and one index in the middle."""
    want = [0, 1, 63, 64, 255, 256, 511, 512, n - 3, n - 2, n - 1, n // 2 + 7]
    out = []
    for p in want:
        if 0 <= p < n and p not in out:
            out.append(p)
    return out


@functools.lru_cache(maxsize=8)
def tree_base(n, dt):
    """philox uniform [0,1) (floats) / values in [-8,8] (i64); read-only."""
    x = kr.uniform(n, dt, 40 + kr.DT[dt])
    x.setflags(write=False)
    return x


def sentinels(dt):
    """(max sentinel, min sentinel): outside the base data's range."""
    if dt == "i64":
        return np.int64(kr.I64_MAX), np.int64(kr.I64_MIN)
    return kr.NP[dt].type(2.0), kr.NP[dt].type(-2.0)


def poke(d, idx, value):
    """Overwrite one element of a single-chunk DArray in place."""
    from distributedarrays_jl_amd._ffi import lib, check
    v = np.array([value], dtype=kr.NP[d.dtype])
    check(lib.da_h2d(d.at_byte(idx * v.itemsize), v.ctypes.data, v.itemsize))


def check_planted_extrema(dja, dt, n):
    """One maximum and one minimum sentinel, at every planting site in
    turn: dmaximum/dminimum/dextrema must return exactly the sentinels."""
    base = tree_base(n, dt)
    hi, lo = sentinels(dt)
    pos = tree_positions(n)
    d = dja.distribute(base)
    try:
        for j, p in enumerate(pos):
            q = pos[(j + 1) % len(pos)]
            poke(d, p, hi)
            if q != p:
                poke(d, q, lo)
            want_lo = lo if q != p else hi
            got = (dja.dmaximum(d), dja.dminimum(d), dja.dextrema(d))
            assert got[0] == hi, (dt, n, p, q, got)
            assert got[1] == want_lo, (dt, n, p, q, got)
            assert got[2] == (want_lo, hi), (dt, n, p, q, got)
            if q == p:            # n == 1: the lone element as minimum too
                poke(d, p, lo)
                assert dja.dextrema(d) == (lo, lo), (dt, n)
            poke(d, p, base[p])
            poke(d, q, base[q])
        assert dja.dmaximum(d) == base.max(), "restore failed"
    finally:
        d.close()


def check_planted_nan(dja, dt, n):
    """A single NaN at every planting site in turn reaches the result of
    every fold, through stage 1, the block tree and the cross-block fold."""
    base = tree_base(n, dt)
    d = dja.distribute(base)
    try:
        for p in tree_positions(n):
            poke(d, p, np.nan)
            for name in ("dmaximum", "dminimum", "dsum"):
                got = getattr(dja, name)(d)
                assert got != got, (name, dt, n, p, got)
            assert dja.dcount("isnan", d) == 1, (dt, n, p)
            assert dja.dany("isnan", d), (dt, n, p)
            assert not dja.dall("isfinite", d), (dt, n, p)
            poke(d, p, base[p])
        assert dja.dcount("isnan", d) == 0
        assert dja.dall("isfinite", d)
    finally:
        d.close()


def golden_sequence(n):
    """x[j] = j * 0x9E3779B97F4A7C15 mod 2^64: the sum of a subset names the
    subset, so a dropped or doubled element changes the wrapped sum."""
    with np.errstate(over="ignore"):
        x = np.arange(n, dtype=np.uint64) * np.uint64(0x9E3779B97F4A7C15)
    return x.view(np.int64)


def check_once_only(dja, n):
    x = golden_sequence(n)
    d = dja.distribute(x)
    try:
        with np.errstate(over="ignore"):
            want = int(x.sum(dtype=np.int64))
        got = dja.dsum(d)
        assert got == want, (n, got, want)
    finally:
        d.close()


def check_sum_in_bound(dja, dt, n, seed):
    """dsum against the longdouble sum, any-order bound (n-1)*u*sum|x|;
    i64 exact.  Also dmaximum, exact."""
    x = kr.uniform(n, dt, seed)
    if dt != "i64":
        x = x - kr.NP[dt].type(0.5)
    d = dja.distribute(x)
    try:
        got = dja.dsum(d)
        if dt == "i64":
            assert got == int(x.sum()), (dt, n, got)
        else:
            w = x.astype(np.longdouble)
            bound = (n - 1) * np.longdouble(kr.UNIT[dt]) * np.abs(w).sum()
            assert abs(np.longdouble(got) - w.sum()) <= bound, (dt, n, got)
        assert dja.dmaximum(d) == x.max(), (dt, n)
    finally:
        d.close()


# ---------------------------------------------------------------- map math
def check_map_ulp(dja, n=2000):
    """f64 sin/cos/exp through da_map on a small hard vector (specials at
    both ends, length = 3 mod 4): <= 1 ulp against mpmath on the fast
    range and the bits of the CPU model.  Run under DA_MAP_W=2 by
    variant_child, this covers the vector-of-2 kernels; the full sweep is
    in test_gpu_math_ulp."""
    import fastmath_model as fm
    import ulp_ref as U
    for op in ("sin", "cos", "exp"):
        x = U.with_specials(U.sweep(op, "f64", n=n), U.specials("f64"))
        ref = U.reference(op, x, "f64", use_mp=True)
        d = dja.distribute(x)
        out = dja.dmap(op, d)
        try:
            got = out.localpart().copy()
        finally:
            out.close(); d.close()
        err = U.ulp_err(got, ref, "f64")
        fast = fm.fast_range(op, x)
        w, at = U.worst(err[fast], x[fast])
        print("map %s f64, %d elements: worst %.4f ulp at %r" % (
            op, x.size, w, float(at)))
        assert w <= 1.0 + U.REF_SLACK, (op, w, float(at))
        assert err[~fast].max() <= 3.0 + U.REF_SLACK, (op, err[~fast].max())
        assert np.array_equal(kr.bits(got[fast]),
                              kr.bits(fm.MODEL[op](x[fast]))), op


# -------------------------------------------------------------------- gemm
GEMM_FN = {"f64": "da_gemm_f64", "f32": "da_gemm_f32", "i64": "da_gemm_i64"}


def gemm_path(lib, m, n, k):
    from distributedarrays_jl_amd import _ffi
    return _ffi.GEMM_PATHS[lib.dbg_gemm_path(m, n, k)]


class Panel:
    """rows x cols block at (top, left) inside a Fortran-order parent whose
    every other element holds `border` (NaN for float operands)."""

    def __init__(self, block, top=0, bottom=0, left=0, right=0, border=None):
        rows, cols = block.shape
        dt = block.dtype
        if border is None:
            border = np.nan if dt.kind == "f" else -(1 << 40) - 1
        self.ld = top + rows + bottom
        self.host = np.full((self.ld, left + cols + right), border, dtype=dt,
                            order="F")
        self.sl = (slice(top, top + rows), slice(left, left + cols))
        self.host[self.sl] = block
        self.byte_off = (left * self.ld + top) * dt.itemsize
        self.dev = kr.Dev.of(self.host)

    def ptr(self):
        return self.dev.at(self.byte_off)

    def fetch(self):
        return self.dev.get(self.host.dtype, self.host.size).reshape(
            self.host.shape, order="F")

    def free(self):
        self.dev.free()


def gemm_exact(lib, dt, m, n, k, alpha=1, beta=0, c_block=None, layout=None,
               a_block=None, want=None):
    """Run C = alpha*A*B + beta*C on integer-valued inputs and require the
    exact int64 result in C's block and unchanged bits everywhere else in
    C's parent.

    layout: dict of Panel margins per operand, e.g. {"A": dict(bottom=16)}.
    c_block: initial C block (default: integers in [-4,4]; NaN allowed when
    beta == 0).  a_block overrides A (e.g. NaN-poisoned, alpha == 0).
    want: expected int64 block when it is not alpha*A*B + beta*C0."""
    from distributedarrays_jl_amd._ffi import check
    layout = layout or {}
    A, B = kr.gemm_int_inputs(m, n, k, dt, 1000 + 7 * m + 3 * n + k)
    if c_block is None:
        c_block = kr.small_ints(m * n, 77, 4).reshape((m, n), order="F") \
            .astype(kr.NP[dt])
    if want is None:
        with np.errstate(over="ignore"):
            want = kr.gemm_int_reference(A, B, c_block, alpha, beta)
    if a_block is not None:
        A = a_block
    pa = Panel(A, **layout.get("A", {}))
    pb = Panel(B, **layout.get("B", {}))
    pc = Panel(c_block, **layout.get("C", {}))
    try:
        ab = (ctypes.c_int64(alpha), ctypes.c_int64(beta)) if dt == "i64" \
            else (ctypes.c_double(alpha), ctypes.c_double(beta))
        check(getattr(lib, GEMM_FN[dt])(pc.ptr(), pa.ptr(), pb.ptr(), m, n, k,
                                        pa.ld, pb.ld, pc.ld, *ab))
        check(lib.da_synchronize())
        got = pc.fetch()
        blk = got[pc.sl]
        tag = (dt, m, n, k, alpha, beta, sorted(layout))
        if dt != "i64":
            assert not np.isnan(blk).any(), tag
        assert np.array_equal(blk, want.astype(kr.NP[dt])), tag
        got[pc.sl] = pc.host[pc.sl]
        assert np.array_equal(kr.bits(np.ravel(got, order="F")),
                              kr.bits(np.ravel(pc.host, order="F"))), \
            "C outside the %dx%d block was written: %r" % (m, n, tag)
    finally:
        pc.free(); pb.free(); pa.free()


def padded(dt=None):
    """lda = m+16, ldb = k+16, ldc = m+16: NaN pad rows under A and B, a
    sentinel under C."""
    return {"A": dict(bottom=16), "B": dict(bottom=16),
            "C": dict(bottom=16, border=-777)}


def submatrix(dt):
    """Each operand sits `b` rows and columns inside a NaN-bordered parent.
    b = 16 elements for 8-byte types and 32 for f32, so the byte offset
    (b*ld + b)*itemsize is a multiple of 128 and ld stays 16-aligned."""
    b = 32 if dt == "f32" else 16
    m = dict(top=b, bottom=b, left=b, right=b)
    return {"A": dict(m), "B": dict(m), "C": dict(m)}


def nan_block(m, n, dt):
    return np.full((m, n), np.nan, dtype=kr.NP[dt], order="F")


def gemm_real_in_bound(lib, dt, m, n, k):
    """Real-valued inputs: |got - ref| <= k*u*(|A|.|B|) elementwise."""
    from distributedarrays_jl_amd._ffi import check
    t = kr.NP[dt].type
    A = np.asfortranarray((kr.uniform(m * k, dt, 11) - t(0.5))
                          .reshape((m, k), order="F"))
    B = np.asfortranarray((kr.uniform(k * n, dt, 12) - t(0.5))
                          .reshape((k, n), order="F"))
    ref, bound = kr.gemm_real_reference(A, B, dt)
    da, db = kr.Dev.of(A), kr.Dev.of(B)
    dc = kr.Dev.of(nan_block(m, n, dt))
    try:
        check(getattr(lib, GEMM_FN[dt])(dc.p, da.p, db.p, m, n, k, m, k, m,
                                        ctypes.c_double(1.0),
                                        ctypes.c_double(0.0)))
        check(lib.da_synchronize())
        got = dc.get(kr.NP[dt], m * n).reshape((m, n), order="F")
    finally:
        dc.free(); db.free(); da.free()
    err = np.abs(got.astype(ref.dtype) - ref)
    print("gemm %s %dx%dx%d: max err %.3e, min slack %.3e" % (
        dt, m, n, k, float(err.max()), float((bound - err).min())))
    assert (err <= bound).all(), (dt, m, n, k, float(err.max()))
