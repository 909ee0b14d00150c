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


# ------------------------------------------------------- elementwise edges
EDGE_SIZES = (0, 1, 2, 3, 4, 5, 7, 8, 9, 255, 256, 257, 1023, 1024, 1025,
              4099)
# = 3 mod 4, and the smallest round length at which a capped grid
# (8192 blocks x 256 threads) takes a second trip through a vector-of-4
# loop (n/4 > 2^21); the vector-of-2 and scalar loops wrap from 2^22, 2^21
EDGE_WRAP = (1 << 23) + 4099
EDGE_GUARD = 64
EDGE_SENT = 0xA5                   # every byte of an unwritten element
EDGE_FAMILIES = ("fill", "map", "map2", "map2_scalar", "bcast_fma", "blas1",
                 "cast", "rand", "transpose", "diag_scale")
EDGE_MAP_HOT = ("identity", "neg", "abs", "abs2", "inv", "sqrt", "floor",
                "sign")
EDGE_MAP_COLD = "ceil"             # exact, and not a compile-time op
EDGE_MAP_I64 = ("identity", "neg", "abs", "abs2", "sign")
EDGE_MAP2 = ("add", "sub", "mul", "div", "min2", "max2")
EDGE_MAP2_I64 = ("add", "sub", "mul", "idiv", "mod", "rem", "and", "or",
                 "xor", "min2", "max2")
EDGE_OFFSETS = (0, 1, 2, 3, 5)     # odd and even; every residue mod 4
EDGE_SHAPES = ((1, 1), (1, 33), (33, 1), (31, 33), (64, 32), (65, 97))
_GOLD = 0x9E3779B97F4A7C15


def edge_input(dt, n, salt, specials=()):
    """x[j] = (j + salt) * golden ratio mod 2^64, as raw i64 or as a float
    in [-0.5, 0.5): every element names its index, so a shifted, dropped
    or repeated lane shows.  `specials` are planted at both ends (the
    first lanes and the scalar tail)."""
    with np.errstate(over="ignore"):
        u = (np.arange(n, dtype=np.uint64) + np.uint64(salt)) * \
            np.uint64(_GOLD)
    if dt == "i64":
        x = u.view(np.int64).copy()
    elif dt == "f64":
        x = (u >> np.uint64(11)).astype(np.float64) * 2.0 ** -53 - 0.5
    else:
        x = (u >> np.uint64(40)).astype(np.float32) * np.float32(2.0 ** -24) \
            - np.float32(0.5)
    for k, v in enumerate(specials):
        if k < n:
            x[k] = v
        if n - 1 - k >= len(specials):
            x[n - 1 - k] = v
    return x


def _np_map(op, x):
    """numpy value of the exact unary ops, in x's dtype.  sign keeps a NaN
    and a signed zero (Julia sign), which np.sign does not."""
    with np.errstate(all="ignore"):
        if op == "sign" and x.dtype.kind == "f":
            one = x.dtype.type(1)
            return np.where(x > 0, one, np.where(x < 0, -one, x))
        if op == "inv":
            return x.dtype.type(1) / x
        return {"identity": lambda v: v.copy(), "neg": lambda v: -v,
                "abs": np.abs, "abs2": lambda v: v * v, "sqrt": np.sqrt,
                "floor": np.floor, "ceil": np.ceil, "sign": np.sign}[op](x)


class _Edges:
    """Guarded destinations and a list of everything that did not match:
    one GPU run reports every failing (family, dtype, size), not the first."""

    def __init__(self):
        from distributedarrays_jl_amd._ffi import lib, check
        from distributedarrays_jl_amd import _opcodes as oc
        self.lib, self.check, self.oc = lib, check, oc
        self.bad = []
        self.bufs = []

    def dev(self, arr):
        b = kr.Dev.of(arr)
        self.bufs.append(b)
        return b

    def dest(self, dt, n, init=None):
        """n elements (sentinel bytes, or `init`) and EDGE_GUARD sentinel
        elements after them."""
        host = np.empty(n + EDGE_GUARD, dtype=kr.NP[dt])
        host.view(np.uint8)[:] = EDGE_SENT
        if init is not None:
            host[:n] = init
        return self.dev(host)

    def expect(self, tag, buf, want):
        n = want.size
        got = buf.get(want.dtype, n + EDGE_GUARD)
        if not (got[n:].view(np.uint8) == EDGE_SENT).all():
            self.bad.append("%r: guard after %d elements overwritten"
                            % (tag, n))
        diff = np.flatnonzero(kr.bits(got[:n]) != kr.bits(want))
        if diff.size:
            j = int(diff[0])
            self.bad.append("%r: %d/%d differ, first at %d: got %r want %r"
                            % (tag, diff.size, n, j, got[j], want[j]))

    def free(self):
        while self.bufs:
            self.bufs.pop().free()


def _edge_fill(e, n, wrap):
    for dt, v in (("f64", 2.5), ("f32", -1.25), ("i64", -7.0)):
        d = e.dest(dt, n)
        e.check(e.lib.da_fill(d.p, v, n, kr.DT[dt]))
        e.expect(("fill", dt, n), d, np.full(n, v, dtype=kr.NP[dt]))
        e.free()


def _edge_map(e, n, wrap):
    def run(op, dt, x, inplace=False):
        src = e.dev(x)
        dst = e.dest(dt, n, x if inplace else None)
        e.check(e.lib.da_map(e.oc.MAP_OP[op], dst.p,
                             dst.p if inplace else src.p, n, kr.DT[dt]))
        e.expect(("map", op, dt, n, inplace), dst, _np_map(op, x))
        e.free()

    for dt in ("f64", "f32"):
        nan, t = np.nan, kr.NP[dt].type
        x = edge_input(dt, n, 3, (nan, -0.0, 0.0))
        for op in (("abs2", EDGE_MAP_COLD) if wrap
                   else EDGE_MAP_HOT + (EDGE_MAP_COLD,)):
            xin = x
            if op in ("inv", "sqrt"):
                # no NaN in: a division or root of one need not keep its
                # sign and payload; sqrt of non-negatives only
                xin = edge_input(dt, n, 3, (-0.0, 0.0))
                if op == "sqrt":
                    xin = np.abs(xin) * t(4)
                    xin[:2] = (-0.0, 0.0)[:n]      # sqrt(-0.0) = -0.0
            run(op, dt, xin * t(8) if op in ("floor", "ceil") else xin)
        if not wrap:
            run("abs2", dt, x, inplace=True)   # dst == src exactly
    xi = edge_input("i64", n, 5, (0, -1, kr.I64_MIN))
    for op in (("neg",) if wrap else EDGE_MAP_I64):
        run(op, "i64", xi)


def _map2_inputs(dt, n, for_scalar_rev=False):
    if dt == "i64":
        a = edge_input(dt, n, 13)
        with np.errstate(over="ignore"):
            b = np.abs(edge_input(dt, n, 14)) % 1000 + 1
        return (b if for_scalar_rev else a), b
    t = kr.NP[dt].type
    a = edge_input(dt, n, 11, (np.nan, -0.0, 1.0))
    b = edge_input(dt, n, 12) + t(1.0)          # in [0.5, 1.5): no zero
    b = b.astype(kr.NP[dt])
    for k, v in enumerate((0.25, 3.0, np.nan)):  # a NaN on this side too,
        if k < n:                                # never opposite a's
            b[k] = v
        if n - 1 - k >= 3:
            b[n - 1 - k] = v
    return a, b


def _no_nan(x):
    """x with every NaN replaced: the subtrahend of `sub` carries none.
    IEEE 754 leaves the sign of a propagated NaN open, and a - b may be
    evaluated as a + (-b), which flips it."""
    y = x.copy()
    y[np.isnan(y)] = 2.0
    return y


def _edge_rejects_cmp(e, fn, dt, n):
    """The comparisons (da_cmpop) belong to expression programs; da_map2
    and da_map2_scalar refuse them and write nothing."""
    d = e.dest(dt, n)
    for name, code in sorted(e.oc.CMP_OPS.items()):
        rc = fn(code, d.p)
        if n and rc != -3:
            e.bad.append("%s %s %s n=%d: rc %d, want -3" % (
                fn.__name__, name, dt, n, rc))
        if not n and rc != 0:
            e.bad.append("%s %s %s n=0: rc %d" % (fn.__name__, name, dt, rc))
    got = d.get(np.uint8, d.nbytes)
    if not (got == EDGE_SENT).all():
        e.bad.append("%s cmp %s n=%d: refused call wrote" % (
            fn.__name__, dt, n))


def _edge_map2(e, n, wrap):
    from oracle import ops as oops
    for dt in ("f64", "f32", "i64"):
        a, b = _map2_inputs(dt, n)
        da, db = e.dev(a), e.dev(b)
        ops = EDGE_MAP2_I64 if dt == "i64" else EDGE_MAP2
        b_sub, db_sub = b, db
        if dt != "i64":
            b_sub = _no_nan(b)
            db_sub = e.dev(b_sub)
        for op in (ops[2:3] if wrap else ops):
            d = e.dest(dt, n)
            bb, dbb = (b_sub, db_sub) if op == "sub" else (b, db)
            e.check(e.lib.da_map2(e.oc.MAP2_OP[op], d.p, da.p, dbb.p, n,
                                  kr.DT[dt]))
            with np.errstate(all="ignore"):
                want = oops.oracle_map2(op, a, bb)
            e.expect(("map2", op, dt, n), d, want)
        if not wrap:
            def map2(code, p):
                return e.lib.da_map2(code, p, da.p, db.p, n, kr.DT[dt])
            _edge_rejects_cmp(e, map2, dt, n)
        e.free()


def _edge_map2_scalar(e, n, wrap):
    from oracle import ops as oops
    for dt in ("f64", "f32", "i64"):
        c = kr.NP[dt].type(7 if dt == "i64" else 0.75)
        ops = EDGE_MAP2_I64 if dt == "i64" else EDGE_MAP2
        for rev in (0, 1):
            if wrap and rev:
                continue
            a, _ = _map2_inputs(dt, n, for_scalar_rev=bool(rev))
            da = e.dev(a)
            a_sub, da_sub = a, da
            if dt != "i64" and rev:       # c - a: a is the subtrahend
                a_sub = _no_nan(a)
                da_sub = e.dev(a_sub)
            for op in (ops[1:2] if wrap else ops):
                d = e.dest(dt, n)
                aa, daa = (a_sub, da_sub) if op == "sub" else (a, da)
                e.check(e.lib.da_map2_scalar(e.oc.MAP2_OP[op], d.p, daa.p,
                                             float(c), rev, n, kr.DT[dt]))
                with np.errstate(all="ignore"):
                    want = oops.oracle_map2(op, c, aa) if rev \
                        else oops.oracle_map2(op, aa, c)
                e.expect(("map2_scalar", op, dt, n, rev), d,
                         np.asarray(want, dtype=kr.NP[dt]))
            if not wrap:
                def map2_scalar(code, p):
                    return e.lib.da_map2_scalar(code, p, da.p, float(c), rev,
                                                n, kr.DT[dt])
                _edge_rejects_cmp(e, map2_scalar, dt, n)
            e.free()


def _edge_bcast_fma(e, n, wrap):
    from oracle import ops as oops
    for dt in ("f64", "f32"):
        a, b = edge_input(dt, n, 21), edge_input(dt, n, 22)
        da, db, d = e.dev(a), e.dev(b), e.dest(dt, n)
        e.check(e.lib.da_bcast_fma(d.p, da.p, db.p, 0.25, n, kr.DT[dt]))
        e.expect(("bcast_fma", dt, n), d, oops.oracle_bcast_fma(a, b, 0.25))
        e.free()


def _edge_blas1(e, n, wrap):
    """axpby, add (unit and scaled) and scale: the in-place kernels."""
    from oracle import ops as oops
    for dt in ("f64", "f32", "i64"):
        x, y = edge_input(dt, n, 31), edge_input(dt, n, 32)
        dx = e.dev(x)
        if dt != "i64":
            d = e.dest(dt, n, y)
            e.check(e.lib.da_axpby(d.p, dx.p, -0.5, 1.0, n, kr.DT[dt]))
            e.expect(("axpby", dt, n), d, oops.oracle_axpy(-0.5, x, y))
        for s in ((-0.5,) if wrap else (1.0, -0.5, 3.0)):
            d = e.dest(dt, n, y)
            e.check(e.lib.da_add(d.p, dx.p, s, n, kr.DT[dt]))
            e.expect(("add", s, dt, n), d, oops.oracle_add(y, x, s))
        for s in ((3.0,) if wrap else (-0.5, 3.0)):
            d = e.dest(dt, n, y)
            e.check(e.lib.da_scale(d.p, s, n, kr.DT[dt]))
            e.expect(("scale", s, dt, n), d, oops.oracle_scale(y, s))
        e.free()


def _edge_cast(e, n, wrap):
    ties = (0.5, -0.5, 1.5, -1.5, 2.5, -2.5)   # float -> i64 rounds half-even
    for sd in ("f64", "f32", "i64"):
        if sd == "i64":
            x = edge_input(sd, n, 41, (0, -1, kr.I64_MAX, kr.I64_MIN))
        else:
            x = edge_input(sd, n, 41) * kr.NP[sd].type(1000)
            for k, v in enumerate(ties):
                if k < n:
                    x[k] = v
                if n - 1 - k >= len(ties):
                    x[n - 1 - k] = v
        dx = e.dev(x)
        for dd in ("f64", "f32", "i64"):
            if dd == sd:
                continue
            d = e.dest(dd, n)
            e.check(e.lib.da_cast(d.p, kr.DT[dd], dx.p, kr.DT[sd], n))
            want = (np.rint(x) if dd == "i64" else x).astype(kr.NP[dd])
            e.expect(("cast", dd, sd, n), d, want)
        e.free()


def _rand_windows(n, wrap):
    """Whole array, or at the wrap length the stretches where an indexing
    slip can show: both ends and 4096 elements either side of 2^22 and
    2^23, where a capped grid starts another trip (2 and 4 outputs per
    philox block).  The philox reference costs seconds per 2^23 elements
    on the host, and between those points every trip runs the same code;
    that every element in between was written is checked separately."""
    if not wrap:
        return [(0, n)]
    return [(max(0, p - 4096), min(n, p + 4096))
            for p in (0, 1 << 22, 1 << 23, n)]


def _edge_rand(e, n, wrap):
    from oracle import philox
    seed = 4321
    refs = {("f64", 0): philox.fill_uniform_f64,
            ("f32", 0): philox.fill_uniform_f32,
            ("i64", 0): philox.fill_int64,
            ("f64", 1): philox.fill_normal_f64}
    for off in ((3,) if wrap else EDGE_OFFSETS):
        for dt, kind in (("f64", 0), ("f32", 0), ("i64", 0), ("f64", 1),
                         ("f32", 1)):
            tag = ("rand", "normal" if kind else "uniform", dt, n, off)
            d = e.dest(dt, n)
            e.check(e.lib.da_rand(d.p, n, kr.DT[dt], seed, kind, off))
            got = d.get(kr.NP[dt], n + EDGE_GUARD)
            if not (got[n:].view(np.uint8) == EDGE_SENT).all():
                e.bad.append("%r: guard overwritten" % (tag,))
            sent = got[n:n + 1]
            if n and (kr.bits(got[:n]) == kr.bits(sent)[0]).any():
                e.bad.append("%r: elements left unwritten" % (tag,))
            if (dt, kind) == ("f32", 1):    # bits pinned by the digests
                if not np.isfinite(got[:n]).all():
                    e.bad.append("%r: not finite" % (tag,))
                continue
            for lo, hi in _rand_windows(n, wrap):
                ref = refs[dt, kind](hi - lo, seed, off + lo)
                if kind:
                    ok = np.allclose(got[lo:hi], ref, rtol=1e-12, atol=1e-12)
                else:
                    ok = np.array_equal(kr.bits(got[lo:hi]), kr.bits(ref))
                if not ok:
                    j = int(np.flatnonzero(got[lo:hi] != ref)[0])
                    e.bad.append("%r: [%d, %d) differs, first at %d: got %r "
                                 "want %r" % (tag, lo, hi, lo + j,
                                              got[lo + j], ref[j]))
            e.free()


def _edge_transpose(e, shape, wrap):
    m, n = shape
    for dt in ("f64", "f32", "i64"):
        x = edge_input(dt, m * n, 51)
        dx, d = e.dev(x), e.dest(dt, m * n)
        e.check(e.lib.da_transpose(d.p, dx.p, m, n, kr.DT[dt]))
        want = x.reshape((m, n), order="F").T.ravel(order="F")
        e.expect(("transpose", dt, m, n), d, want)
        e.free()


def _edge_diag_scale(e, shape, wrap):
    m, n = shape
    for dt in ("f64", "f32"):
        x = edge_input(dt, m * n, 61)
        for side in (0, 1):
            dg = edge_input(dt, (m, n)[side], 62)
            ddg, d = e.dev(dg), e.dest(dt, m * n, x)
            e.check(e.lib.da_diag_scale(d.p, m, n, ddg.p, side, kr.DT[dt]))
            X = x.reshape((m, n), order="F")
            want = X * dg[:, None] if side == 0 else X * dg[None, :]
            e.expect(("diag_scale", dt, m, n, side), d,
                     want.ravel(order="F"))
            e.free()


_EDGE_RUN = {"fill": _edge_fill, "map": _edge_map, "map2": _edge_map2,
             "map2_scalar": _edge_map2_scalar, "bcast_fma": _edge_bcast_fma,
             "blas1": _edge_blas1, "cast": _edge_cast, "rand": _edge_rand,
             "transpose": _edge_transpose, "diag_scale": _edge_diag_scale}


def check_elementwise_edges(dja, sizes=EDGE_SIZES, wrap=EDGE_WRAP,
                            families=EDGE_FAMILIES):
    """Every launcher of kernels_elementwise at ABI level, every dtype it
    accepts, at each length in `sizes` with all ops and once per family and
    dtype at the `wrap` length (None: skip).  Destinations carry EDGE_GUARD
    sentinel elements after n; results and guard are compared bit for bit
    (f64 normals: rtol = atol = 1e-12; f32 normals: finite, guard only).
    dja is the initialised package (comm.init done)."""
    e = _Edges()
    try:
        for fam in families:
            run = _EDGE_RUN[fam]
            if fam in ("transpose", "diag_scale"):
                for shape in EDGE_SHAPES:
                    run(e, shape, False)
                continue
            for n in sizes:
                run(e, n, False)
            if wrap:
                run(e, wrap, True)
            e.check(e.lib.da_synchronize())
    finally:
        e.free()
    assert not e.bad, "%d mismatches:\n%s" % (len(e.bad),
                                               "\n".join(e.bad[:40]))
