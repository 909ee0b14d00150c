"""da_scan on the GPU: every kernel family (cols / block / spans, pinned
through dbg_scan_variant before each launch) at its tile, span and
threshold edges, with and without a carry, out of place and in place,
aligned and misaligned; then the Python API at world 1.

Exact checks (bit for bit; by value for min/max so a signed zero does not
matter) use data on which ANY bracketing gives the same result:
  - every i64 op on raw philox bits (wrap-around on both sides);
  - min/max on every dtype;
  - float add on integers: |x| <= 3 for f32 keeps every prefix below 2^24
    up to n = 2^22+1 (3*(2^22+2) < 2^24); |x| <= 8 is safe for f64;
  - float mul on ones with at most 44 powers of two 2^+-e, e <= 3, the
    sign of the exponent alternating: every prefix is a power of two
    within 2^+-66 (2^+-67 with a 2^+-1 carry).
Bounded checks (philox uniform - 0.5, near-one data for products) use the
first-order any-order bounds against a longdouble reference, the carry
counting as a term: |err_k| <= k*u*sum_{i<=k}|x_i| for the k-term prefix
of a sum, relative error <= k*u/(1-k*u) for a product."""
import ctypes

import numpy as np
import pytest

import kernel_ref as kr

pytestmark = pytest.mark.gpu

T = 2048             # SCAN_TILE
BLOCK_LINES = 512    # SCAN_BLOCK_LINES
GMAX = 2048          # SCAN_GMAX: spans per launch
DTYPES = ["f64", "f32", "i64"]
OPS = ["add", "mul", "min", "max"]
UF = {"add": np.add, "mul": np.multiply, "min": np.minimum,
      "max": np.maximum}
CTYPE = {"f64": ctypes.c_double, "f32": ctypes.c_float, "i64": ctypes.c_int64}


@pytest.fixture(scope="module")
def dja():
    import distributedarrays_jl_amd as dja
    dja.comm.init()
    return dja


def family(inner, axis, outer):
    from distributedarrays_jl_amd import _ffi
    return _ffi.SCAN_VARIANTS[_ffi.lib.dbg_scan_variant(inner, axis, outer)]


# ------------------------------------------------------------------ data
def product_data(n, dt, seed):
    """Ones with <= 44 powers of two 2^+-e, 1 <= e <= 3, at philox-drawn
    sites, the sign of the exponent alternating from site to site: every
    prefix product of every line is a power of two within 2^+-66."""
    x = np.ones(n, dtype=kr.NP[dt])
    if n == 0:
        return x
    sites = sorted(set(int(p) for p in
                       np.mod(kr.philox.fill_int64(44, seed), n)))
    for k, p in enumerate(sites):
        e = (k // 2) % 3 + 1
        x[p] = 2.0 ** (e if k % 2 == 0 else -e)
    return x


def exact_data(op, n, dt, seed):
    if n == 0:
        return np.zeros(0, dtype=kr.NP[dt])
    if dt == "i64":
        return kr.philox.fill_int64(n, seed)
    if op == "add":
        return kr.small_ints(n, seed, 3 if dt == "f32" else 8).astype(
            kr.NP[dt])
    if op == "mul":
        return product_data(n, dt, seed)
    return kr.uniform(n, dt, seed) - kr.NP[dt].type(0.5)


def exact_carry(op, m, dt, seed):
    if dt != "i64" and op == "mul":
        s = kr.small_ints(m, seed, 1)
        return np.where(s > 0, 2.0, np.where(s < 0, -0.5, 1.0)).astype(
            kr.NP[dt])
    return exact_data(op, m, dt, seed)


def exact_reference(op, x, shape, carry):
    """numpy accumulate along the middle axis of the column-major view,
    the carry folded in front; flat, in the kernel's element order."""
    inner, axis, outer = shape
    v = x.reshape(shape, order="F")
    with np.errstate(over="ignore"):
        r = UF[op].accumulate(v, axis=1) if axis else v
        if carry is not None and axis:
            r = UF[op](carry.reshape((inner, 1, outer), order="F"), r)
    return np.asfortranarray(r).ravel(order="F")


# ---------------------------------------------------------------- driver
class Bufs:
    """Device buffers of one shape and dtype, reused across ops: src, dst
    (each with 64 spare bytes so a test can shift them) and carry."""

    def __init__(self, shape, dt):
        self.shape, self.dt = shape, dt
        self.n = shape[0] * shape[1] * shape[2]
        self.m = shape[0] * shape[2]
        self.esz = kr.NP[dt].itemsize
        self.src = kr.Dev(self.n * self.esz + 64)
        self.dst = kr.Dev(self.n * self.esz + 64)
        self.car = kr.Dev(self.m * self.esz + 64)

    def free(self):
        for b in (self.src, self.dst, self.car):
            b.free()

    def scan(self, op, x, carry=None, inplace=False, src_off=0, dst_off=0):
        from distributedarrays_jl_amd._ffi import lib, check
        x = np.ascontiguousarray(x, dtype=kr.NP[self.dt])
        assert x.size == self.n
        sp = self.src.at(src_off)
        dp = sp if inplace else self.dst.at(dst_off)
        if self.n:
            check(lib.da_h2d(sp, x.ctypes.data, x.nbytes))
        cp = None
        if carry is not None:
            c = np.ascontiguousarray(carry, dtype=kr.NP[self.dt])
            assert c.size == self.m
            cp = self.car.p
            if self.m:
                check(lib.da_h2d(cp, c.ctypes.data, c.nbytes))
        if not inplace and self.n:
            # poison, so an element the kernel skips cannot pass
            junk = np.full(self.n, 0x55, dtype=np.uint8).repeat(self.esz)
            check(lib.da_h2d(dp, junk.ctypes.data, junk.nbytes))
        i, a, o = self.shape
        check(lib.da_scan(kr.REDOP[op], dp, sp, i, a, o, kr.DT[self.dt], cp))
        out = np.empty(self.n, dtype=kr.NP[self.dt])
        if self.n:
            check(lib.da_d2h(dp, out.ctypes.data, out.nbytes))
        return out


def assert_same(op, got, ref, tag):
    assert got.dtype == ref.dtype, tag
    if op in ("min", "max"):
        bad = np.flatnonzero(got != ref)
    else:
        bad = np.flatnonzero(kr.bits(got) != kr.bits(ref))
    assert bad.size == 0, "%r: %d/%d differ, first at %d: got %r ref %r" % (
        tag, bad.size, got.size, int(bad[0]), got[bad[0]], ref[bad[0]])


def check_exact_shape(shape, dt, fam, seed, ops=OPS):
    """Every op: without carry, with carry, and once in place (the carry
    alternating), all exact."""
    assert family(*shape) == fam, (shape, family(*shape))
    b = Bufs(shape, dt)
    try:
        for k, op in enumerate(ops):
            x = exact_data(op, b.n, dt, seed + k)
            c = exact_carry(op, b.m, dt, seed + 10 + k)
            got = b.scan(op, x)
            assert_same(op, got, exact_reference(op, x, shape, None),
                        (shape, dt, op, "no carry"))
            got = b.scan(op, x, carry=c)
            assert_same(op, got, exact_reference(op, x, shape, c),
                        (shape, dt, op, "carry"))
            ci = c if k % 2 else None
            got = b.scan(op, x, carry=ci, inplace=True)
            assert_same(op, got, exact_reference(op, x, shape, ci),
                        (shape, dt, op, "in place"))
    finally:
        b.free()


# ------------------------------------------------- inner == 1, few lines
def line_family(n):
    return "spans" if n > T else "block"


LINE_EDGES = [0, 1, 2, 63, 64, 65, 255, 256, 257, T - 1, T, T + 1,
              2 * T - 1, 2 * T, 2 * T + 1, 3 * T + 5]


@pytest.mark.parametrize("dt", DTYPES)
@pytest.mark.parametrize("n", LINE_EDGES)
def test_one_line_edges(dja, n, dt):
    """Line lengths around a wave, a block row and a tile; above one tile
    the line is cut into spans of one tile each (one span +- 1, two spans
    +- 1)."""
    check_exact_shape((1, n, 1), dt, line_family(n), 100 + n % 97)


@pytest.mark.parametrize("dt", DTYPES)
@pytest.mark.parametrize("n", [(1 << 20) + 1, GMAX * T, GMAX * T + 1])
def test_spans_large(dja, n, dt):
    """513 spans (more than one row of the last arriver's scan of the
    totals), exactly GMAX one-tile spans, and GMAX spans + 1, where the
    span grows to two tiles and the last span holds one element."""
    check_exact_shape((1, n, 1), dt, "spans", 7, ops=["add", "max"]
                      if dt != "i64" else ["add", "mul"])


@pytest.mark.parametrize("dt", DTYPES)
@pytest.mark.parametrize("shape", [
    (1, 3 * T + 5, 3),                  # 682 spans allowed per line, 4 used
    (1, 6 * T + 1, 300),                # 6 spans allowed: 2 tiles per span
    (1, T + 1, BLOCK_LINES - 1),        # 2 spans, the second of 1 element
])
def test_spans_several_lines(dja, shape, dt):
    check_exact_shape(shape, dt, "spans", 21)


# ------------------------------------------------ inner == 1, many lines
@pytest.mark.parametrize("dt", DTYPES)
@pytest.mark.parametrize("shape", [
    (1, 1, BLOCK_LINES), (1, 65, BLOCK_LINES + 1), (1, T + 1, BLOCK_LINES),
    (1, 3 * T + 5, BLOCK_LINES), (1, 1, 1), (1, T, BLOCK_LINES - 1),
    (1, 3, 16384 + 3),                  # more lines than workgroups
])
def test_block(dja, shape, dt):
    """One workgroup per line.  Odd line lengths start every second line
    8 (4) bytes off a 16-byte boundary: the scalar head."""
    check_exact_shape(shape, dt, "block", 33)


# ----------------------------------------------------------------- cols
@pytest.mark.parametrize("dt", DTYPES)
@pytest.mark.parametrize("outer", [1, 3])
def test_cols(dja, outer, dt):
    shapes = [(i, a, outer) for i in (2, 63, 64, 65, 257) for a in (1, 2, 65)]
    # the 32- and 4-deep load batches behind element 0: none, one 4-batch
    # exactly, + tail, one 32-batch exactly, + tail, + 4-batch, + both
    shapes += [(65, a, outer) for a in (4, 5, 6, 33, 34, 37, 38)]
    for s in shapes:
        check_exact_shape(s, dt, "cols", 50 + s[0] + s[1])


def test_cols_many_lines(dja):
    """The line -> (i, o) split with many workgroups, outer > 1 and an
    inner that is no multiple of the wave."""
    check_exact_shape((1000, 5, 7), "i64", "cols", 3, ops=["add"])


# ------------------------------------------------------------ alignment
@pytest.mark.parametrize("dt", ["f64", "f32", "i64"])
@pytest.mark.parametrize("n,fam", [(3 * T + 5, "spans"), (T, "block")])
def test_misaligned(dja, n, fam, dt):
    """src and dst equally off a 16-byte boundary (scalar head, then
    vectors) and differently off it (scalar rows)."""
    assert family(1, n, 1) == fam
    esz = kr.NP[dt].itemsize
    b = Bufs((1, n, 1), dt)
    try:
        x = exact_data("add", n, dt, 5)
        ref = exact_reference("add", x, (1, n, 1), None)
        same = [(k * esz, k * esz) for k in range(1, 16 // esz)]
        for so, do in same + [(esz, 0), (0, esz), (16 + esz, 16 - esz)]:
            got = b.scan("add", x, src_off=so, dst_off=do)
            assert_same("add", got, ref, (n, dt, so, do))
        got = b.scan("add", x, inplace=True, src_off=esz)
        assert_same("add", got, ref, (n, dt, "in place", esz))
    finally:
        b.free()


# --------------------------------------------------------------- bounded
BOUNDED = [((1, (1 << 20) + 1, 1), "spans"),
           ((1, 3 * T + 5, BLOCK_LINES + 1), "block"),
           ((65, 65, 3), "cols"), ((2, 5000, 2), "cols")]


@pytest.mark.parametrize("dt", ["f64", "f32"])
@pytest.mark.parametrize("shape,fam", BOUNDED)
def test_float_bounds(dja, shape, fam, dt):
    assert family(*shape) == fam
    inner, axis, outer = shape
    n, m = inner * axis * outer, inner * outer
    general, near_one = kr.dims_inputs(n, dt, 11)
    cg, c1 = kr.dims_inputs(m, dt, 12)
    u = np.longdouble(kr.UNIT[dt])
    b = Bufs(shape, dt)
    try:
        for carry in (None, cg):
            got = b.scan("add", general, carry=carry)
            w = general.astype(np.longdouble).reshape(shape, order="F")
            k0 = 0
            if carry is not None:
                cw = carry.astype(np.longdouble).reshape((inner, 1, outer),
                                                         order="F")
                ref = cw + np.cumsum(w, axis=1)
                mag = np.abs(cw) + np.cumsum(np.abs(w), axis=1)
                k0 = 1
            else:
                ref = np.cumsum(w, axis=1)
                mag = np.cumsum(np.abs(w), axis=1)
            k = (np.arange(axis, dtype=np.longdouble) + 1 + k0).reshape(
                (1, axis, 1))
            bound = k * u * mag
            err = np.abs(got.astype(np.longdouble).reshape(shape, order="F")
                         - ref)
            worst = float((err / np.maximum(bound, np.finfo(np.longdouble)
                                            .tiny)).max())
            print("add %s %s carry=%s worst err/bound %.3g"
                  % (shape, dt, carry is not None, worst))
            assert (err <= bound).all(), (shape, dt, "add", worst)
        for carry in (None, c1):
            got = b.scan("mul", near_one, carry=carry)
            w = near_one.astype(np.longdouble).reshape(shape, order="F")
            ref = np.cumprod(w, axis=1)
            k0 = 0
            if carry is not None:
                ref = carry.astype(np.longdouble).reshape(
                    (inner, 1, outer), order="F") * ref
                k0 = 1
            k = (np.arange(axis, dtype=np.longdouble) + 1 + k0).reshape(
                (1, axis, 1))
            rel = np.abs(got.astype(np.longdouble).reshape(shape, order="F")
                         - ref) / np.abs(ref)
            bound = k * u / (1 - k * u)
            worst = float((rel / bound).max())
            print("mul %s %s carry=%s worst rel/bound %.3g"
                  % (shape, dt, carry is not None, worst))
            assert (rel <= bound).all(), (shape, dt, "mul", worst)
    finally:
        b.free()


# ------------------------------------------------- NaN and element zero
NAN_SHAPES = [((1, 5 * T + 3, 2), "spans", (0, 2 * T + 100, 0)),
              ((1, 2 * T + 9, BLOCK_LINES + 1), "block", (0, T + 7, 5)),
              ((65, 20, 3), "cols", (7, 9, 1))]


@pytest.mark.parametrize("dt", ["f64", "f32"])
@pytest.mark.parametrize("shape,fam,site", NAN_SHAPES)
def test_nan_poisons_the_rest_of_its_line_only(dja, shape, fam, site, dt):
    assert family(*shape) == fam
    n = shape[0] * shape[1] * shape[2]
    b = Bufs(shape, dt)
    try:
        for op in ("add", "min", "max"):
            x = exact_data(op, n, dt, 9)
            clean = exact_reference(op, x, shape, None).reshape(shape,
                                                                order="F")
            v = x.reshape(shape, order="F").copy(order="F")
            v[site] = np.nan
            want = np.zeros(shape, dtype=bool, order="F")
            want[site[0], site[1]:, site[2]] = True
            got = b.scan(op, v.ravel(order="F")).reshape(shape, order="F")
            assert np.array_equal(np.isnan(got), want), (shape, dt, op)
            assert np.array_equal(got[~want], clean[~want]), (shape, dt, op)
    finally:
        b.free()


@pytest.mark.parametrize("dt", ["f64", "f32"])
@pytest.mark.parametrize("shape,fam", [((1, 3 * T + 5, 1), "spans"),
                                       ((1, 70, BLOCK_LINES), "block"),
                                       ((1, 1, 1), "block"),
                                       ((65, 3, 2), "cols")])
def test_element_zero_is_copied_bit_for_bit(dja, shape, fam, dt):
    """carry == NULL: -0.0 and a NaN with a payload come back unchanged as
    element 0 of their lines, under every op."""
    assert family(*shape) == fam
    n = shape[0] * shape[1] * shape[2]
    ut = {"f64": np.uint64, "f32": np.uint32}[dt]
    payload = {"f64": 0x7FF8000000ABCDEF, "f32": 0x7FC0ABCD}[dt]
    b = Bufs(shape, dt)
    try:
        for op in OPS:
            v = np.ones(shape, dtype=kr.NP[dt], order="F")
            v[:, 0, :] = -0.0
            last = (shape[0] - 1, 0, shape[2] - 1)
            if n > 1:
                vb = v.view(ut)
                vb[last] = payload
            got = b.scan(op, v.ravel(order="F")).reshape(shape, order="F")
            assert np.array_equal(kr.bits(got[:, 0, :]),
                                  kr.bits(v[:, 0, :])), (shape, dt, op)
            if n > 1:
                assert np.isnan(got[last[0], :, last[2]]).all()
    finally:
        b.free()


# ------------------------------------------- stale totals, ticket, misuse
@pytest.mark.parametrize("n", [(1 << 20) + 1, GMAX * T + 1])
def test_no_stale_span_totals(dja, n):
    """Two arrays whose span totals all differ, scanned alternately 16
    times each through the same totals buffer: a last arriver (or a second
    launch) that read the previous call's totals from a cache would carry
    the other array's prefixes."""
    from distributedarrays_jl_amd._ffi import lib, check
    assert family(1, n, 1) == "spans"
    xa = kr.philox.fill_int64(n, 41)
    xb = kr.philox.fill_int64(n, 42)
    with np.errstate(over="ignore"):
        ra, rb = np.cumsum(xa), np.cumsum(xb)
    A, B, D = kr.Dev.of(xa), kr.Dev.of(xb), kr.Dev(n * 8)
    try:
        for it in range(16):
            for src, ref in ((A, ra), (B, rb)):
                check(lib.da_scan(kr.REDOP["add"], D.p, src.p, 1, n, 1,
                                  kr.DT["i64"], None))
                got = D.get(np.int64, n)
                assert np.array_equal(got, ref), (n, it)
    finally:
        for d in (A, B, D):
            d.free()


def test_ticket_integrity(dja):
    """60 back-to-back calls: spans scans of changing n and dtype between
    flat reduces and counts.  The scan's first launch takes one ticket per
    block and the host advances the base by exactly its grid, or the next
    reduce's last arriver is misjudged and its result is wrong or stale."""
    from distributedarrays_jl_amd._ffi import lib, check
    sizes = [T + 1, 5 * T + 3, (1 << 18) + 1, 100 * T, 3 * T]
    data = {}
    for dt in DTYPES:
        for n in sizes:
            x = kr.small_ints(n, 60 + n % 7, 3).astype(kr.NP[dt])
            data[dt, n] = (x, kr.Dev.of(x), np.cumsum(x, dtype=kr.NP[dt]))
    out = kr.Dev(max(sizes) * 8)
    try:
        for call in range(60):
            dt = DTYPES[call % 3]
            n = sizes[(call * 7) % len(sizes)]
            x, buf, ref = data[dt, n]
            kind = call % 4
            if kind in (0, 2):
                assert family(1, n, 1) == "spans"
                check(lib.da_scan(kr.REDOP["add"], out.p, buf.p, 1, n, 1,
                                  kr.DT[dt], None))
                got = out.get(kr.NP[dt], n)
                assert np.array_equal(got, ref), (call, dt, n)
            elif kind == 1:
                r = CTYPE[dt]()
                check(lib.da_reduce(kr.MAPOP["identity"], kr.REDOP["add"],
                                    buf.p, n, kr.DT[dt], ctypes.byref(r)))
                assert r.value == x.sum(), (call, dt, n)
            else:
                c = ctypes.c_int64(-1)
                check(lib.da_count(kr.MAPOP["nonzero"], buf.p, n, kr.DT[dt],
                                   ctypes.byref(c)))
                assert c.value == np.count_nonzero(x), (call, dt, n)
    finally:
        out.free()
        for _, buf, _ in data.values():
            buf.free()


def test_rejected_calls_launch_nothing(dja):
    from distributedarrays_jl_amd._ffi import lib
    x = np.arange(8, dtype=np.float64)
    S, D = kr.Dev.of(x), kr.Dev.of(np.zeros(8))
    try:
        assert lib.da_scan(0, S.at(8), S.p, 1, 4, 1, 0, None) < 0
        assert b"overlaps src" in lib.da_errstr(0)
        assert lib.da_scan(0, D.p, S.p, 1, 4, 1, 0, D.at(16)) < 0
        assert b"overlaps carry" in lib.da_errstr(0)
        assert lib.da_scan(7, D.p, S.p, 1, 4, 1, 0, None) < 0
        assert lib.da_scan(0, D.p, S.p, 1, 4, 1, 9, None) < 0
        assert lib.da_scan(0, None, S.p, 1, 4, 1, 0, None) < 0
        assert lib.da_scan(0, None, None, 1, 0, 1, 0, None) == 0   # empty
        assert lib.da_scan(0, None, None, 0, 5, 3, 0, None) == 0
        assert np.array_equal(S.get(np.float64, 8), x)
        assert np.array_equal(D.get(np.float64, 8), np.zeros(8))
    finally:
        S.free()
        D.free()


# ------------------------------------------------------------ Python API
def _ints(shape, dt, seed, bound):
    n = int(np.prod(shape))
    return np.asfortranarray(kr.small_ints(n, seed, bound).astype(kr.NP[dt])
                             .reshape(shape, order="F"))


@pytest.mark.parametrize("dt", DTYPES)
def test_python_api_world1(dja, dt):
    start = dja.bytes_in_use()
    wrap = {"add": dja.dcumsum, "mul": dja.dcumprod, "max": dja.dcummax,
            "min": dja.dcummin}
    cases = [((5000,), (None, 0)), ((70, 33), (0, 1)), ((9, 300, 5), (1,)),
             ((3, 4, 1000), (2,))]
    for shape, dimlist in cases:
        g = _ints(shape, dt, 17, 3)
        # products: +-1 and +-2 / +-0.5 at a few sites stay exact
        p = np.where(_ints(shape, dt, 18, 40) == 0, 2, 1) * \
            np.where(_ints(shape, dt, 19, 1) < 0, -1, 1)
        p = np.asfortranarray(p.astype(kr.NP[dt]))
        D, P = dja.distribute(g), dja.distribute(p)
        for dims in dimlist:
            ax = 0 if dims is None else dims
            for op in OPS:
                h, H = (p, P) if op == "mul" else (g, D)
                R = wrap[op](H) if dims is None else wrap[op](H, dims)
                with np.errstate(over="ignore"):
                    ref = UF[op].accumulate(h, axis=ax)
                assert R.dims == H.dims and R.dtype == dt
                assert np.array_equal(R.collect(), ref), (shape, dims, op)
                R.close()
            # init
            R = dja.daccumulate("add", D, dims, init=-5)
            assert np.array_equal(R.collect(),
                                  np.cumsum(g, axis=ax) + kr.NP[dt].type(-5))
            R.close()
            R = dja.daccumulate("max", D, dims, init=1)
            assert np.array_equal(
                R.collect(), np.maximum(np.maximum.accumulate(g, axis=ax),
                                        kr.NP[dt].type(1)))
            R.close()
            # accumulate! in place and into another array
            C = D.copy()
            assert dja.daccumulate_("add", C, C, dims) is C
            assert np.array_equal(C.collect(), np.cumsum(g, axis=ax))
            E = D.similar()
            dja.daccumulate_("min", E, C, dims, init=0)
            assert np.array_equal(
                E.collect(), np.minimum(np.minimum.accumulate(
                    np.cumsum(g, axis=ax), axis=ax), kr.NP[dt].type(0)))
            C.close()
            E.close()
        D.close()
        P.close()
    M = dja.distribute(_ints((4, 4), dt, 1, 3))
    with pytest.raises(dja.DArrayError):
        dja.dcumsum(M)
    with pytest.raises(dja.DArrayError):
        dja.daccumulate("add", M, 2)
    M.close()
    assert dja.bytes_in_use() == start
