"""Every kernel family behind da_reduce_dims, at the smallest shapes that
reach it, against the any-order references of tests/kernel_ref.py.

da_reduce_dims is called directly with an explicit (inner, axis, outer)
view.  Each shape carries the variant it is meant to reach and the test
asserts dbg_reduce_dims_variant agrees BEFORE launching — the launcher
calls the same selector, so a later threshold change fails here instead of
silently moving a shape to another kernel.

Exact cases (min/max everywhere, i64 add/mul mod 2^64) compare bits.
Float add must meet |got - ref| <= (axis-1)*u*sum|x_i| per output and
float mul |got - ref| <= (axis-1)*u*|ref|: the worst case of any
summation order, so no constant here depends on the kernels.

The slices variant's second kernel grid-strides only past 2048*256
outputs, and the dispatcher sends any shape with 262144 or more outputs
elsewhere, so that loop's second trip is unreachable by construction; the
threads, waves and blocks stride loops each run with more outputs than
their grid covers ((1025,2,2049), (3,64,11000), (33,7,300)).
"""
import ctypes

import numpy as np
import pytest

import kernel_ref as kr

pytestmark = pytest.mark.gpu

# (intended variant, (inner, axis, outer))
SHAPES = [
    ("threads", (64, 3, 4096)),     # smallest entry: 262144 outputs
    ("threads", (4099, 5, 64)),     # inner not a multiple of the block
    ("threads", (1025, 2, 2049)),   # 2100225 outputs > 8192*256: grid-stride
    ("threads", (512, 1, 512)),     # axis = 1
    ("waves", (1, 64, 16384)),      # smallest entry
    ("waves", (63, 65, 261)),       # axis not a multiple of 64
    ("waves", (5, 129, 3300)),      # three lane strides, the last partial
    ("waves", (3, 64, 11000)),      # 33000 outputs > 32768 waves: wave-stride
    ("blocks", (1, 1, 1)),          # smallest entry
    ("blocks", (1, 255, 7)),        # axis just under a block
    ("blocks", (1, 257, 7)),        # axis just over a block
    ("blocks", (33, 7, 300)),       # 9900 outputs > 8192 blocks: LDS reuse
    ("blocks", (100, 3, 100)),      # inner >= 64 but axis < 64
    ("slices", (64, 64, 1)),        # smallest entry
    ("slices", (257, 67, 3)),       # partial row tile, uneven a0/a1 split
    ("slices", (1000, 200, 5)),     # larger case
]
REDOPS = ("add", "mul", "min", "max")
# identity/abs2 have constant-folded instantiations; abs/nonzero ride the
# runtime-switch fallback
MAPOPS = ("identity", "abs2", "abs", "nonzero")
DTYPES = ("f64", "f32", "i64")


@pytest.fixture(scope="module")
def lib():
    import distributedarrays_jl_amd as dja
    from distributedarrays_jl_amd import _ffi
    dja.comm.init()
    return _ffi.lib


def variant_of(lib, shape):
    from distributedarrays_jl_amd import _ffi
    return _ffi.DIMS_VARIANTS[lib.dbg_reduce_dims_variant(*shape)]


def reduce_dims(lib, f, op, src, shape, dt, dst):
    from distributedarrays_jl_amd._ffi import check
    inner, axis, outer = shape
    check(lib.da_reduce_dims(kr.MAPOP[f], kr.REDOP[op], src.p, inner, axis,
                             outer, kr.DT[dt], dst.p))
    check(lib.da_synchronize())


def test_three_shapes_per_variant():
    for v in ("threads", "waves", "blocks", "slices"):
        assert sum(1 for w, _ in SHAPES if w == v) >= 3, v


@pytest.mark.parametrize("dt", DTYPES)
@pytest.mark.parametrize("variant,shape", SHAPES,
                         ids=["%s-%dx%dx%d" % ((v,) + s) for v, s in SHAPES])
def test_dims_variant_all_ops(lib, variant, shape, dt):
    assert variant_of(lib, shape) == variant, \
        "dispatcher no longer sends %r to %s" % (shape, variant)
    inner, axis, outer = shape
    nout = inner * outer
    xs, xm = kr.dims_inputs(inner * axis * outer, dt, 101)
    ds = kr.Dev.of(xs)
    dm = ds if xm is xs else kr.Dev.of(xm)
    dst = kr.Dev(nout * kr.NP[dt].itemsize)
    failures = []
    try:
        for op in REDOPS:
            x, dx = (xm, dm) if op == "mul" else (xs, ds)
            for f in MAPOPS:
                with np.errstate(over="ignore"):
                    ref, bound = kr.dims_reference(f, op, x, inner, axis,
                                                   outer)
                reduce_dims(lib, f, op, dx, shape, dt, dst)
                got = dst.get(kr.NP[dt], nout)
                if bound is not None:
                    err = np.abs(got.astype(np.longdouble) - ref)
                    print("%s %s/%s: max err %.3e, max bound %.3e" % (
                        dt, op, f, float(err.max()), float(bound.max())))
                bad = kr.dims_mismatch(got, ref, bound)
                if bad:
                    failures.append("%s/%s: %s" % (op, f, bad))
    finally:
        dst.free()
        if dm is not ds:
            dm.free()
        ds.free()
    assert not failures, "\n".join(failures)


# one shape per variant whose LAST stride over the axis holds the NaN:
# (shape, axis position of the NaN)
NAN_CASES = [
    ("threads", (64, 3, 4096), 2),      # last serial step
    ("waves", (5, 129, 3300), 128),     # third lane stride (lane 0 only)
    ("blocks", (1, 257, 7), 256),       # second block stride (thread 0 only)
    ("slices", (257, 67, 3), 66),       # last column of the last slice
]


@pytest.mark.parametrize("dt", ["f64", "f32"])
@pytest.mark.parametrize("variant,shape,apos", NAN_CASES,
                         ids=[c[0] for c in NAN_CASES])
def test_dims_variant_nan_propagation(lib, variant, shape, apos, dt):
    """One NaN in exactly one slice: min and max of that output are NaN,
    every other output is bit-identical to the NaN-free run."""
    assert variant_of(lib, shape) == variant
    inner, axis, outer = shape
    nout = inner * outer
    x, _ = kr.dims_inputs(inner * axis * outer, dt, 202)
    i0, o0 = inner - 1, outer // 2
    xn = x.copy()
    xn[i0 + apos * inner + o0 * inner * axis] = np.nan
    hit = i0 + o0 * inner
    dx, dn = kr.Dev.of(x), kr.Dev.of(xn)
    dst = kr.Dev(nout * kr.NP[dt].itemsize)
    try:
        for op in ("min", "max"):
            reduce_dims(lib, "identity", op, dx, shape, dt, dst)
            clean = dst.get(kr.NP[dt], nout)
            ref, _ = kr.dims_reference("identity", op, x, inner, axis, outer)
            assert kr.dims_mismatch(clean, ref, None) is None
            reduce_dims(lib, "identity", op, dn, shape, dt, dst)
            got = dst.get(kr.NP[dt], nout)
            assert np.isnan(got[hit]), (op, got[hit])
            same = kr.bits(got) == kr.bits(clean)
            same[hit] = True
            assert same.all(), (op, np.flatnonzero(~same)[:5])
    finally:
        dst.free(); dn.free(); dx.free()


@pytest.mark.parametrize("dt", DTYPES)
def test_axis_zero_gives_fold_identity(lib, dt):
    shape = (5, 0, 3)
    src = kr.Dev(16)
    dst = kr.Dev(15 * kr.NP[dt].itemsize)
    try:
        for op in REDOPS:
            for f in ("identity", "abs"):
                dst.put(np.full(15, 77, dtype=kr.NP[dt]))
                reduce_dims(lib, f, op, src, shape, dt, dst)
                got = dst.get(kr.NP[dt], 15)
                want = np.full(15, kr.fold_identity(op, dt), dtype=kr.NP[dt])
                assert kr.dims_mismatch(got, want, None) is None, (op, f)
    finally:
        dst.free(); src.free()


@pytest.mark.parametrize("shape", [(0, 5, 3), (4, 5, 0), (0, 0, 0)])
def test_no_outputs_leaves_dst_untouched(lib, shape):
    for dt in DTYPES:
        sentinel = np.full(8, -12345, dtype=kr.NP[dt])
        src = kr.Dev.of(np.ones(64, dtype=kr.NP[dt]))
        dst = kr.Dev.of(sentinel)
        try:
            rc = lib.da_reduce_dims(kr.MAPOP["identity"], kr.REDOP["add"],
                                    src.p, shape[0], shape[1], shape[2],
                                    kr.DT[dt], dst.p)
            assert rc == 0
            lib.da_synchronize()
            assert np.array_equal(kr.bits(dst.get(kr.NP[dt], 8)),
                                  kr.bits(sentinel))
        finally:
            dst.free(); src.free()


# ---- Python-level surface ------------------------------------------------
@pytest.mark.parametrize("shape,axes", [
    ((96, 40), (0,)), ((96, 40), (1,)), ((17, 9, 11), (1,)),
    ((17, 9, 11), (0, 2)),
])
def test_dprod_and_dminimum_dims(lib, shape, axes):
    import distributedarrays_jl_amd as dja
    n = int(np.prod(shape))
    xs, xm = kr.dims_inputs(n, "f64", 303)
    xs = np.asfortranarray(xs.reshape(shape, order="F"))
    xm = np.asfortranarray(xm.reshape(shape, order="F"))
    d = dja.distribute(xs)
    M = dja.dminimum_dims(d, axes)
    ref = xs.min(axis=axes, keepdims=True)
    assert M.dims == ref.shape
    assert np.array_equal(M.collect(), ref)
    M.close(); d.close()
    d = dja.distribute(xm)
    P = dja.dprod_dims(d, axes)
    nred = int(np.prod([shape[a] for a in axes]))
    ref = xm.astype(np.longdouble).prod(axis=axes, keepdims=True)
    got = P.collect()
    assert got.shape == ref.shape
    # any-order product bound over all nred factors of each output
    assert (np.abs(got - ref) <= (nred - 1) * kr.UNIT["f64"]
            * np.abs(ref)).all()
    P.close(); d.close()
    with np.errstate(over="ignore"):
        xi = np.asfortranarray(kr.philox.fill_int64(n, 304)
                               .reshape(shape, order="F"))
        d = dja.distribute(xi)
        P = dja.dprod_dims(d, axes)
        assert np.array_equal(P.collect(), xi.prod(axis=axes, keepdims=True))
        M = dja.dminimum_dims(d, axes)
        assert np.array_equal(M.collect(), xi.min(axis=axes, keepdims=True))
        M.close(); P.close(); d.close()


def test_multi_axis_map_applied_once(lib):
    """dreduce_dims("abs2", "add", d, (0, 2)): f on the first pass only —
    applying it again on the second pass would give sum((sum x^2)^2)."""
    import distributedarrays_jl_amd as dja
    shape = (64, 32, 16)
    x, _ = kr.dims_inputs(64 * 32 * 16, "f64", 305)
    x = np.asfortranarray(x.reshape(shape, order="F"))
    d = dja.distribute(x)
    R = dja.dreduce_dims("abs2", "add", d, (0, 2))
    sq = (x * x).astype(np.longdouble)
    ref = sq.sum(axis=(0, 2), keepdims=True)
    got = R.collect()
    assert got.shape == (1, 32, 1)
    # 64*16 terms per output; the terms are the rounded squares, all >= 0
    assert (np.abs(got - ref) <= (64 * 16 - 1) * kr.UNIT["f64"] * ref).all()
    R.close()
    # exact on integers: any second application of f would change the bits
    xi = np.asfortranarray(kr.small_ints(64 * 32 * 16, 306, 8)
                           .reshape(shape, order="F"))
    di = dja.distribute(xi)
    Ri = dja.dreduce_dims("abs2", "add", di, (0, 2))
    assert np.array_equal(Ri.collect(),
                          (xi * xi).sum(axis=(0, 2), keepdims=True))
    Ri.close(); di.close(); d.close()
