"""Local GEMM pinned exactly.  Inputs are integers in [-4, 4], so every
product and partial sum is exact in f64 and in f32 (|sum| <= 16k << 2^24)
and the int64 numpy matmul is the reference for ANY accumulation order:
all comparisons are array_equal.  Shapes cover a single k-tile (the
prefetch pipeline never enters its kt+1 arms), workgroup counts that are
no multiple of 8 (XCD-swizzle remainder), 1xN and Nx1 grids, deep k, each
side of the MFMA/naive dispatch boundary, padded leading dimensions,
sub-matrix pointers, and the BLAS alpha/beta special cases.  Each shape
asserts dbg_gemm_path first — the launcher calls the same selector."""
import numpy as np
import pytest

import kernel_checks as kc
import kernel_ref as kr

pytestmark = pytest.mark.gpu

MFMA_SHAPES = [
    (128, 128, 16),     # single k-tile, one workgroup
    (128, 128, 32),
    (384, 384, 48),     # 9 workgroups
    (640, 896, 16),     # 35 workgroups, single k-tile
    (640, 896, 32),     # 35 workgroups, two k-tiles
    (128, 1152, 32),    # grid 1x9
    (1152, 128, 32),    # grid 9x1
    (256, 128, 1024),   # deep k
]
NAIVE_SHAPES = [
    (129, 128, 16), (128, 127, 16), (128, 128, 17),   # one past each tile
    (1, 7, 3), (1, 150, 200), (200, 1, 150),
]
FLOATS = ("f64", "f32")
ids3 = lambda s: "%dx%dx%d" % s


@pytest.fixture(scope="module")
def lib():
    import distributedarrays_jl_amd as dja
    from distributedarrays_jl_amd import _ffi
    dja.comm.init()
    return _ffi.lib


@pytest.mark.parametrize("dt", FLOATS)
@pytest.mark.parametrize("shape", MFMA_SHAPES, ids=ids3)
def test_mfma_shapes_exact(lib, shape, dt):
    assert kc.gemm_path(lib, *shape) == "mfma"
    kc.gemm_exact(lib, dt, *shape)


@pytest.mark.parametrize("dt", FLOATS)
@pytest.mark.parametrize("shape", MFMA_SHAPES, ids=ids3)
def test_mfma_shapes_real_inputs_in_bound(lib, shape, dt):
    assert kc.gemm_path(lib, *shape) == "mfma"
    kc.gemm_real_in_bound(lib, dt, *shape)


TILE_SHAPES = [(128, 128, 16), (384, 384, 48), (640, 896, 32)]


def test_mfma_plain_padded_beta0(lib):
    """One, 9 and 35 workgroups through the tile kernel, both float dtypes:
    plain, padded with accumulation, and beta = 0 over a NaN C (C is never
    read).  One test, not a parametrised one: it is the check set that the
    former DA_GEMM_V=3 variant child ran, now in the default process."""
    for shape in TILE_SHAPES:
        m, n, k = shape
        assert kc.gemm_path(lib, *shape) == "mfma"
        for dt in FLOATS:
            kc.gemm_exact(lib, dt, m, n, k)
            kc.gemm_exact(lib, dt, m, n, k, alpha=1, beta=-2,
                          layout=kc.padded())
            kc.gemm_exact(lib, dt, m, n, k, beta=0,
                          c_block=kc.nan_block(m, n, dt))
        kc.gemm_real_in_bound(lib, "f64", m, n, k)


@pytest.mark.parametrize("dt", FLOATS)
@pytest.mark.parametrize("shape", NAIVE_SHAPES, ids=ids3)
def test_dispatch_boundary_naive_exact(lib, shape, dt):
    assert kc.gemm_path(lib, *shape) == "naive"
    kc.gemm_exact(lib, dt, *shape)
    kc.gemm_exact(lib, dt, *shape, alpha=2, beta=-1)


def test_i64_gemm_wrap_exact(lib):
    kc.gemm_exact(lib, "i64", 60, 50, 40, alpha=3, beta=-2)
    # full-range operands: products and sums wrap mod 2^64 on both sides
    m, n, k = 60, 50, 40
    with np.errstate(over="ignore"):
        A = kr.philox.fill_int64(m * k, 5).reshape((m, k), order="F")
        B = kr.philox.fill_int64(k * n, 6).reshape((k, n), order="F")
        C = kr.philox.fill_int64(m * n, 7).reshape((m, n), order="F")
        want = 3 * (A @ B) - 2 * C
    pa, pb, pc = kc.Panel(A), kc.Panel(B), kc.Panel(C)
    try:
        from distributedarrays_jl_amd._ffi import check
        check(lib.da_gemm_i64(pc.ptr(), pa.ptr(), pb.ptr(), m, n, k,
                              m, k, m, 3, -2))
        check(lib.da_synchronize())
        assert np.array_equal(pc.fetch(), want)
    finally:
        pc.free(); pb.free(); pa.free()


PANEL_SHAPES = [(128, 128, 16), (384, 384, 48), (129, 128, 16), (1, 7, 3)]


@pytest.mark.parametrize("dt", FLOATS)
@pytest.mark.parametrize("shape", PANEL_SHAPES, ids=ids3)
def test_padded_panels(lib, shape, dt):
    """lda = m+16, ldb = k+16, ldc = m+16; NaN under A and B must not leak
    in, the sentinel rows under C must keep their bits."""
    kc.gemm_exact(lib, dt, *shape, layout=kc.padded())
    kc.gemm_exact(lib, dt, *shape, alpha=1, beta=1, layout=kc.padded())


# sub-matrix views keep every leading dimension and offset 16-element
# aligned (the MFMA kernels use 16-byte vector loads; see darray_hip.h)
SUB_SHAPES = [(128, 128, 16), (384, 384, 48), (128, 127, 16), (16, 7, 32)]


@pytest.mark.parametrize("dt", FLOATS)
@pytest.mark.parametrize("shape", SUB_SHAPES, ids=ids3)
def test_submatrix_operands(lib, shape, dt):
    """A, B and C point inside NaN-bordered parents (128-byte-multiple
    offsets, 16-element-aligned leading dimensions); borders untouched."""
    lay = kc.submatrix(dt)
    b = lay["A"]["top"]
    for rows in (shape[0], shape[2]):      # rows of A and C, rows of B
        ld = rows + 2 * b
        assert ld % 16 == 0
        assert ((b * ld + b) * kr.NP[dt].itemsize) % 128 == 0
    kc.gemm_exact(lib, dt, *shape, layout=lay)
    kc.gemm_exact(lib, dt, *shape, alpha=-1, beta=2, layout=lay)


BOTH_PATHS = [(384, 384, 48), (129, 128, 16)]


@pytest.mark.parametrize("dt", FLOATS)
@pytest.mark.parametrize("shape", BOTH_PATHS, ids=["mfma", "naive"])
def test_alpha_beta_semantics(lib, shape, dt):
    m, n, k = shape
    assert kc.gemm_path(lib, *shape) == ("mfma" if m % 128 == 0 else "naive")
    # beta = 0 never reads C: a NaN-filled C gives a NaN-free exact result
    kc.gemm_exact(lib, dt, m, n, k, beta=0, c_block=kc.nan_block(m, n, dt))
    kc.gemm_exact(lib, dt, m, n, k, beta=0, c_block=kc.nan_block(m, n, dt),
                  layout=kc.padded())
    # exact accumulation
    kc.gemm_exact(lib, dt, m, n, k, alpha=1, beta=1)
    kc.gemm_exact(lib, dt, m, n, k, alpha=1, beta=-2)
    kc.gemm_exact(lib, dt, m, n, k, alpha=-3, beta=-2)
    # alpha = 0 never reads A or B: NaN in A, result exactly beta*C
    kc.gemm_exact(lib, dt, m, n, k, alpha=0, beta=-2,
                  a_block=kc.nan_block(m, k, dt))
    kc.gemm_exact(lib, dt, m, n, k, alpha=0, beta=0,
                  a_block=kc.nan_block(m, k, dt),
                  c_block=kc.nan_block(m, n, dt))
    # k = 0: beta*C; with beta = 0 over a NaN C: zeros
    kc.gemm_exact(lib, dt, m, n, 0, alpha=1, beta=-2, layout=kc.padded())
    kc.gemm_exact(lib, dt, m, n, 0, alpha=1, beta=0,
                  c_block=kc.nan_block(m, n, dt))


@pytest.mark.parametrize("dt", FLOATS + ("i64",))
def test_empty_output_leaves_c_untouched(lib, dt):
    lay = {"C": dict(bottom=16, right=2, border=-777)}
    kc.gemm_exact(lib, dt, 0, 5, 16, beta=0, layout=lay)
    kc.gemm_exact(lib, dt, 5, 0, 16, beta=0, layout=lay)
    kc.gemm_exact(lib, dt, 0, 0, 0, beta=3, layout=lay)
