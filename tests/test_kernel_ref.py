"""CPU validation of tests/kernel_ref.py — the references and bounds the
kernel-level GPU tests rely on are checked here against the oracle
(oracle.ops.oracle_reduce_dims), math.fsum and exact integer arithmetic,
so a wrong reference cannot hide behind a GPU-only test."""
import math
from fractions import Fraction

import numpy as np
import pytest

import kernel_ref as kr
from oracle import ops as oops

SHAPES = [(1, 1, 1), (5, 7, 3), (64, 3, 9), (3, 65, 4), (33, 1, 2),
          (1, 257, 2)]


def _oracle(f, op, x, inner, axis, outer):
    cube = np.asfortranarray(x.reshape((inner, axis, outer), order="F"))
    idxs = [[(0, inner), (0, axis), (0, outer)]]
    with np.errstate(over="ignore"):
        r = oops.oracle_reduce_dims(f, op, [cube], idxs,
                                    (inner, axis, outer), (1,))
    return np.asfortranarray(r).ravel(order="F")


@pytest.mark.parametrize("dt", ["f64", "f32", "i64"])
@pytest.mark.parametrize("shape", SHAPES)
def test_dims_reference_agrees_with_oracle(shape, dt):
    inner, axis, outer = shape
    xs, xm = kr.dims_inputs(inner * axis * outer, dt, 5)
    for op in ("add", "mul", "min", "max"):
        x = xm if op == "mul" else xs
        for f in ("identity", "abs", "abs2", "nonzero"):
            with np.errstate(over="ignore"):
                ref, bound = kr.dims_reference(f, op, x, inner, axis, outer)
            got = _oracle(f, op, x, inner, axis, outer)
            assert (bound is None) == (dt == "i64" or op in ("min", "max"))
            # numpy's pairwise fold is one valid evaluation order, so it
            # must sit inside the any-order bound around the reference
            assert kr.dims_mismatch(got, ref, bound) is None, (op, f)


@pytest.mark.parametrize("dt", ["f64", "f32"])
def test_dims_reference_sum_is_fsum(dt):
    inner, axis, outer = 3, 41, 2
    x, _ = kr.dims_inputs(inner * axis * outer, dt, 6)
    ref, bound = kr.dims_reference("identity", "add", x, inner, axis, outer)
    cube = x.reshape((inner, axis, outer), order="F")
    for o in range(outer):
        for i in range(inner):
            col = [float(v) for v in cube[i, :, o]]
            exact = math.fsum(col)
            j = i + o * inner
            assert abs(float(ref[j]) - exact) <= 2.0 ** -60 * abs(exact)
            want = (axis - 1) * kr.UNIT[dt] * math.fsum(abs(v) for v in col)
            assert abs(float(bound[j]) - want) <= 1e-12 * want


def test_dims_reference_product_is_exact_rational():
    inner, axis, outer = 2, 9, 2
    _, x = kr.dims_inputs(inner * axis * outer, "f64", 7)
    ref, bound = kr.dims_reference("identity", "mul", x, inner, axis, outer)
    cube = x.reshape((inner, axis, outer), order="F")
    for o in range(outer):
        for i in range(inner):
            exact = Fraction(1)
            for v in cube[i, :, o]:
                exact *= Fraction(float(v))
            j = i + o * inner
            assert abs(Fraction(float(ref[j])) - exact) <= \
                Fraction(1, 2 ** 52) * abs(exact)
            assert float(bound[j]) == pytest.approx(
                8 * 2.0 ** -53 * abs(float(ref[j])), rel=1e-12)


def test_dims_reference_axis_zero_is_identity():
    for dt in ("f64", "f32", "i64"):
        x = np.zeros(0, dtype=kr.NP[dt])
        for op, want in (("add", 0), ("mul", 1)):
            ref, bound = kr.dims_reference("identity", op, x, 5, 0, 3)
            assert bound is None and ref.shape == (15,)
            assert ref.dtype == kr.NP[dt] and (ref == want).all()
    ref, _ = kr.dims_reference("identity", "min", np.zeros(0), 5, 0, 3)
    assert np.isposinf(ref).all()
    ref, _ = kr.dims_reference("identity", "max", np.zeros(0, np.int64),
                               5, 0, 3)
    assert (ref == kr.I64_MIN).all()


def test_dims_mismatch_rejects_what_it_should():
    x, _ = kr.dims_inputs(5 * 7 * 3, "f64", 8)
    ref, bound = kr.dims_reference("identity", "add", x, 5, 7, 3)
    good = ref.astype(np.float64)
    assert kr.dims_mismatch(good, ref, bound) is None
    bad = good.copy()
    bad[4] += 4 * float(bound[4]) + 1e-300
    assert "first at 4" in kr.dims_mismatch(bad, ref, bound)
    bad = good.copy()
    bad[2] = np.nan
    assert kr.dims_mismatch(bad, ref, bound) is not None
    ref, bound = kr.dims_reference("identity", "max", x, 5, 7, 3)
    assert kr.dims_mismatch(ref.copy(), ref, None) is None
    bad = ref.copy()
    bad[0] = np.nextafter(bad[0], 2.0)
    assert kr.dims_mismatch(bad, ref, None) is not None
    z = np.zeros(3)
    assert kr.dims_mismatch(-z, z, None) is not None   # -0.0 is not +0.0


def test_gemm_references():
    A, B = kr.gemm_int_inputs(7, 5, 6, "f32", 3)
    assert A.dtype == np.float32 and A.flags.f_contiguous
    assert np.abs(A).max() <= 4 and np.abs(B).max() <= 4
    assert (A == np.rint(A)).all() and len(np.unique(A)) > 3
    C = kr.small_ints(35, 9, 4).reshape((7, 5), order="F")
    ref = kr.gemm_int_reference(A, B, C, 3, -2)
    want = [[3 * sum(int(A[i, l]) * int(B[l, j]) for l in range(6))
             - 2 * int(C[i, j]) for j in range(5)] for i in range(7)]
    assert ref.dtype == np.int64 and ref.tolist() == want
    nanC = np.full((7, 5), np.nan)
    assert kr.gemm_int_reference(A, B, nanC, 1, 0).tolist() == \
        (A.astype(np.int64) @ B.astype(np.int64)).tolist()
    Ar = np.asfortranarray(kr.uniform(42, "f64", 4).reshape(7, 6) - 0.5)
    Br = np.asfortranarray(kr.uniform(30, "f64", 5).reshape(6, 5) - 0.5)
    ref, bound = kr.gemm_real_reference(Ar, Br, "f64")
    got = Ar @ Br
    assert (np.abs(got - ref) <= bound).all()
    assert float(bound[0, 0]) == pytest.approx(
        6 * 2.0 ** -53 * float(np.abs(Ar[0]) @ np.abs(Br[:, 0])), rel=1e-12)


def test_fold_identities_and_small_ints():
    assert kr.fold_identity("min", "i64") == kr.I64_MAX
    assert kr.fold_identity("max", "f32") == -np.inf
    v = kr.small_ints(4096, 1, 8)
    assert v.dtype == np.int64 and v.min() == -8 and v.max() == 8
