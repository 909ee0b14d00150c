"""Shared pieces of the kernel-level GPU tests (test_gpu_dims_variants,
test_gpu_reduce_tree, test_gpu_gemm_exact and variant_child): plain
high-precision references with worst-case error bounds, deterministic
inputs, and a raw device buffer over the C ABI.

Nothing here is tuned against a kernel's output.  The float bounds are the
textbook worst cases for ANY evaluation order (Higham, Accuracy and
Stability of Numerical Algorithms, 2nd ed., section 4.2 for sums, 3.1 for
products and dot products), with u the unit roundoff of the format:

  sum of n terms      |got - exact| <= (n-1) * u * sum|x_i|
  product of n terms  |got - exact| <= (n-1) * u * |exact|
  dot product, k      |got - exact| <= k * u * (|a| . |b|)

The reference side is numpy longdouble (64-bit significand on x86-64), whose
own error is 2^-11 of the f64 bound and is ignored.  test_kernel_ref.py
checks this module on the CPU against oracle.ops and math.fsum.
"""
import ctypes

import numpy as np

from oracle import philox

NP = {"f64": np.dtype("float64"), "f32": np.dtype("float32"),
      "i64": np.dtype("int64")}
DT = {"f64": 0, "f32": 1, "i64": 2}                       # enum da_dtype
REDOP = {"add": 0, "mul": 1, "min": 2, "max": 3}          # enum da_redop
MAPOP = {"identity": 0, "abs": 1, "abs2": 2, "isnan": 3,  # enum da_redf
         "isfinite": 4, "nonzero": 5}
UNIT = {"f64": 2.0 ** -53, "f32": 2.0 ** -24}             # unit roundoff
I64_MAX = np.iinfo(np.int64).max
I64_MIN = np.iinfo(np.int64).min


def dtype_name(x):
    return {v: k for k, v in NP.items()}[np.dtype(x.dtype)]


def fold_identity(op, dt):
    """Identity element of each redop (what an empty fold returns)."""
    if op == "add":
        return NP[dt].type(0)
    if op == "mul":
        return NP[dt].type(1)
    if dt == "i64":
        return np.int64(I64_MAX if op == "min" else I64_MIN)
    return NP[dt].type(np.inf if op == "min" else -np.inf)


# ------------------------------------------------------------------ inputs
def uniform(n, dt, seed):
    """philox uniform [0,1) for floats; small values in [-8, 8] for i64."""
    if dt == "f64":
        return philox.fill_uniform_f64(n, seed)
    if dt == "f32":
        return philox.fill_uniform_f32(n, seed)
    return small_ints(n, seed, 8)


def small_ints(n, seed, bound):
    """philox i64 reduced into [-bound, bound]."""
    if n == 0:
        return np.zeros(0, dtype=np.int64)
    return np.mod(philox.fill_int64(n, seed), 2 * bound + 1) - bound


def dims_inputs(n, dt, seed):
    """(general, near_one): data for add/min/max and data for mul.  Floats:
    one philox draw u -> u-0.5 (both signs, so abs matters) and
    0.98+0.04u (products stay near 1).  i64: raw philox bits for both —
    add and mul wrap mod 2^64 on either side."""
    if dt == "i64":
        x = philox.fill_int64(n, seed)
        return x, x
    u = uniform(n, dt, seed)
    t = NP[dt].type
    return u - t(0.5), u * t(0.04) + t(0.98)


# --------------------------------------------------- dims-reduce reference
def map_values(f, x):
    """The kernel's map function, evaluated in x's own dtype (one rounding
    for abs2 on floats; wrapping on i64)."""
    if f == "identity":
        return x
    if f == "abs":
        return np.abs(x)          # abs(INT64_MIN) wraps to itself, as on device
    if f == "abs2":
        return x * x
    if f == "nonzero":
        return (x != 0).astype(x.dtype)
    raise ValueError(f)


def dims_reference(f, op, x, inner, axis, outer):
    """Reference of da_reduce_dims(f, op) on x viewed column-major as
    (inner, axis, outer), reduced over the middle axis.

    Returns (ref, bound), both flat in the kernel's output order
    (i + o*inner).  bound is None where the result must be bit-exact
    (min/max on every dtype, everything on i64): ref then has x's dtype.
    For float add/mul ref and bound are longdouble."""
    dt = dtype_name(x)
    v = map_values(f, x).reshape((inner, axis, outer), order="F")
    if axis == 0:
        ref = np.full((inner, outer), fold_identity(op, dt), dtype=NP[dt])
        return ref.ravel(order="F"), None
    if op in ("min", "max"):
        r = v.min(axis=1) if op == "min" else v.max(axis=1)
        return r.ravel(order="F"), None
    if dt == "i64":
        r = v.sum(axis=1, dtype=np.int64) if op == "add" \
            else v.prod(axis=1, dtype=np.int64)
        return r.ravel(order="F"), None
    w = v.astype(np.longdouble)
    nu = np.longdouble(axis - 1) * np.longdouble(UNIT[dt])
    if op == "add":
        ref = w.sum(axis=1)
        bound = nu * np.abs(w).sum(axis=1)
    else:
        ref = w.prod(axis=1)
        bound = nu * np.abs(ref)
    return ref.ravel(order="F"), bound.ravel(order="F")


def bits(a):
    """Integer view for bit-for-bit comparison of any supported dtype."""
    a = np.ascontiguousarray(a)
    return a.view({8: np.uint64, 4: np.uint32}[a.dtype.itemsize])


def dims_mismatch(got, ref, bound):
    """None when `got` meets the reference, else a short description with
    the worst figure.  Exact cases compare bits; bounded cases compare
    |got - ref| <= bound elementwise in longdouble."""
    if bound is None:
        if got.dtype != ref.dtype:
            return "dtype %s != %s" % (got.dtype, ref.dtype)
        bad = np.flatnonzero(bits(got) != bits(ref))
        if bad.size == 0:
            return None
        j = int(bad[0])
        return "%d/%d outputs differ, first at %d: got %r ref %r" % (
            bad.size, got.size, j, got[j], ref[j])
    err = np.abs(got.astype(np.longdouble) - ref)
    ok = err <= bound          # NaN/inf in got compare False
    if ok.all():
        return None
    j = int(np.flatnonzero(~ok)[0])
    return "%d/%d outputs over the bound, first at %d: got %r ref %r " \
           "err %.3e bound %.3e" % ((~ok).sum(), got.size, j, got[j],
                                    float(ref[j]), float(err[j]),
                                    float(bound[j]))


# ----------------------------------------------------------- gemm reference
def gemm_int_inputs(m, n, k, dt, seed):
    """Integer-valued A (m x k), B (k x n) in [-4, 4], Fortran order, cast
    to dt: every product and partial sum is exact in f64 and in f32
    (|sum| <= 16k << 2^24), so any accumulation order gives the same bits."""
    A = small_ints(m * k, seed, 4).reshape((m, k), order="F")
    B = small_ints(k * n, seed + 1, 4).reshape((k, n), order="F")
    return (np.asfortranarray(A.astype(NP[dt])),
            np.asfortranarray(B.astype(NP[dt])))


def gemm_int_reference(A, B, C, alpha, beta):
    """alpha*A*B + beta*C in int64 (BLAS beta == 0: C is not read)."""
    P = int(alpha) * (A.astype(np.int64) @ B.astype(np.int64))
    if beta == 0:
        return P
    return P + int(beta) * C.astype(np.int64)


def gemm_real_reference(A, B, dt):
    """(ref, bound) for C = A*B with real inputs: the matmul one precision
    up (longdouble for f64, f64 for f32) and the dot-product bound
    k*u*(|A|.|B|), elementwise."""
    k = A.shape[1]
    hi = np.longdouble if dt == "f64" else np.float64
    Al, Bl = A.astype(hi), B.astype(hi)
    ref = Al @ Bl
    bound = hi(k) * hi(UNIT[dt]) * (np.abs(Al) @ np.abs(Bl))
    return ref, bound


# ------------------------------------------------------------ device buffer
class Dev:
    """Raw device buffer through da_alloc/da_h2d/da_d2h (no DArray layer),
    so a test controls pointers, offsets and leading dimensions itself."""

    def __init__(self, nbytes):
        from distributedarrays_jl_amd._ffi import lib, check
        self._lib, self._check = lib, check
        self.nbytes = int(nbytes)
        self.p = ctypes.c_void_p()
        check(lib.da_alloc(max(self.nbytes, 1), 0, ctypes.byref(self.p)))

    @classmethod
    def of(cls, arr):
        arr = np.asarray(arr)
        buf = cls(arr.nbytes)
        buf.put(arr)
        return buf

    def at(self, byte_off=0):
        return ctypes.c_void_p(self.p.value + int(byte_off))

    def put(self, arr):
        a = np.ravel(np.asarray(arr), order="K")
        a = np.ascontiguousarray(a)
        assert a.nbytes <= self.nbytes
        if a.nbytes:
            self._check(self._lib.da_h2d(self.p, a.ctypes.data, a.nbytes))

    def get(self, dtype, count):
        out = np.empty(int(count), dtype=dtype)
        assert out.nbytes <= self.nbytes
        if out.nbytes:
            self._check(self._lib.da_d2h(self.p, out.ctypes.data,
                                         out.nbytes))
        return out

    def free(self):
        if self.p.value:
            self._check(self._lib.da_free(self.p))
            self.p = ctypes.c_void_p()
