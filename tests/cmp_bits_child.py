"""Comparison numerics of the expression language on the GPU, shared by
tests/test_gpu_compact.py (which calls lines() in its own process, where the
hipRTC JIT runs the programs) and its child process (this file as a script,
started with DA_EXPR_JIT=0 so the interpreters run them).  lines() checks
every result of one group of cases against numpy's own comparison operators
and returns one text line of bits per case; the parent asserts that the two
texts are equal.

    DA_EXPR_JIT=0 python tests/cmp_bits_child.py
"""
import os
import sys
import zlib

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))

OPS = {"eq": np.equal, "ne": np.not_equal, "lt": np.less,
       "le": np.less_equal, "gt": np.greater, "ge": np.greater_equal}
NPDT = {"f64": np.float64, "f32": np.float32, "i64": np.int64}
N = 2 * 2048 + 3          # odd, more than one block of every kernel


def float_data(dt, kr):
    """(a, b): NaN, +-inf, +-0.0, a denormal, equal neighbours — every
    planted value meets every other one, and itself — then philox noise
    rounded to a few values so that equal pairs keep occurring."""
    t = NPDT[dt]
    tiny = np.finfo(t).smallest_subnormal
    vals = np.array([np.nan, np.inf, -np.inf, 0.0, -0.0, tiny, -tiny, 1.0,
                     1.0, -1.0, 0.5], dtype=t)
    a = np.repeat(vals, vals.size)
    b = np.tile(vals, vals.size)
    pad = N - a.size
    ra = np.round(kr.uniform(pad, dt, 71) * 4).astype(t) / t(4)
    rb = np.round(kr.uniform(pad, dt, 72) * 4).astype(t) / t(4)
    return np.concatenate([a, ra]), np.concatenate([b, rb])


def int_data(kr):
    """(a, b): every pair of INT64_MIN, INT64_MAX, -1, 0, 1 (their
    differences wrap), then small philox integers."""
    lo, hi = np.iinfo(np.int64).min, np.iinfo(np.int64).max
    vals = np.array([lo, hi, -1, 0, 1, lo + 1, hi - 1], dtype=np.int64)
    a = np.repeat(vals, vals.size)
    b = np.tile(vals, vals.size)
    pad = N - a.size
    return (np.concatenate([a, kr.small_ints(pad, 73, 3)]),
            np.concatenate([b, kr.small_ints(pad, 74, 3)]))


def _bits(x):
    x = np.ascontiguousarray(x)
    return x.view(np.uint64 if x.dtype.itemsize == 8 else np.uint32)


def _one(dja, E, tag, tree, expect, dt):
    """materialize, count and reduce("add") of one tree against numpy."""
    expect = np.asfortranarray(expect.astype(NPDT[dt]))
    G = E.materialize(tree)
    got = G.collect()
    G.close()
    assert got.dtype == expect.dtype and got.shape == expect.shape, tag
    bad = np.flatnonzero(_bits(got).ravel() != _bits(expect).ravel())
    assert bad.size == 0, "%s: %d wrong, first at %d" % (tag, bad.size,
                                                         bad[0])
    k = E.count(tree)
    assert k == int(np.count_nonzero(expect)), (tag, k)
    s = E.reduce("add", tree)
    assert s == k, (tag, s, k)        # a sum of k ones, k < 2^24: exact
    return "%s %08x %d %r" % (tag, zlib.crc32(_bits(got).tobytes()), k,
                              float(s))


PARTS = {"f64": ("arr", "const", "strided"),
         "f32": ("arr", "const", "strided"), "i64": ("arr", "const")}


def lines(dja, dt, part):
    """The cases of one dtype and part, all six ops each: "arr" an array
    against an array (and the Python operators), "const" an array against
    constants, "strided" (floats) an (m, n) array against a (1, n) row."""
    sys.path.insert(0, _HERE)
    import kernel_ref as kr
    from distributedarrays_jl_amd import expr as E
    out = []
    if part == "strided":
        m, n = 67, 5
        x = np.asfortranarray(
            (np.round(kr.uniform(m * n, dt, 75) * 4) / 4)
            .astype(NPDT[dt]).reshape((m, n), order="F"))
        x[3, 1] = np.nan
        x[5, 2] = -0.0
        row = np.asfortranarray(x[7:8, :].copy())
        row[0, 4] = np.nan
        X, R = dja.distribute(x), dja.distribute(row)
        for name, f in OPS.items():
            with np.errstate(invalid="ignore"):
                out.append(_one(dja, E, "%s %s strided" % (dt, name),
                                getattr(E, name)(E.ref(X), E.ref(R)),
                                f(x, row), dt))
        X.close()
        R.close()
        return out
    a, b = int_data(kr) if dt == "i64" else float_data(dt, kr)
    A, B = dja.distribute(a), dja.distribute(b)
    consts = (0, 1, -(1 << 53)) if dt == "i64" else (1.0, 0.0)
    with np.errstate(invalid="ignore"):
        for name, f in OPS.items():
            op = getattr(E, name)
            if part == "arr":
                out.append(_one(dja, E, "%s %s arr" % (dt, name),
                                op(E.ref(A), E.ref(B)), f(a, b), dt))
                continue
            for c in consts:
                out.append(_one(dja, E, "%s %s %r" % (dt, name, c),
                                op(E.ref(A), c), f(a, NPDT[dt](c)), dt))
        # the Python operators build the same trees
        if part == "arr":
            out.append(_one(dja, E, "%s operator >" % dt,
                            E.ref(A) > E.ref(B), a > b, dt))
        else:
            out.append(_one(dja, E, "%s operator <=" % dt,
                            E.ref(A) <= consts[0],
                            a <= NPDT[dt](consts[0]), dt))
    A.close()
    B.close()
    return out


def main():
    sys.path.insert(0, os.path.dirname(_HERE))
    import distributedarrays_jl_amd as dja
    from distributedarrays_jl_amd._ffi import lib
    dja.comm.init()
    for dt, parts in PARTS.items():
        for part in parts:
            for ln in lines(dja, dt, part):
                print("%s %s|%s" % (dt, part, ln))
    assert lib.da_expr_jit_state() != 2, "the JIT ran with DA_EXPR_JIT=0"
    dja.d_closeall()
    assert dja.bytes_in_use() == 0
    print("cmp done")
    return 0


if __name__ == "__main__":
    sys.exit(main())
