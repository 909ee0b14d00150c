"""TEST-ONLY reference for the fused dims-reductions: the terms of a
broadcast program from oracle.expr.evaluate (grown by the comparison
opcodes, which it predates) and the per-output checks of a fold along axes.
Shared by the fakelib and the GPU suites."""
import math

import numpy as np

import oracle.expr as oexpr

CMP = {64: np.equal, 65: np.not_equal, 66: np.less, 67: np.less_equal,
       68: np.greater, 69: np.greater_equal}          # enum da_cmpop
UNIT = {np.dtype("float64"): 2.0 ** -53, np.dtype("float32"): 2.0 ** -24}


def evaluate(prog, args, consts, dt):
    """oracle.expr.evaluate instruction by instruction; a comparison is
    1 / 0 in the tree's dtype (IEEE: false against a NaN, except ne)."""
    dt = np.dtype(dt)
    stack = []
    for ins in prog:
        kind, idx = ins >> 8, ins & 0xFF
        if kind == 1:
            stack.append(args[idx])
        elif kind == 2:
            stack.append(dt.type(consts[idx]))
        elif kind == 3 and idx in CMP:
            b = stack.pop()
            a = stack.pop()
            stack.append(CMP[idx](a, b).astype(dt))
        else:
            n = 1 if kind == 0 else 2
            operands = [np.asarray(v, dtype=dt) for v in stack[-n:]]
            del stack[-n:]
            sub = [(1 << 8) | k for k in range(n)] + [ins]
            stack.append(oexpr.evaluate(sub, operands, [], dt))
    assert len(stack) == 1
    return np.asarray(stack[0], dtype=dt)


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint64 if a.dtype.itemsize == 8 else np.uint32)


def same_bits(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and \
        np.array_equal(bits(a), bits(b))


def check_fold(got, t, axes, op, tag, integral=False):
    """got: the device's result (reduced axes of size 1); t: the terms, full
    shape.  min, max, i64 folds and counts (op None): exact bits, a NaN
    term giving NaN for its own output only.  Float add: |got - fsum(t)| <=
    1.01 (N-1) u sum|t| per output, N the terms folded into it (any
    summation order obeys it).  Float mul: |got/exact - 1| <= 1.01 N u.
    integral: the terms are integers small enough that every partial sum
    is exact, so numpy's sum IS fsum (for outputs too many to fsum one by
    one)."""
    axes = tuple(axes)
    dt = t.dtype
    N = int(np.prod([t.shape[a] for a in axes])) if axes else 1
    kshape = tuple(1 if a in axes else t.shape[a] for a in range(t.ndim))
    assert got.shape == kshape, (tag, got.shape, kshape)
    if op is None:
        want = np.count_nonzero(t, axis=axes, keepdims=True).astype(np.int64)
        assert got.dtype == np.int64 and np.array_equal(got, want), tag
        return
    assert got.dtype == dt, (tag, got.dtype)
    if dt.kind == "i":
        f = {"add": np.add, "mul": np.multiply, "min": np.minimum,
             "max": np.maximum}[op]
        with np.errstate(over="ignore"):
            want = f.reduce(t, axis=axes, keepdims=True)
        assert np.array_equal(got, want), (tag, op)
        return
    if op in ("min", "max"):
        want = (np.min if op == "min" else np.max)(t, axis=axes,
                                                   keepdims=True)
        nan = np.isnan(want)
        assert np.array_equal(np.isnan(got), nan), (tag, op)
        assert np.array_equal(bits(got)[~nan], bits(want)[~nan]), (tag, op)
        return
    u = UNIT[dt]
    # terms of output o as row o: bring the reduced axes last
    keep = [a for a in range(t.ndim) if a not in axes]
    rows = np.transpose(t, keep + list(axes)).reshape(-1, N)
    flat = np.transpose(got, keep + list(axes)).reshape(-1)
    if op == "add":
        if integral:
            exact = rows.astype(np.float64).sum(axis=1)
            mag = np.abs(rows.astype(np.float64)).sum(axis=1)
            assert mag.max(initial=0.0) < 1.0 / u      # partial sums exact
            err = np.abs(flat.astype(np.float64) - exact)
            worst = float((err - 1.01 * (N - 1) * u * mag).max(initial=-1))
            print("%s add (integral) worst err-bound %.3e" % (tag, worst))
            assert worst <= 0, (tag, worst)
            return
        assert rows.shape[0] * N <= 1 << 17, "fsum: too many terms"
        for o in range(rows.shape[0]):
            tl = [float(v) for v in rows[o]]
            err = abs(float(flat[o]) - math.fsum(tl))
            bound = 1.01 * (N - 1) * u * math.fsum(abs(v) for v in tl)
            assert err <= bound, (tag, o, float(flat[o]), err, bound)
        return
    exact = np.prod(rows.astype(np.longdouble), axis=1)
    rel = np.abs(flat.astype(np.longdouble) / exact - 1)
    print("%s mul worst rel %.3e bound %.3e" % (tag, float(rel.max()),
                                                1.01 * N * u))
    assert (rel <= 1.01 * N * u).all(), (tag, float(rel.max()))
