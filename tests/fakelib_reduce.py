"""TEST-ONLY: fakelib.FakeLib grown by the fused expression reductions
(da_expr_reduce / da_expr_count), restated as oracle.expr.evaluate +
numpy.  Same purpose and same rules as fakelib.py: only tests install
it, explicitly; numerics are numpy's, the tests built on it check
orchestration (domain, localisation, empty chunks, the cross-rank fold).
`calls` records every ABI entry the reductions go through, so a test can
see which one a Python path took."""
import ctypes

import numpy as np

import fakelib
from fakelib import _NPDT, _REDOP_NAMES, _addr, _tv


class FakeLibReduce(fakelib.FakeLib):
    def __init__(self):
        super().__init__()
        self.calls = []

    def da_reduce(self, *a):
        self.calls.append("da_reduce")
        return super().da_reduce(*a)

    def da_count(self, *a):
        self.calls.append("da_count")
        return super().da_count(*a)

    def _terms(self, prog, plen, dims, nd, srcs, src_strides, nsrcs,
               consts, nconsts, n, dtype):
        import oracle.expr as oexpr
        dt = _NPDT[int(dtype)]
        plen, nd, n = int(plen), int(nd), int(n)
        nsrcs, nconsts = int(nsrcs), int(nconsts)
        if n == 0:
            return np.zeros(0, dtype=dt)
        pv = ctypes.cast(prog, ctypes.POINTER(ctypes.c_int32))
        program = [int(pv[i]) for i in range(plen)]
        cv = ctypes.cast(consts, ctypes.POINTER(ctypes.c_double))
        cc = [float(cv[i]) for i in range(nconsts)]
        sv = ctypes.cast(srcs, ctypes.POINTER(ctypes.c_void_p))
        if _addr(src_strides) == 0:
            args = [_tv(sv[i], n, dt) for i in range(nsrcs)]
        else:
            dv = ctypes.cast(dims, ctypes.POINTER(ctypes.c_uint64))
            shape = tuple(int(dv[d]) for d in range(nd))
            assert int(np.prod(shape)) == n, (shape, n)
            stv = ctypes.cast(src_strides, ctypes.POINTER(ctypes.c_uint64))
            args = []
            for i in range(nsrcs):
                ss = [int(stv[i * nd + d]) for d in range(nd)]
                args.append(np.lib.stride_tricks.as_strided(
                    _tv(sv[i], 1, dt), shape=shape,
                    strides=tuple(s * dt.itemsize for s in ss)))
        out = oexpr.evaluate(program, args, cc, dt)
        return np.broadcast_to(out, out.shape if out.size == n
                               else (n,)).ravel(order="F")

    def da_expr_reduce(self, prog, plen, dims, nd, srcs, src_strides, nsrcs,
                       consts, nconsts, n, dtype, redop, out):
        self.calls.append("da_expr_reduce")
        dt = _NPDT[int(dtype)]
        t = self._terms(prog, plen, dims, nd, srcs, src_strides, nsrcs,
                        consts, nconsts, n, dtype)
        op = _REDOP_NAMES[int(redop)]
        if t.size == 0:
            if op in ("add", "mul"):
                val = dt.type(0 if op == "add" else 1)
            elif dt.kind == "i":
                info = np.iinfo(np.int64)
                val = info.max if op == "min" else info.min
            else:
                val = np.inf if op == "min" else -np.inf
        else:
            with np.errstate(over="ignore"):
                val = {"add": lambda: t.sum(dtype=dt),
                       "mul": lambda: t.prod(dtype=dt),
                       "min": t.min, "max": t.max}[op]()
        ct = {0: ctypes.c_double, 1: ctypes.c_float, 2: ctypes.c_int64}[
            int(dtype)]
        ctypes.cast(out, ctypes.POINTER(ct))[0] = \
            int(val) if int(dtype) == 2 else float(val)
        return 0

    def da_expr_count(self, prog, plen, dims, nd, srcs, src_strides, nsrcs,
                      consts, nconsts, n, dtype, out):
        self.calls.append("da_expr_count")
        t = self._terms(prog, plen, dims, nd, srcs, src_strides, nsrcs,
                        consts, nconsts, n, dtype)
        ctypes.cast(out, ctypes.POINTER(ctypes.c_int64))[0] = \
            int(np.count_nonzero(t))
        return 0


def install():
    """fakelib.install() with the grown fake."""
    from distributedarrays_jl_amd import _ffi, ops, darray, spmd, expr
    fake = FakeLibReduce()
    _ffi.lib = fake
    for mod in (ops, darray, spmd, expr):
        mod.lib = fake
    return fake
