"""Child process of tests/test_gpu_math_ulp.py: every route to the functor
table on one hard vector, bytes compared.  Imports the package BEFORE
anything that could load torch, so hipRTC compiles with the ROCm
code-object manager the library was built against.

    python tests/route_bits_child.py REPORT.json

REPORT.json: {"unary": {"op|dtype": null or a description}, "binary": {...},
"jit_state": int, "jit_err": str, "comgr": [paths in load order]}.
Exit status 0 when every route ran, whatever the comparisons gave; 3 on a
device error (nothing more is launched).
"""
import json
import os
import sys

_HERE = os.path.dirname(os.path.abspath(__file__))

UNARY = ["neg", "abs", "abs2", "inv", "sqrt", "floor", "ceil", "round",
         "trunc", "sign", "isnan", "isinf", "isfinite",
         "cbrt", "exp", "exp2", "exp10", "expm1", "log", "log2", "log10",
         "log1p", "sin", "cos", "tan", "asin", "acos", "atan", "sinh", "cosh",
         "tanh", "asinh", "acosh", "atanh", "sinpi", "cospi", "deg2rad",
         "rad2deg", "sec", "csc", "cot", "erf", "erfc", "erfinv", "erfcinv",
         "erfcx", "gamma", "lgamma", "sinc", "cosc", "sind", "cosd", "tand",
         "asind", "acosd", "atand", "acot", "acotd", "asec", "acsc", "asech",
         "acsch", "acoth"]
BINARY = ["add", "sub", "mul", "div", "min2", "max2", "rem", "mod", "pow",
          "atan2"]


def route_vector(U, np, dt):
    """specials (subnormals included: a route that flushes them shows up),
    the doubles closest to multiples of pi/2, a signed whole-range sweep."""
    body = U.sweep("atan", dt, n=2000)
    if dt == "f64":
        deep = U.pio2_hard("deep")
        body = np.concatenate([deep[:512], deep[-512:], body])
    return U.with_specials(body.astype(U.NP[dt]), U.specials(dt))


def main(argv):
    if len(argv) != 2:
        print(__doc__, file=sys.stderr)
        return 2
    sys.path.insert(0, os.path.dirname(_HERE))
    sys.path.insert(0, _HERE)
    import distributedarrays_jl_amd as dja          # first: pins ROCm's libs
    from distributedarrays_jl_amd import expr as E
    from distributedarrays_jl_amd._ffi import lib, DArrayError
    import numpy as np
    import kernel_ref as kr
    import ulp_ref as U
    dja.comm.init()

    def mk(arr):
        d = dja.DArray(arr.shape, kr.dtype_name(arr))
        d.set_localpart(np.asfortranarray(arr))
        return d

    def interp(f):
        os.environ["DA_EXPR_JIT"] = "0"             # read per call
        try:
            return f()
        finally:
            del os.environ["DA_EXPR_JIT"]

    def compare(m, e, inputs):
        want = kr.bits(m.localpart()).copy()
        jit = E.materialize(e)
        itp = interp(lambda: E.materialize(e))
        msg = None
        for name, arr in (("hipRTC", jit), ("interpreter", itp)):
            bad = np.flatnonzero(kr.bits(arr.localpart()) != want)
            if bad.size and msg is None:
                j = int(bad[0])
                msg = "%s: %d of %d differ, first at %r: %r vs da_map %r" % (
                    name, bad.size, want.size,
                    [float(v[j]) for v in inputs],
                    float(arr.localpart()[j]), float(m.localpart()[j]))
        jit.close(); itp.close()
        return msg

    report = {"unary": {}, "binary": {}}
    try:
        for dt in ("f64", "f32"):
            x = route_vector(U, np, dt)
            d = mk(x)
            for op in UNARY:
                m = dja.dmap(op, d)
                e = getattr(E, op)(E.ref(d))
                msg = compare(m, e, [x])
                if msg is None and op in ("sin", "cos", "exp"):
                    keep = np.isfinite(m.localpart())
                    ds = mk(x[keep])
                    ms = dja.dmap(op, ds)
                    es = getattr(E, op)(E.ref(ds))
                    top = dja.dmaximum(ms)
                    got = (float(ms.localpart().max()), E.reduce("max", es),
                           interp(lambda: E.reduce("max", es)))
                    if any(g != top for g in got):
                        msg = "max-reduce: %r vs dmaximum %r" % (got, top)
                    ms.close(); ds.close()
                m.close()
                report["unary"]["%s|%s" % (op, dt)] = msg
            d.close()
            a, b = U.grid2(dt)
            da_, db = mk(a), mk(b)
            for op in BINARY:
                m = dja.elementwise(op, da_, db)
                e = E.Binary(op, E.ref(da_), E.ref(db))
                report["binary"]["%s|%s" % (op, dt)] = compare(m, e, [a, b])
                m.close()
            da_.close(); db.close()
    except DArrayError as err:
        print("device error, stopping: %r" % (err,), file=sys.stderr)
        return 3
    report["jit_state"] = int(lib.da_expr_jit_state())
    report["jit_err"] = repr(lib.da_expr_jit_errstr())
    report["comgr"] = [l.split()[-1] for l in open("/proc/self/maps")
                       if "libamd_comgr" in l and "r-xp" in l]
    dja.d_closeall()
    with open(argv[1], "w") as f:
        json.dump(report, f)
    bad = {k: v for part in ("unary", "binary")
           for k, v in report[part].items() if v}
    print("routes: %d compared, %d differ" % (
        len(report["unary"]) + len(report["binary"]), len(bad)))
    for k, v in bad.items():
        print("  %s: %s" % (k, v))
    return 0


if __name__ == "__main__":
    sys.exit(main(sys.argv))
