"""Child process of tests/test_gpu_expr_reduce.py: prints the hex bits of a
fixed, philox-seeded list of fused expression reductions, one per line,
under whatever DA_* switches the parent put in the environment (they are
read once per process).  The single-launch path and the two-kernel path
(DA_RED_FUSED=0) must print the same text.

    python tests/expr_reduce_bits_child.py
"""
import os
import sys

_HERE = os.path.dirname(os.path.abspath(__file__))

SIZES = (257, (1 << 20) + 1)


def main():
    sys.path.insert(0, os.path.dirname(_HERE))
    sys.path.insert(0, _HERE)
    import numpy as np
    import distributedarrays_jl_amd as dja
    from distributedarrays_jl_amd import expr as E
    import kernel_ref as kr
    dja.comm.init()

    def show(tag, v, dt):
        got = np.array([v], dtype=kr.NP[dt])
        print("%s %x" % (tag, int(kr.bits(got)[0])))

    for n in SIZES:
        for dt in ("f64", "f32"):
            half = kr.NP[dt].type(0.5)
            x = dja.distribute(kr.uniform(n, dt, 910 + kr.DT[dt]) - half)
            y = dja.distribute(kr.uniform(n, dt, 920 + kr.DT[dt]) - half)
            show("%s %d dot" % (dt, n),
                 E.reduce("add", E.ref(x) * E.ref(y)), dt)
            show("%s %d sin max" % (dt, n),
                 E.reduce("max", E.sin(E.ref(x)) + E.ref(y) * 0.5), dt)
            show("%s %d count" % (dt, n),
                 E.count(E.sign(E.max2(E.ref(x), 0.0))), "i64")
            x.close()
            y.close()
        xi = dja.distribute(kr.small_ints(n, 930, 8))
        show("i64 %d add" % n, E.reduce("add", abs(E.ref(xi)) * 3 + 1), "i64")
        xi.close()
    X = dja.distribute(np.asfortranarray(
        (kr.uniform(33 * 7, "f64", 940) - 0.5).reshape((33, 7), order="F")))
    M = dja.dmean_dims(X, (0,))
    e = E.abs2(E.ref(X) - E.ref(M))
    show("strided add", E.reduce("add", e), "f64")
    show("strided min", E.reduce("min", e), "f64")
    show("strided count", E.count(e), "i64")
    show("var", dja.dvar(X), "f64")
    dja.d_closeall()
    assert dja.bytes_in_use() == 0
    print("bits done")
    return 0


if __name__ == "__main__":
    sys.exit(main())
