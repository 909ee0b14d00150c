"""Child process of tests/test_gpu_reduce_single_launch.py: prints the hex
bits of a fixed, philox-seeded list of flat reductions, one per line, under
whatever DA_* switches the parent put in the environment (they are read
once per process).  The single-launch path and the two-kernel path
(DA_RED_FUSED=0) must print the same text.

    python tests/reduce_bits_child.py
"""
import os
import sys

_HERE = os.path.dirname(os.path.abspath(__file__))

SIZES = (257, (1 << 20) + 1, (1 << 22) + 1)
DTYPES = ("f64", "f32")
OPS = (("identity", "add"), ("identity", "max"), ("abs2", "add"))


def main():
    sys.path.insert(0, os.path.dirname(_HERE))
    sys.path.insert(0, _HERE)
    import numpy as np
    import distributedarrays_jl_amd as dja
    import kernel_ref as kr
    dja.comm.init()
    for dt in DTYPES:
        for n in SIZES:
            x = kr.uniform(n, dt, 900 + kr.DT[dt]) - kr.NP[dt].type(0.5)
            d = dja.distribute(x)
            for f, op in OPS:
                got = np.array([dja.mapreduce(f, op, d)], dtype=kr.NP[dt])
                print("%s %d %s %s %x" % (dt, n, f, op, int(kr.bits(got)[0])))
            d.close()
    dja.d_closeall()
    print("bits done")
    return 0


if __name__ == "__main__":
    sys.exit(main())
