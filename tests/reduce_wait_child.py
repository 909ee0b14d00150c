"""The call sequence of tests/test_gpu_reduce_wait.py, importable (sequence,
waits) and runnable as a child process under whatever DA_* switches the
parent put in the environment (DA_RED_SPIN_US is read once per process).

    python tests/reduce_wait_child.py ROUNDS N [N ...]

prints one "tag got want" line per scalar result, then
"waits <polled> <synced> <calls>" for the calls of this run, then
"wait done".

Per size n, `rounds` rounds.  Round i reduces one of two i64 arrays whose
sums differ (golden sequence a, and 3a+1), alternating, through da_reduce
(reduce_fused), and interleaves one further call that publishes into the
same pinned slot, in turn:
  i % 4 == 0  an f32 sum (4 bytes into a slot that last held 8),
  i % 4 == 1  da_count (count_fused),
  i % 4 == 2  expr.reduce through the hipRTC-generated kernel,
  i % 4 == 3  expr.reduce through the interpreter kernel (DA_EXPR_JIT=0 is
              read per call).
Every expected value is an exact integer: i64 sums wrap, the f32 data are
integers in [-8, 8], at most 2^20 of them (the f32 array is cut there), so
every partial sum in any order is an integer of magnitude <= 2^23."""
import os
import sys

_HERE = os.path.dirname(os.path.abspath(__file__))


def waits():
    """(polled, synced) since da_init."""
    import ctypes
    from distributedarrays_jl_amd._ffi import lib, check
    polled, synced = ctypes.c_uint64(), ctypes.c_uint64()
    check(lib.da_dbg_reduce_waits(ctypes.byref(polled), ctypes.byref(synced)))
    return int(polled.value), int(synced.value)


def sequence(dja, n, rounds):
    """[(tag, got, want)] of 2 * rounds scalar results at size n."""
    import numpy as np
    import kernel_checks as kc
    import kernel_ref as kr
    from distributedarrays_jl_amd import expr as E
    a = kc.golden_sequence(n)
    with np.errstate(over="ignore"):
        b = a * np.int64(3) + np.int64(1)
        host = (a, b)
        sums = [int(x.sum(dtype=np.int64)) for x in host]
        twice = [int((x + x).sum(dtype=np.int64)) for x in host]
    assert sums[0] != sums[1]
    f = kr.small_ints(min(n, 1 << 20), 90 + n % 7, 8).astype(np.float32)
    ds = [dja.distribute(x) for x in host]
    fd = dja.distribute(f)
    out = []
    try:
        for i in range(rounds):
            k = i & 1
            out.append(("n%d r%d sum%d" % (n, i, k), dja.dsum(ds[k]),
                        sums[k]))
            tag = "n%d r%d " % (n, i)
            if i % 4 == 0:
                out.append((tag + "f32", int(dja.dsum(fd)),
                            int(f.sum(dtype=np.int64))))
            elif i % 4 == 1:
                out.append((tag + "count", dja.dcount("nonzero", ds[k]),
                            int(np.count_nonzero(host[k]))))
            elif i % 4 == 2:
                out.append((tag + "jit", E.reduce(
                    "add", E.ref(ds[k]) + E.ref(ds[k])), twice[k]))
            else:
                os.environ["DA_EXPR_JIT"] = "0"
                try:
                    got = E.reduce("max", E.ref(ds[k]))
                finally:
                    del os.environ["DA_EXPR_JIT"]
                out.append((tag + "interp", got, int(host[k].max())))
    finally:
        fd.close()
        for d in ds:
            d.close()
    return out


def main():
    sys.path.insert(0, os.path.dirname(_HERE))
    sys.path.insert(0, _HERE)
    import distributedarrays_jl_amd as dja
    dja.comm.init()
    rounds = int(sys.argv[1])
    p0, s0 = waits()
    calls = 0
    for n in [int(v) for v in sys.argv[2:]]:
        for tag, got, want in sequence(dja, n, rounds):
            print("%s %d %d" % (tag, got, want))
            calls += 1
    p1, s1 = waits()
    print("waits %d %d %d" % (p1 - p0, s1 - s0, calls))
    dja.d_closeall()
    print("wait done")
    return 0


if __name__ == "__main__":
    sys.exit(main())
