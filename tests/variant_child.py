"""Child process of tests/test_gpu_variants.py (and tools/variant_check.py):
runs one named check set on the GPU under whatever DA_* switches the
parent put in the environment.  The kernel-variant switches are read once
per process, so every variant gets a fresh interpreter; the parent starts
the children strictly one at a time and stops at the first one that dies.

    python tests/variant_child.py {reduce|small}

VARIANTS is the single table of env-gated variants and the set each runs.
"""
import os
import sys

_HERE = os.path.dirname(os.path.abspath(__file__))

# (environment, check set)
VARIANTS = [
    ({"DA_RED_FUSED": "1"}, "reduce"),
    ({"DA_RV4": "1"}, "reduce"),
    ({"DA_RBLOCKS": "1"}, "reduce"),
    ({"DA_RBLOCKS": "7"}, "reduce"),
    ({"DA_RBLOCKS": "8192"}, "reduce"),
    ({"DA_NT": "1"}, "small"),
    ({"DA_MM_OVERLAP": "0"}, "small"),
    ({"DA_EXPR_JIT": "0"}, "small"),
    ({"DA_MAP_W": "2"}, "small"),
    ({"DA_BC_W": "2"}, "small"),
]


def variant_id(env):
    return ",".join("%s=%s" % kv for kv in sorted(env.items()))


def run_reduce(dja, lib):
    import kernel_checks as kc
    for n in (1, 257, kc.TREE_N):
        for dt in ("f64", "f32", "i64"):
            kc.check_planted_extrema(dja, dt, n)
            if dt != "i64":
                kc.check_planted_nan(dja, dt, n)
        kc.check_once_only(dja, n)
    kc.check_once_only(dja, (1 << 22) + 1)   # more pairs than 8192 blocks hold
    # changing n (hence grid size) and interleaved dtypes in ONE process:
    # with DA_RED_FUSED=1 a ticket that did not return to 0 makes the next
    # launch miss its last arriver, and the stale result fails the check
    seed = 500
    for n in (1, 257, 100001, 2, kc.TREE_N, 513, 70000, 3, 1 << 21, 255):
        for dt in ("f64", "i64", "f32"):
            seed += 1
            kc.check_sum_in_bound(dja, dt, n, seed)


def run_small(dja, lib):
    """The small end-to-end check shared with tools/variant_check.py."""
    import numpy as np
    import kernel_ref as kr
    from oracle import philox
    from distributedarrays_jl_amd import expr as E
    m = 256
    A = np.asfortranarray(philox.fill_uniform_f64(m * m, 1)
                          .reshape(m, m, order="F"))
    B = np.asfortranarray(philox.fill_uniform_f64(m * m, 2)
                          .reshape(m, m, order="F"))
    dA, dB = dja.distribute(A), dja.distribute(B)
    C = dja.dmatmul(dA, dB)
    ref, bound = kr.gemm_real_reference(A, B, "f64")
    assert (np.abs(C.localpart() - ref) <= bound).all()
    x = philox.fill_uniform_f64(100001, 3)
    d = dja.distribute(x)
    w = x.astype(np.longdouble)
    assert abs(np.longdouble(dja.dsum(d)) - w.sum()) <= \
        (x.size - 1) * np.longdouble(kr.UNIT["f64"]) * np.abs(w).sum()
    o = E.materialize(E.ref(d) * 2.0 + 1.0)
    assert np.array_equal(o.localpart(), x * 2.0 + 1.0)
    s = dja.dmap("abs2", d)
    assert np.array_equal(s.localpart(), x * x)
    import kernel_checks as kc
    kc.check_map_ulp(dja)
    # every elementwise launcher at its edges: under DA_NT=1, DA_MAP_W=2
    # and DA_BC_W=2 these are the vector-of-2 and non-temporal kernels
    kc.check_elementwise_edges(dja, kc.EDGE_SIZES, kc.EDGE_WRAP)
    for h in (o, s, d, C, dA, dB):
        h.close()


SETS = {"reduce": run_reduce, "small": run_small}


def main(argv):
    if len(argv) != 2 or argv[1] not in SETS:
        print(__doc__, file=sys.stderr)
        return 2
    sys.path.insert(0, os.path.dirname(_HERE))
    sys.path.insert(0, _HERE)
    import distributedarrays_jl_amd as dja
    from distributedarrays_jl_amd import _ffi
    dja.comm.init()
    SETS[argv[1]](dja, _ffi.lib)
    dja.d_closeall()
    assert dja.bytes_in_use() == 0, "HBM leak: %d" % dja.bytes_in_use()
    print("variant ok: %s [%s]" % (argv[1], variant_id(
        {k: v for k, v in os.environ.items() if k.startswith("DA_")})))
    return 0


if __name__ == "__main__":
    sys.exit(main(sys.argv))
