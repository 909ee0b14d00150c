#!/usr/bin/env python3
"""The fused dims-reduction (expr.reduce with dims) against the routes the
library had before it, same process, same arrays, f64:

  demean   sum(abs2, X .- mu; dims) at 16384^2, mu a row: fused (8 B per
           element) against expr.materialize + dsum_dims (24 B: read X,
           write the temporary, read it again).  GATE: fused is faster.
  3d       sum(D; dims=(0,1)) on a 1024 x 1024 x 256 array (2 GiB): fused
           against the per-axis dsum_dims, which writes an intermediate
           between the axes.  GATE: fused is not slower.
  plain    sum(X; dims) of a bare array at 16384^2, dims 0 and 1: the
           general kernel against the specialised da_reduce_dims kernels
           behind dsum_dims.  Recorded, not gated.

Timing: da_event_* around each whole call (kernels, the slab combine and
its stream sync included), 3 warm-ups, median of --runs (>= 10) runs, the
two routes of a case interleaved so both see the same clocks.  GB/s is the
ALGORITHMIC byte count of each route over its time.  One JSON line per
case, then a markdown table; exit status 1 if a gate fails.  One process
per invocation; bound it from outside:

    timeout -k 10 300 python tools/expr_dims_bench.py [--runs 15] [--small]
"""
import argparse
import ctypes
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=15)
    ap.add_argument("--small", action="store_true",
                    help="1/64 of every array (plumbing check)")
    args = ap.parse_args()
    runs = max(args.runs, 10)

    import distributedarrays_jl_amd as dja
    from distributedarrays_jl_amd import _ffi, expr as E
    from distributedarrays_jl_amd._ffi import lib, check
    dja.comm.init()

    e0, e1 = ctypes.c_void_p(), ctypes.c_void_p()
    check(lib.da_event_create(ctypes.byref(e0)))
    check(lib.da_event_create(ctypes.byref(e1)))

    def timed(fn):
        check(lib.da_event_record(e0))
        fn()
        check(lib.da_event_record(e1))
        check(lib.da_synchronize())
        ms = ctypes.c_float()
        check(lib.da_event_elapsed(e0, e1, ctypes.byref(ms)))
        return ms.value

    def variant(shape, dims):
        arr = (ctypes.c_uint64 * len(shape))(*shape)
        nb, gx = ctypes.c_uint32(), ctypes.c_uint32()
        rc = lib.dbg_expr_dims_variant(arr, len(shape),
                                       sum(1 << a for a in dims),
                                       ctypes.byref(nb), ctypes.byref(gx))
        return "%s nb=%d gx=%d" % (_ffi.EXPR_DIMS_VARIANTS[rc], nb.value,
                                   gx.value)

    rows = []

    def case(name, shape, dims, fused, other, other_name, fused_bytes,
             other_bytes, gate):
        def a():
            fused().close()

        def b():
            other().close()

        for _ in range(3):
            a()
            b()
        tf, to = [], []
        for _ in range(runs):
            tf.append(timed(a))
            to.append(timed(b))
        mf, mo = statistics.median(tf), statistics.median(to)
        ok = None if gate is None else bool(mf < mo if gate == "faster"
                                            else mf <= mo)
        rec = {"case": name, "shape": list(shape), "dims": list(dims),
               "schedule": variant(shape, dims),
               "fused_ms": round(mf, 4), "other": other_name,
               "other_ms": round(mo, 4),
               "fused_min_max_ms": [round(min(tf), 4), round(max(tf), 4)],
               "other_min_max_ms": [round(min(to), 4), round(max(to), 4)],
               "other_over_fused": round(mo / mf, 3),
               "fused_bytes": fused_bytes, "other_bytes": other_bytes,
               "fused_gbs": round(fused_bytes / mf / 1e6, 1),
               "other_gbs": round(other_bytes / mo / 1e6, 1),
               "gate": gate, "gate_ok": ok, "runs": runs}
        print(json.dumps(rec), flush=True)
        rows.append(rec)

    m = 16384 // (8 if args.small else 1)
    X = dja.drand((m, m), "f64", dist=(1, 1))
    n = m * m
    for dims in ((0,), (1,)):
        mu = dja.dmean_dims(X, dims)
        e = E.abs2(E.ref(X) - E.ref(mu))

        def two_step(e=e, dims=dims):
            tmp = E.materialize(e)
            try:
                return dja.dsum_dims(tmp, dims)
            finally:
                tmp.close()

        case("demean", (m, m), dims,
             lambda e=e, dims=dims: E.reduce("add", e, dims=dims), two_step,
             "materialize + dsum_dims", 8 * n, 24 * n,
             "faster" if dims == (0,) else None)
        mu.close()
    for dims in ((0,), (1,)):
        case("plain", (m, m), dims,
             lambda dims=dims: E.reduce("add", E.ref(X), dims=dims),
             lambda dims=dims: dja.dsum_dims(X, dims), "dsum_dims",
             8 * n, 8 * n, None)
    X.close()

    s3 = (1024 // (8 if args.small else 1), 1024 // (8 if args.small else 1),
          256)
    D = dja.drand(s3, "f64", dist=(1, 1, 1))
    n3 = s3[0] * s3[1] * s3[2]
    # per-axis route: read D, write and re-read the (1, 1024, 256) rows
    case("3d", s3, (0, 1),
         lambda: E.reduce("add", E.ref(D), dims=(0, 1)),
         lambda: dja.dsum_dims(D, (0, 1)), "dsum_dims (per axis)",
         8 * n3, 8 * n3 + 16 * s3[1] * s3[2], "not slower")
    D.close()

    check(lib.da_event_destroy(e0))
    check(lib.da_event_destroy(e1))
    print("| case | shape | dims | schedule | fused ms (min..max) | GB/s | "
          "other | other ms (min..max) | GB/s | other/fused | gate |")
    print("|---|---|---|---|---|---|---|---|---|---|---|")
    for r in rows:
        print("| %s | %s | %s | %s | %.3f (%.3f..%.3f) | %.0f | %s | "
              "%.3f (%.3f..%.3f) | %.0f | %.2f | %s |" % (
                  r["case"], tuple(r["shape"]), tuple(r["dims"]),
                  r["schedule"], r["fused_ms"], r["fused_min_max_ms"][0],
                  r["fused_min_max_ms"][1], r["fused_gbs"], r["other"],
                  r["other_ms"], r["other_min_max_ms"][0],
                  r["other_min_max_ms"][1], r["other_gbs"],
                  r["other_over_fused"],
                  "-" if r["gate"] is None else
                  "%s: %s" % (r["gate"], "ok" if r["gate_ok"] else "FAIL")))
    dja.d_closeall()
    return 0 if all(r["gate_ok"] is not False for r in rows) else 1


if __name__ == "__main__":
    sys.exit(main())
