#!/usr/bin/env python3
"""da_scan against da_d2d of the same byte count, same process, same
buffers: f64 add at one shape per kernel family.  The yardstick is the
copy (one read + one write), never the scan itself: the traffic model
says cols and block move what the copy moves (ratio 1.0) and spans moves
one more read (ratio 1.5).

Timing: da_event_* around each call, 3 warm-ups, median of --runs (>= 10)
runs, scan and copy runs interleaved so both see the same clocks.  One
JSON line per shape, then a markdown table.  One process per invocation;
bound it from outside:

    timeout -k 10 300 python tools/scan_bench.py [--runs 15] [--small]
"""
import argparse
import ctypes
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

SHAPES = [((1, 1 << 28, 1), "spans", 1.5, "beyond the 256 MiB cache"),
          ((1, 1 << 24, 1), "spans", 1.5, "inside the cache"),
          ((1, 16384, 16384), "block", 1.0, ""),
          ((16384, 16384, 1), "cols", 1.0, "")]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=15)
    ap.add_argument("--small", action="store_true",
                    help="1/64 of every shape (plumbing check)")
    args = ap.parse_args()
    runs = max(args.runs, 10)

    import distributedarrays_jl_amd as dja
    from distributedarrays_jl_amd import _ffi
    from distributedarrays_jl_amd._ffi import lib, check
    dja.comm.init()

    e0, e1 = ctypes.c_void_p(), ctypes.c_void_p()
    check(lib.da_event_create(ctypes.byref(e0)))
    check(lib.da_event_create(ctypes.byref(e1)))

    def timed(fn):
        check(lib.da_event_record(e0))
        fn()
        check(lib.da_event_record(e1))
        ms = ctypes.c_float()
        check(lib.da_event_elapsed(e0, e1, ctypes.byref(ms)))
        return ms.value

    rows = []
    for (inner, axis, outer), fam, model, note in SHAPES:
        if args.small:
            if inner > 1:
                inner //= 64
            elif outer > 1:
                outer //= 64
            else:
                axis //= 64
        got = _ffi.SCAN_VARIANTS[lib.dbg_scan_variant(inner, axis, outer)]
        assert got == fam, ((inner, axis, outer), got, fam)
        n = inner * axis * outer
        src = dja.drand((n,), "f64")
        dst = dja.dzeros((n,), "f64")

        def scan():
            check(lib.da_scan(0, dst._ptr(), src._ptr(), inner, axis, outer,
                              0, None))

        def copy():
            check(lib.da_d2d(dst._ptr(), src._ptr(), n * 8))

        for _ in range(3):
            scan()
            copy()
        check(lib.da_synchronize())
        ts, tc = [], []
        for _ in range(runs):
            ts.append(timed(scan))
            tc.append(timed(copy))
        ms_s, ms_c = statistics.median(ts), statistics.median(tc)
        rec = {"shape": [inner, axis, outer], "family": fam,
               "scan_ms": round(ms_s, 4), "copy_ms": round(ms_c, 4),
               "ratio": round(ms_s / ms_c, 3), "model": model,
               "scan_min_max_ms": [round(min(ts), 4), round(max(ts), 4)],
               "copy_min_max_ms": [round(min(tc), 4), round(max(tc), 4)],
               "copy_gbs": round(2 * n * 8 / ms_c / 1e6, 1),
               "runs": runs, "note": note}
        print(json.dumps(rec), flush=True)
        rows.append(rec)
        src.close()
        dst.close()

    check(lib.da_event_destroy(e0))
    check(lib.da_event_destroy(e1))
    print("| shape | family | scan ms (min..max) | copy ms (min..max) | "
          "ratio | model |")
    print("|---|---|---|---|---|---|")
    for r in rows:
        print("| %s | %s | %.3f (%.3f..%.3f) | %.3f (%.3f..%.3f) | %.2f | "
              "%.1f |" % (tuple(r["shape"]), r["family"], r["scan_ms"],
                          r["scan_min_max_ms"][0], r["scan_min_max_ms"][1],
                          r["copy_ms"], r["copy_min_max_ms"][0],
                          r["copy_min_max_ms"][1], r["ratio"], r["model"]))
    dja.d_closeall()


if __name__ == "__main__":
    main()
