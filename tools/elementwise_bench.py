#!/usr/bin/env python3
"""Every launcher of kernels_elementwise x every dtype it accepts: the bits
it produces and the time it takes, at ABI level.

Per leg, first one call at n = 4099 on fixed-seed philox inputs with
specials planted at both ends (NaN, -0.0, inf, 0.0; ties for the casts)
and the SHA-256 of the output bytes: two builds that print the same digests
compute the same bits, normals and transcendentals included.  Then the
same call at 2^27 elements (1 GiB per 8-byte array, beyond the 256 MiB
cache).

Timing: da_event_* around each call, 3 warm-ups, median of --runs (>= 10)
runs.  One JSON line per leg.  One process per invocation; bound it from
outside:

    timeout -k 10 300 python tools/elementwise_bench.py [--runs 15] [--small]
"""
import argparse
import ctypes
import hashlib
import json
import os
import statistics
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

DIGEST_N = 4099
NP = {"f64": np.float64, "f32": np.float32, "i64": np.int64}
DT = {"f64": 0, "f32": 1, "i64": 2}
FLOATS, ALL = ("f64", "f32"), ("f64", "f32", "i64")


def host_input(dt, n, seed, specials=True):
    """philox data: floats in [-0.5, 0.5) with specials at both ends, raw
    bits for i64."""
    from oracle import philox
    if dt == "i64":
        return philox.fill_int64(n, seed)
    fill = philox.fill_uniform_f64 if dt == "f64" else philox.fill_uniform_f32
    x = (fill(n, seed) - NP[dt](0.5)).astype(NP[dt])
    if specials:
        sp = (np.nan, -0.0, np.inf, 0.0, -np.inf)
        x[:len(sp)] = sp
        x[n - len(sp):] = sp[::-1]
    return x


def legs(lib, MAP_OP, MAP2_OP):
    """(name, dst dtype, [src dtypes], in-place, bytes moved per element,
    call(dst, srcs, n), input kind)."""
    out = []

    def add(name, dd, sds, call, inplace=False, kind="specials"):
        size = {"f64": 8, "f32": 4, "i64": 8}
        moved = size[dd] * (2 if inplace else 1) + sum(size[s] for s in sds)
        out.append((name, dd, sds, inplace, moved, call, kind))

    for dt in ALL:
        c = DT[dt]
        add("fill_%s" % dt, dt, [],
            lambda d, s, n, c=c: lib.da_fill(d, 2.5, n, c))
        add("rand_uniform_%s" % dt, dt, [],
            lambda d, s, n, c=c: lib.da_rand(d, n, c, 4321, 0, 3))
        if dt != "i64":
            add("rand_normal_%s" % dt, dt, [],
                lambda d, s, n, c=c: lib.da_rand(d, n, c, 4321, 1, 3))
        ops = ("neg",) if dt == "i64" else ("sin", "abs2", "ceil")
        for op in ops:           # hot transcendental, hot exact, cold
            add("map_%s_%s" % (op, dt), dt, [dt],
                lambda d, s, n, c=c, o=MAP_OP[op]: lib.da_map(o, d, s[0], n,
                                                              c))
        add("map2_add_%s" % dt, dt, [dt, dt],
            lambda d, s, n, c=c: lib.da_map2(MAP2_OP["add"], d, s[0], s[1],
                                             n, c))
        add("map2_scalar_mul_%s" % dt, dt, [dt],
            lambda d, s, n, c=c: lib.da_map2_scalar(MAP2_OP["mul"], d, s[0],
                                                    3.0, 0, n, c))
        if dt != "i64":
            add("bcast_fma_%s" % dt, dt, [dt, dt],
                lambda d, s, n, c=c: lib.da_bcast_fma(d, s[0], s[1], 0.25,
                                                      n, c))
            add("axpby_%s" % dt, dt, [dt],
                lambda d, s, n, c=c: lib.da_axpby(d, s[0], -0.5, 0.75, n, c),
                inplace=True)
        add("add_scaled_%s" % dt, dt, [dt],
            lambda d, s, n, c=c: lib.da_add(d, s[0], -3.0, n, c),
            inplace=True)
        add("add_unit_%s" % dt, dt, [dt],
            lambda d, s, n, c=c: lib.da_add(d, s[0], 1.0, n, c),
            inplace=True)
        add("scale_%s" % dt, dt, [],
            lambda d, s, n, c=c: lib.da_scale(d, 3.0, n, c), inplace=True)
        for sd in ALL:
            if sd != dt:
                add("cast_%s_from_%s" % (dt, sd), dt, [sd],
                    lambda d, s, n, c=c, sc=DT[sd]: lib.da_cast(d, c, s[0],
                                                                sc, n),
                    kind="ties")
        add("transpose_%s" % dt, dt, [dt],
            lambda d, s, n, c=c: lib.da_transpose(d, s[0], *shape2(n), c))
        if dt != "i64":
            add("diag_scale_%s" % dt, dt, [dt],
                lambda d, s, n, c=c: lib.da_diag_scale(d, *shape2(n), s[0],
                                                       0, c),
                inplace=True)
    return out


def shape2(n):
    """n as m x k with m the largest power of two <= sqrt(n) dividing n,
    or 1 x n when n is odd."""
    m = 1
    while n % (2 * m) == 0 and (2 * m) * (2 * m) <= n:
        m *= 2
    return m, n // m


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=15)
    ap.add_argument("--small", action="store_true",
                    help="2^20 elements (plumbing check)")
    args = ap.parse_args()
    runs = max(args.runs, 10)
    n_big = 1 << (20 if args.small else 27)

    import distributedarrays_jl_amd as dja
    from distributedarrays_jl_amd._ffi import lib, check
    from distributedarrays_jl_amd._opcodes import MAP_OP, MAP2_OP
    dja.comm.init()

    e0, e1 = ctypes.c_void_p(), ctypes.c_void_p()
    check(lib.da_event_create(ctypes.byref(e0)))
    check(lib.da_event_create(ctypes.byref(e1)))

    def timed(fn):
        check(lib.da_event_record(e0))
        check(fn())
        check(lib.da_event_record(e1))
        ms = ctypes.c_float()
        check(lib.da_event_elapsed(e0, e1, ctypes.byref(ms)))
        return ms.value

    def alloc(nbytes):
        p = ctypes.c_void_p()
        check(lib.da_alloc(nbytes, 0, ctypes.byref(p)))
        return p

    def upload(arr):
        p = alloc(arr.nbytes)
        check(lib.da_h2d(p, arr.ctypes.data, arr.nbytes))
        return p

    for name, dd, sds, inplace, moved, call, kind in legs(lib, MAP_OP,
                                                          MAP2_OP):
        # ---- bits at n = 4099
        n = DIGEST_N
        hs = [host_input(sd, n, 70 + k, kind == "specials")
              for k, sd in enumerate(sds)]
        if kind == "ties":
            for h in hs:
                if h.dtype.kind == "f":
                    h *= h.dtype.type(1000)
                    h[:6] = (0.5, -0.5, 1.5, -1.5, 2.5, -2.5)
        if name.startswith("diag_scale"):
            hs = [hs[0][:shape2(n)[0]]]
        hd = host_input(dd, n, 69) if inplace else np.zeros(n, NP[dd])
        srcs = [upload(np.ascontiguousarray(h)) for h in hs]
        dst = upload(hd)
        check(call(dst, srcs, n))
        out = np.empty(n, NP[dd])
        check(lib.da_d2h(dst, out.ctypes.data, out.nbytes))
        sha = hashlib.sha256(out.tobytes()).hexdigest()
        for p in srcs + [dst]:
            check(lib.da_free(p))

        # ---- time at 2^27: inputs made on the device
        n = n_big
        size = {"f64": 8, "f32": 4, "i64": 8}
        srcs = []
        for k, sd in enumerate(sds):
            p = alloc(n * size[sd])
            check(lib.da_rand(p, n, DT[sd], 80 + k, 0, 0))
            srcs.append(p)
        dst = alloc(n * size[dd])
        check(lib.da_rand(dst, n, DT[dd], 79, 0, 0))
        for _ in range(3):
            check(call(dst, srcs, n))
        check(lib.da_synchronize())
        ts = [timed(lambda: call(dst, srcs, n)) for _ in range(runs)]
        for p in srcs + [dst]:
            check(lib.da_free(p))
        ms = statistics.median(ts)
        print(json.dumps({"leg": name, "n": n, "ms": round(ms, 4),
                          "min_max_ms": [round(min(ts), 4),
                                         round(max(ts), 4)],
                          "gbs": round(moved * n / ms / 1e6, 1),
                          "runs": runs, "sha256_n4099": sha}), flush=True)

    check(lib.da_event_destroy(e0))
    check(lib.da_event_destroy(e1))
    dja.d_closeall()


if __name__ == "__main__":
    main()
