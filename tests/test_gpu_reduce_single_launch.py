"""The single-launch flat reduce and count (last block to finish folds the
partials and writes the result to pinned host memory): grid and tail
edges for every dtype and op, a warm-cache stale-partial check, ticket
integrity across changing grids and dtypes, bit identity with the
two-kernel path, and the two-kernel path itself under DA_RED_FUSED=0.

Bounds: min/max, every i64 op and every count are exact.  Float sums use
the any-order bound (n-1)*u*sum|v| of kernel_ref against a longdouble
sum.  Float products use data whose product is exact in ANY order: ones,
with powers of two 2^e, 1 <= |e| <= 3, at no more than 44 sites (the
planting sites of kernel_checks plus 32 philox-drawn ones), signs
alternating.  Every partial product is then a power of two no further
from 1 than 2^+-66, inside f32's normal range, so the product must match
bit for bit."""
import ctypes
import os
import subprocess
import sys

import numpy as np
import pytest

import kernel_checks as kc
import kernel_ref as kr

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
CTYPE = {"f64": ctypes.c_double, "f32": ctypes.c_float, "i64": ctypes.c_int64}
EDGES = [0, 1, 2, 3, 255, 256, 257, 511, 513,
         (1 << 20) - 1, 1 << 20, (1 << 20) + 1, (1 << 22) + 1]
DTYPES = ["f64", "f32", "i64"]
CHILD_TIMEOUT = 120
_faulted = []     # children that died; non-empty stops further children


@pytest.fixture(scope="module")
def dja():
    import distributedarrays_jl_amd as dja
    dja.comm.init()
    return dja


def raw_reduce(f, op, buf, n, dt):
    from distributedarrays_jl_amd._ffi import lib, check
    out = CTYPE[dt]()
    check(lib.da_reduce(kr.MAPOP[f], kr.REDOP[op], buf.p, n, kr.DT[dt],
                        ctypes.byref(out)))
    return kr.NP[dt].type(out.value)


def raw_count(pred, buf, n, dt):
    from distributedarrays_jl_amd._ffi import lib, check
    out = ctypes.c_int64(-1)
    check(lib.da_count(kr.MAPOP[pred], buf.p, n, kr.DT[dt],
                       ctypes.byref(out)))
    return out.value


def same_bits(a, b):
    return kr.bits(np.array([a]))[0] == kr.bits(np.array([b]))[0]


def product_input(n, dt):
    """(x, exact product).  Floats: see the module docstring.  i64: odd
    philox values, whose wrapped product never collapses to zero."""
    if dt == "i64":
        x = kr.philox.fill_int64(n, 77) | np.int64(1)
        with np.errstate(over="ignore"):
            return x, np.int64(np.prod(x, dtype=np.int64)) if n else np.int64(1)
    x = np.ones(n, dtype=kr.NP[dt])
    sites = kc.tree_positions(n) if n else []
    extra = [int(p) for p in np.mod(kr.philox.fill_int64(32, 78), max(n, 1))]
    for p in extra:
        if p not in sites and 0 <= p < n:
            sites.append(p)
    total = 0
    for k, p in enumerate(sites):
        e = (k // 2) % 3 + 1
        e = e if k % 2 == 0 else -e       # +e, -e, +e', -e', ...
        x[p] = 2.0 ** e
        total += e
    return x, kr.NP[dt].type(2.0 ** total)


def check_float_sum(got, v, dt, tag):
    w = v.astype(np.longdouble)
    bound = max(v.size - 1, 0) * np.longdouble(kr.UNIT[dt]) * np.abs(w).sum()
    err = abs(np.longdouble(got) - w.sum())
    assert err <= bound, (tag, got, float(err), float(bound))


@pytest.mark.parametrize("dt", DTYPES)
@pytest.mark.parametrize("n", EDGES)
def test_ops_at_edges(dja, n, dt):
    """The planted-value and in-bound checks of kernel_checks, then add,
    mul, max, min; abs2+add; abs+add; abs+max (no constant-folded
    instantiation: the runtime-switch kernel); the three predicates."""
    if n:
        kc.check_planted_extrema(dja, dt, n)
        if dt != "i64":
            kc.check_planted_nan(dja, dt, n)
        kc.check_sum_in_bound(dja, dt, n, 700 + kr.DT[dt])
    x = kc.tree_base(n, dt)            # shared with the planted checks
    if dt != "i64":
        x = x - kr.NP[dt].type(0.5)
    px, pwant = product_input(n, dt)
    buf, pbuf = kr.Dev.of(x), kr.Dev.of(px)
    try:
        tag = (dt, n)
        if n == 0:
            for op in ("add", "mul", "min", "max"):
                assert same_bits(raw_reduce("identity", op, buf, 0, dt),
                                 kr.fold_identity(op, dt)), (tag, op)
        else:
            assert same_bits(raw_reduce("identity", "max", buf, n, dt),
                             x.max()), tag
            assert same_bits(raw_reduce("identity", "min", buf, n, dt),
                             x.min()), tag
            assert same_bits(raw_reduce("abs", "max", buf, n, dt),
                             np.abs(x).max()), tag
        assert same_bits(raw_reduce("identity", "mul", pbuf, n, dt),
                         pwant), (tag, "mul")
        for f in ("identity", "abs2", "abs"):
            v = kr.map_values(f, x)
            got = raw_reduce(f, "add", buf, n, dt)
            if dt == "i64":
                assert got == v.sum(dtype=np.int64), (tag, f)
            else:
                check_float_sum(got, v, dt, (tag, f))
        assert raw_count("nonzero", buf, n, dt) == np.count_nonzero(x), tag
        assert raw_count("isfinite", buf, n, dt) == n, tag
        assert raw_count("isnan", buf, n, dt) == 0, tag
        if dt != "i64" and n:
            y = x.copy()
            y[0] = np.inf
            y[n // 2] = 0.0
            y[n - 1] = np.nan                   # scalar tail / last pair
            buf.put(y)                          # (sites coincide for n < 3)
            assert raw_count("isnan", buf, n, dt) == 1, tag
            assert raw_count("isfinite", buf, n, dt) == \
                int(np.isfinite(y).sum()), tag
            assert raw_count("nonzero", buf, n, dt) == \
                int(np.count_nonzero(y)), tag
    finally:
        pbuf.free()
        buf.free()


@pytest.mark.parametrize("n", EDGES[1:])
def test_each_element_once_at_edges(dja, n):
    kc.check_once_only(dja, n)


@pytest.mark.parametrize("n", [(1 << 20) + 1, 513])
def test_no_stale_partials(dja, n):
    """Two arrays whose every element, hence every block partial, differs,
    reduced alternately: the last arriver's CU has the other array's
    partials of the previous launch in its cache, so a fold that reads them
    without the acquire returns a wrong integer."""
    a = kc.golden_sequence(n)
    with np.errstate(over="ignore"):
        b = a * np.int64(3) + np.int64(1)
        want = (np.int64(a.sum(dtype=np.int64)),
                np.int64(b.sum(dtype=np.int64)))
    assert want[0] != want[1]
    bufs = (kr.Dev.of(a), kr.Dev.of(b))
    try:
        for it in range(120):
            k = it & 1
            got = raw_reduce("identity", "add", bufs[k], n, "i64")
            assert got == want[k], (n, it, got, want[k])
    finally:
        bufs[1].free()
        bufs[0].free()


def test_ticket_survives_grid_and_dtype_changes(dja):
    """216 back-to-back calls in one process: n (hence grid) and dtype
    change every call, da_reduce alternates with da_count.  Integer-valued
    data in [-8, 8] keeps every sum exact in every dtype (|sum| <= 8n <
    2^24), so one missed or doubled last arriver shows as a wrong value."""
    sizes = (1, 257, 100001, 2, (1 << 20) + 1, 513)
    data = {}
    try:
        for n in sizes:
            for dt in DTYPES:
                x = kr.small_ints(n, 40 + n % 7, 8).astype(kr.NP[dt])
                data[n, dt] = (kr.Dev.of(x), x.sum(dtype=np.int64),
                               int(np.count_nonzero(x)))
        for i in range(216):
            n = sizes[i % 6]
            dt = DTYPES[(i + i // 6) % 3]
            buf, want_sum, want_nz = data[n, dt]
            if i % 3 == 2:
                assert raw_count("nonzero", buf, n, dt) == want_nz, (i, n, dt)
            else:
                got = raw_reduce("identity", "add", buf, n, dt)
                assert int(got) == want_sum, (i, n, dt, got, want_sum)
    finally:
        for buf, _, _ in data.values():
            buf.free()


def run_child(script, args, env_extra, tag):
    """One child at a time, under its own timeout; after a child that died
    no further child is started."""
    if _faulted:
        pytest.skip("an earlier child faulted (%s); not starting further "
                    "GPU processes" % _faulted[0])
    env = dict(os.environ)
    env.update(env_extra)
    try:
        r = subprocess.run([sys.executable, os.path.join(HERE, script)] + args,
                           env=env, capture_output=True, text=True,
                           timeout=CHILD_TIMEOUT)
    except subprocess.TimeoutExpired:
        _faulted.append(tag)
        pytest.fail("%s: child exceeded %d s" % (tag, CHILD_TIMEOUT))
    if r.returncode < 0 or r.returncode in (134, 139):
        _faulted.append(tag)
    assert r.returncode == 0, "%s: child exit %d\n%s" % (
        tag, r.returncode, r.stderr[-2000:])
    return r.stdout


def test_single_launch_and_two_kernel_bits_agree():
    one = run_child("reduce_bits_child.py", [], {}, "bits default")
    two = run_child("reduce_bits_child.py", [], {"DA_RED_FUSED": "0"},
                    "bits DA_RED_FUSED=0")
    assert one.endswith("bits done\n") and one.count("\n") == 19, one
    assert one == two


def test_two_kernel_path_still_works():
    out = run_child("variant_child.py", ["reduce"], {"DA_RED_FUSED": "0"},
                    "reduce DA_RED_FUSED=0")
    assert "variant ok: reduce" in out
