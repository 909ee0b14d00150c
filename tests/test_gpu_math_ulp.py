"""map/map2 math on the device, in ulps against a high-precision reference
(tests/ulp_ref.py), on inputs chosen to be hard: every quadrant and sign,
the doubles nearest multiples of pi/2, the switch points of fastmath.hpp,
the hand-over to OCML, +-0, subnormals, +-inf, NaN.

  a  IEEE-exact ops: the bits of numpy
  b  f64 sin/cos/exp (the project's own polynomials): <= 1 ulp, and the
     bits of the CPU model tests/fastmath_model.py on the fast range
  c  OCML-backed ops: <= ceiling(op, dtype), derived in advance from host
     libm on the same inputs (ulp_ref.CEILINGS)
  d  binary ops on a signed grid, array and scalar forms
  e  every route to the functor table gives the same bytes (compared in a
     fresh process, tests/route_bits_child.py)

Every case prints its worst figure before it asserts.
"""
import contextlib

import numpy as np
import pytest

import fastmath_model as fm
import kernel_ref as kr
import ulp_ref as U

pytestmark = pytest.mark.gpu

DTS = ("f64", "f32")

# OCML routines measured over their ceiling on the MI355X:
# (op, dtype): (measured ulps, worst input, allowed = 2 * measured).
# Only OCML-backed ops may appear here; never sin/cos/exp in f64, the
# exact ops or mod/rem/min2/max2.
KNOWN_LOOSE = {
    # OCML tgammaf on the negative axis; host (scipy, via f64) 0.5 ulp
    ("gamma", "f32"): (5.9105, -15.16215991973877, 2 * 5.9105),
}


@pytest.fixture(scope="module")
def dja():
    import distributedarrays_jl_amd as dja
    dja.comm.init()
    yield dja
    dja.d_closeall()


@contextlib.contextmanager
def device_guard():
    """No case here passes the library an argument it should reject, so an
    error from it is a device error: end the session instead of launching
    the remaining cases on a device in an unknown state."""
    from distributedarrays_jl_amd._ffi import DArrayError
    try:
        yield
    except DArrayError as e:
        pytest.exit("device error, stopping: %r" % (e,), returncode=3)


def dev_map(dja, op, x):
    with device_guard():
        d = dja.distribute(x)
        out = dja.dmap(op, d)
        got = out.localpart().copy()
        out.close(); d.close()
    assert got.dtype == x.dtype and got.shape == x.shape
    return got


def dev_map2(dja, op, a, b):
    with device_guard():
        da_, db = dja.distribute(a), dja.distribute(b)
        out = dja.elementwise(op, da_, db)
        got = out.localpart().copy()
        out.close(); da_.close(); db.close()
    return got


def same_bits(got, ref):
    """Index of the first element that differs in bits (NaN matches NaN of
    any payload), or None."""
    assert got.dtype == ref.dtype and got.shape == ref.shape
    bad = (kr.bits(got) != kr.bits(ref)) & ~(np.isnan(got) & np.isnan(ref))
    return int(np.flatnonzero(bad)[0]) if bad.any() else None


# ------------------------------------------------------------- a. exact ops
def _sign(x):       # Julia sign: NaN and signed zeros pass through
    with np.errstate(invalid="ignore"):
        return np.where((x == 0) | np.isnan(x), x, np.sign(x))


EXACT_REF = {
    "identity": lambda x: x.copy(), "neg": lambda x: -x, "abs": np.abs,
    "abs2": lambda x: x * x, "inv": lambda x: x.dtype.type(1) / x,
    "sqrt": np.sqrt, "floor": np.floor, "ceil": np.ceil, "round": np.rint,
    "trunc": np.trunc, "sign": _sign,
    "isnan": lambda x: np.isnan(x).astype(x.dtype),
    "isinf": lambda x: np.isinf(x).astype(x.dtype),
    "isfinite": lambda x: np.isfinite(x).astype(x.dtype),
}


@pytest.mark.parametrize("dt", DTS)
@pytest.mark.parametrize("op", U.EXACT)
def test_exact_ops_bits(dja, op, dt):
    x = U.vector(op, dt)
    # halves and integers, where floor/ceil/round/trunc decide
    x = np.concatenate([x[:100], (np.arange(-8, 8) * 0.5).astype(x.dtype),
                        x[100:]])
    assert len(x) % 4 == 3
    with np.errstate(all="ignore"):
        ref = np.asarray(EXACT_REF[op](x), dtype=x.dtype)
    got = dev_map(dja, op, x)
    j = same_bits(got, ref)
    assert j is None, (op, dt, x[j], got[j], ref[j])


# ---------------------------------------- b. the project's own sin/cos/exp
OUTSIDE_FAST = 3.0    # host libm stays under 1 ulp there; rule (c): 1 + 2


def _owned_vectors(op):
    yield "sweep", U.vector(op, "f64"), U.reference_cached(op, "f64")
    if op != "exp":
        for which in ("near", "deep"):
            x = U.pio2_hard(which)
            ref = U.reference(op, x[x > 0], "f64", use_mp=True)
            full = np.empty(len(x), dtype=U.HI["f64"])
            full[x > 0] = ref
            full[x < 0] = _mirror(op, x, ref)
            yield which, x, full


def _mirror(op, x, ref_pos):
    """Reference at the negative entries of x from the reference at the
    positive ones: sin is odd and cos is even, exactly, which halves the
    mpmath evaluations."""
    pos, neg = x[x > 0], x[x < 0]
    lookup = dict(zip(pos.tolist(), range(len(pos))))
    idx = np.array([lookup[-v] for v in neg.tolist()])
    return -ref_pos[idx] if op == "sin" else ref_pos[idx]


@pytest.mark.parametrize("op", ["sin", "cos", "exp"])
def test_owned_f64_one_ulp_and_model_bits(dja, op):
    for name, x, ref in _owned_vectors(op):
        got = dev_map(dja, op, x)
        err = U.ulp_err(got, ref, "f64")
        fast = fm.fast_range(op, x)
        w_in, at_in = U.worst(err[fast], x[fast])
        print("%s f64 %s: fast range worst %.4f ulp at %r" % (
            op, name, w_in, float(at_in)))
        model = fm.MODEL[op](x[fast])
        j = same_bits(got[fast], model)
        assert w_in <= 1.0 + U.REF_SLACK, (op, name, w_in, float(at_in))
        if (~fast).any():
            w_out, at_out = U.worst(err[~fast], x[~fast])
            print("%s f64 %s: beyond the fast range worst %.4f ulp at %r" % (
                op, name, w_out, float(at_out)))
            assert w_out <= OUTSIDE_FAST + U.REF_SLACK, (op, w_out, at_out)
        assert j is None, "device differs from fastmath_model at %r: " \
            "%r vs %r" % (x[fast][j], got[fast][j], model[j])


# ------------------------------------------------------ c. OCML-backed ops
CASES_C = [(op, dt) for dt in DTS for op in U.TRANSCENDENTAL
           if (op, dt) not in U.OWNED]


@pytest.mark.parametrize("op,dt", CASES_C)
def test_ocml_ops_within_ceiling(dja, op, dt):
    x = U.vector(op, dt)
    ref = U.reference_cached(op, dt)
    got = dev_map(dja, op, x)
    err = U.ulp_err(got, ref, dt)
    w, at = U.worst(err, x)
    limit = U.bound(op, dt, U.ceiling(op, dt))
    if (op, dt) in KNOWN_LOOSE:
        limit = U.bound(op, dt, KNOWN_LOOSE[(op, dt)][2])
    print("%s %s: worst %.4f ulp at %r, limit %.4f" % (
        op, dt, w, float(at), limit))
    assert w <= limit, (op, dt, limit, U.describe(err, x, got, ref))


def test_known_loose_holds_ocml_only():
    for (op, dt), (meas, at, allowed) in KNOWN_LOOSE.items():
        assert (op, dt) not in U.OWNED and op not in U.EXACT, (op, dt)
        assert op not in ("mod", "rem", "min2", "max2", "deg2rad",
                          "rad2deg"), op
        assert allowed == 2 * meas, (op, dt)


# ------------------------------------------------------------ d. binary ops
def _minmax_ref(op):
    """numpy's NaN-propagating minimum/maximum.  Only where BOTH operands
    are zeros is the pick spelled out (the second operand, as in
    mapops.hpp): numpy's vector loops do not fix which zero they return."""
    def f(a, b):
        r = (np.minimum if op == "min2" else np.maximum)(a, b)
        return np.where((a == 0) & (b == 0), b, r)
    return f


EXACT2_REF = {"add": np.add, "sub": np.subtract, "mul": np.multiply,
              "div": np.divide, "min2": _minmax_ref("min2"),
              "max2": _minmax_ref("max2"), "rem": np.fmod, "mod": np.mod}


@pytest.mark.parametrize("dt", DTS)
@pytest.mark.parametrize("op", sorted(EXACT2_REF))
def test_map2_exact_bits_signed_grid(dja, op, dt):
    a, b = U.grid2(dt)
    with np.errstate(all="ignore"):
        ref = np.asarray(EXACT2_REF[op](a, b), dtype=a.dtype)
    got = dev_map2(dja, op, a, b)
    j = same_bits(got, ref)
    assert j is None, (op, dt, a[j], b[j], got[j], ref[j])
    if op == "mod":      # the bits already say so; spelled out all the same
        z = got == 0
        assert np.array_equal(np.signbit(got[z]), np.signbit(ref[z]))
        assert dev_map2(dja, "mod", np.array([-2.0, 2.0, -0.0], a.dtype),
                        np.array([1.0, -1.0, 3.0], a.dtype)).tolist() \
            == [0.0, -0.0, 0.0]


@pytest.mark.parametrize("dt", DTS)
@pytest.mark.parametrize("op", ["pow", "atan2"])
def test_map2_pow_atan2_ulps(dja, op, dt):
    a, b = U.grid2(dt)
    ref = U.reference2_cached(op, dt)
    got = dev_map2(dja, op, a, b)
    err = U.ulp_err(got, ref, dt)
    j = int(np.argmax(err))
    limit = U.bound(op, dt, U.ceiling(op, dt))
    if (op, dt) in KNOWN_LOOSE:
        limit = U.bound(op, dt, KNOWN_LOOSE[(op, dt)][2])
    print("%s %s: worst %.4f ulp at (%r, %r), limit %.4f" % (
        op, dt, err[j], float(a[j]), float(b[j]), limit))
    assert err[j] <= limit, (op, dt, err[j], a[j], b[j], got[j])


SCALARS = [0.0, -0.0, 1.5, -2.0, 3.0, -2.5, float(2 ** -149), np.inf, -np.inf,
           np.nan]


@pytest.mark.parametrize("dt", DTS)
def test_map2_scalar_both_orders_match_array_form(dja, dt):
    """da_map2_scalar(op, x, c, reverse) against da_map2 on (x, c...) and
    (c..., x): the same bits, for every float binary op."""
    T = U.NP[dt]
    a, b = U.grid2(dt)
    g = np.unique(kr.bits(a)).view(T)            # the grid itself, once
    g = g[:len(g) - ((len(g) - 3) % 4)]
    d = dja.distribute(g)
    try:
        for c in SCALARS:
            cv = np.full(g.shape, c, dtype=T)
            for op in sorted(EXACT2_REF) + ["pow", "atan2"]:
                for reverse in (False, True):
                    out = dja.elementwise_scalar(op, d, c, reverse=reverse)
                    got = out.localpart().copy()
                    out.close()
                    ref = dev_map2(dja, op, cv, g) if reverse \
                        else dev_map2(dja, op, g, cv)
                    j = same_bits(got, ref)
                    assert j is None, (op, dt, c, reverse, g[j], got[j],
                                       ref[j])
    finally:
        d.close()


# -------------------------------------------------------- e. route identity
# The hipRTC route compiles at run time with whichever code-object manager
# (libamd_comgr) the process loaded FIRST.  The package pins the ROCm one
# when it is imported before torch (_ffi.py); in this pytest process other
# test modules import torch during collection, torch's bundled comgr wins,
# and its OCML tgamma is 2 ulp away from the one hipcc linked into the
# library (measured: gamma(1.0) = 0.9999999999999998 from the JIT against
# 1.0, 471 of 3239 f64 elements differ; every other op agreed).  So the
# routes are compared in a fresh process that imports the package first, as
# bench.py and the examples do: tests/route_bits_child.py.
import route_bits_child as rbc


@pytest.fixture(scope="module")
def route_report(tmp_path_factory):
    import json
    import subprocess
    import sys
    out = tmp_path_factory.mktemp("routes") / "report.json"
    r = subprocess.run([sys.executable, rbc.__file__, str(out)],
                       capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, (r.returncode, r.stdout[-2000:],
                               r.stderr[-2000:])
    return json.loads(out.read_text())


def test_routes_child_ran_the_jit(route_report):
    assert route_report["jit_state"] == 2, route_report["jit_err"]
    assert route_report["comgr"], "no comgr in the child's maps"
    assert "torch" not in route_report["comgr"][0], route_report["comgr"]


@pytest.mark.parametrize("dt", DTS)
@pytest.mark.parametrize("op", rbc.UNARY)
def test_routes_identical_bytes(route_report, op, dt):
    """da_map, a one-op da_expr program through hipRTC, the same through
    the interpreter; for sin/cos/exp also the fused max-reduce."""
    assert route_report["unary"]["%s|%s" % (op, dt)] is None


@pytest.mark.parametrize("dt", DTS)
@pytest.mark.parametrize("op", rbc.BINARY)
def test_routes_identical_bytes_binary(route_report, op, dt):
    assert route_report["binary"]["%s|%s" % (op, dt)] is None
