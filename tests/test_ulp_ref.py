"""tests/ulp_ref.py on the CPU: the ulp measure at its edges, the host
libm inside every ceiling the device is held to, and the sensitivity of
the check to a two-ulp fault in one element."""
import numpy as np
import pytest

import ulp_ref as U

ld = np.longdouble


def _err(got, ref, dt):
    return float(U.ulp_err(np.array([got], dtype=U.NP[dt]),
                           np.array([ref], dtype=U.HI[dt]), dt)[0])


def test_ulp_err_binade_edges():
    up, dn = np.nextafter(1.0, 2.0), np.nextafter(1.0, 0.0)
    assert _err(up, ld(1), "f64") == 1.0          # ulp(1) = 2^-52 above
    assert _err(dn, ld(1), "f64") == 0.5          # ... and half that below
    # a reference just below the edge is measured in the SMALLER ulp even
    # though it rounds to 1.0
    just_below = ld(1) - ld(2.0) ** -60
    assert _err(1.0, just_below, "f64") == pytest.approx(2.0 ** -7)
    assert _err(up, just_below, "f64") == pytest.approx(2.0 + 2.0 ** -7)
    assert _err(np.float32(1) + np.float32(2.0 ** -23), 1.0, "f32") == 1.0
    assert _err(np.float32(1) - np.float32(2.0 ** -24), 1.0, "f32") == 0.5
    assert _err(1.0 + 2.0 ** -52, ld(1) + ld(2.0) ** -53, "f64") == 0.5


@pytest.mark.parametrize("dt", ["f64", "f32"])
def test_ulp_err_subnormal_zero_and_top(dt):
    T = U.NP[dt].type
    fi = np.finfo(U.NP[dt])
    sub = float(fi.smallest_subnormal)
    assert _err(T(sub), 0.0, dt) == np.inf        # an exact zero is exact
    assert _err(T(0), sub, dt) == 1.0
    assert _err(T(3 * sub), 2 * sub, dt) == 1.0
    assert _err(T(fi.tiny), float(fi.tiny) - sub, dt) == 1.0
    assert _err(T(0.0), 0.0, dt) == 0.0
    assert _err(T(-0.0), 0.0, dt) == np.inf       # the sign of zero
    assert _err(T(0.0), -0.0, dt) == np.inf
    assert _err(T(-0.0), -0.0, dt) == 0.0
    quarter = U.HI[dt].type(sub) / 4
    assert _err(T(-0.0), quarter, dt) == np.inf   # wrong-signed underflow
    assert _err(T(0.0), quarter, dt) == 0.25
    top = float(fi.max)
    assert _err(T(np.inf), top, dt) == 1.0        # inf stands for 2^(emax+1)
    assert _err(T(top), np.inf, dt) == np.inf
    assert _err(T(np.inf), np.inf, dt) == 0.0
    assert _err(T(np.inf), -np.inf, dt) == np.inf
    assert _err(T(np.nan), np.nan, dt) == 0.0
    assert _err(T(np.nan), 1.0, dt) == np.inf
    assert _err(T(1.0), np.nan, dt) == np.inf


def test_from_mp_keeps_64_bits():
    m = U._mp()
    v = [m.pi, -m.mpf(2) ** -1080, m.mpf(10) ** 400, m.mpf(0), m.mpf(1) / 3]
    got = U.from_mp(v, "f64")
    assert got.dtype == np.longdouble
    assert abs(got[0] - ld(np.pi) - ld(1.2246467991473532e-16)) < ld(2) ** -62
    assert got[1] == -ld(2.0) ** -1080 and got[3] == 0
    assert np.isfinite(got[2]) and got[2] > ld(1e308) * ld(1e90)
    assert abs(got[4] * 3 - 1) < ld(2.0) ** -62
    assert U.from_mp(v, "f32").dtype == np.float64


def test_vectors_shape_and_content():
    for dt in ("f64", "f32"):
        sp = U.specials(dt)
        assert np.isnan(sp).sum() == 2 and np.isinf(sp).sum() == 2
        assert (np.signbit(sp) & (sp == 0)).sum() == 1
        for op in ("sin", "exp", "log", "gamma", "asec", "erfinv"):
            x = U.vector(op, dt)
            assert len(x) % 4 == 3 and len(x) <= 1 << 15
            assert np.array_equal(x[:len(sp)], sp, equal_nan=True)
            assert np.array_equal(x[-len(sp):], sp, equal_nan=True)
    near, deep = U.pio2_table()
    assert near[0] == np.pi / 2 and len(near) == len(deep) == 4096
    assert 826882.8943881015 in deep and 413441.44719405076 in deep
    assert deep.max() < 1.0e6 and len(U.pio2_hard("deep")) % 4 == 3
    x = U.vector("sin", "f64")
    assert (np.abs(x) >= 1e6).sum() > 1000         # the OCML range
    a, b = U.grid2("f64")
    assert len(a) % 4 == 3 and len(a) <= 4096


def test_composite_reference_follows_the_rounded_intermediate():
    """sind(180) is sin(fl(180 * fl(pi/180))) = 1.22e-16, not 0."""
    x = np.array([180.0, 90.0, 30.0])
    ref = U.reference("sind", x, "f64", use_mp=True)
    u = x * (np.pi / 180.0)
    assert ref[0] != 0 and abs(float(ref[0]) - np.sin(u[0])) < 1e-30
    assert np.array_equal(U.host("sind", x), np.sin(u))
    assert U.POST_STEPS("sind") == 0 and U.POST_STEPS("asind") == 1
    assert U.bound("asind", "f64", 4.0) == 4.5 + U.REF_SLACK


CASES = [(op, dt) for dt in ("f64", "f32") for op in U.TRANSCENDENTAL]


@pytest.mark.parametrize("op,dt", CASES)
def test_host_libm_within_ceiling_and_fault_detected(op, dt):
    """Host libm/scipy through the same harness stays inside the ceiling
    the device is held to (so the reference, vectors and bound are
    satisfiable), the frozen ceiling is what rule (c) derives, and a result
    off by two nextafter steps in ONE element is rejected."""
    x = U.vector(op, dt)
    ref = U.reference_cached(op, dt)
    got = U.host(op, x)
    err = U.ulp_err(got, ref, dt)
    w, at = U.worst(err, x)
    limit = U.bound(op, dt, U.ceiling(op, dt))
    assert w <= limit, (op, dt, w, float(at))
    if (op, dt) not in U.OWNED:
        assert U.CEILINGS[(op, dt)] <= U.derive_ceiling(w) + 1, (op, dt, w)
    # plant the fault where the host is closest to the reference, away from
    # zeros, infinities and NaN
    ok = np.isfinite(got) & (got != 0) & np.isfinite(err)
    j = int(np.flatnonzero(ok)[np.argmin(err[ok])])
    bad = got.copy()
    away = np.inf if float(got[j]) >= float(ref[j]) else -np.inf
    for _ in range(2 + int(limit)):
        bad[j] = np.nextafter(bad[j], bad.dtype.type(away))
    assert U.ulp_err(bad, ref, dt)[j] > limit, (op, dt, x[j])
    two = got.copy()
    for _ in range(2):
        two[j] = np.nextafter(two[j], two.dtype.type(away))
    assert U.ulp_err(two, ref, dt)[j] >= 1.0
    if limit < 2:
        assert U.ulp_err(two, ref, dt)[j] > limit


@pytest.mark.parametrize("dt", ["f64", "f32"])
@pytest.mark.parametrize("op", ["pow", "atan2"])
def test_host_pow_atan2_within_ceiling(op, dt):
    w, at = U.host_worst2(op, dt)
    assert w <= U.bound(op, dt, U.ceiling(op, dt)), (op, dt, w, at)
    a, b = U.grid2(dt)
    h = U.host2(op, a, b)
    if op == "pow":     # the IEEE special cases are in the grid
        assert (h[(b == 0)] == 1).all()
        neg_frac = (a < 0) & np.isfinite(a) & np.isfinite(b) & \
            (b != np.rint(b))
        assert neg_frac.sum() > 50 and np.isnan(h[neg_frac]).all()
