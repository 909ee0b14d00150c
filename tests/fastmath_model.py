"""numpy restatement of csrc/fastmath.hpp, operation for operation.

The device code is built with -ffp-contract=off and every step of
fast_sin/fast_cos/fast_exp is a single IEEE-754 double operation
(+, -, *, /, rint, fabs, ldexp, a bit mask), so the same sequence in numpy
float64 yields the same bits on the CPU.  tests/test_fastmath_model.py
holds this model to <= 1 ulp against mpmath; tests/test_gpu_math_ulp.py
holds the device to the model bit for bit.  Keep the two files in step:
a change to fastmath.hpp is restated here, constant for constant.

`truncate_qx` and `third_step` switch off the two fdlibm details whose
absence made earlier revisions exceed 1 ulp; the tests use them to show
that the checks would have caught it.

Only the fast range is modelled: |x| < 1e6 for sin/cos, |x| < 708 for exp.
fast_range(op, x) gives the mask; outside it the device calls OCML.
"""
import numpy as np

PIO4 = 0.7853981633974483
SIN_TINY = 7.450580596923828e-09      # 2^-27
EXP_TINY = 3.725290298461914e-09      # 2^-28
SINCOS_MAX = 1.0e6
EXP_MAX = 708.0

_S = (-1.66666666666666324348e-01, 8.33333333332248946124e-03,
      -1.98412698298579493134e-04, 2.75573137070700676789e-06,
      -2.50507602534068634195e-08, 1.58969099521155010221e-10)
_C = (4.16666666666666019037e-02, -1.38888888888741095749e-03,
      2.48015872894767294178e-05, -2.75573143513906633035e-07,
      2.08757232129817482790e-09, -1.13596475577881948265e-11)
_HI_MASK = np.uint64(0xFFFFFFFF00000000)


def _f64(x):
    return np.ascontiguousarray(x, dtype=np.float64)


def k_sin(x, y, iy):
    S1, S2, S3, S4, S5, S6 = _S
    z = x * x
    w = z * z
    r = S2 + z * (S3 + z * S4) + z * w * (S5 + z * S6)
    v = z * x
    if iy == 0:
        return x + v * (S1 + z * r)
    return x - ((z * (0.5 * y - v * r) - y) - v * S1)


def k_cos(x, y, truncate_qx=True):
    C1, C2, C3, C4, C5, C6 = _C
    z = x * x
    r = z * (C1 + z * (C2 + z * (C3 + z * (C4 + z * (C5 + z * C6)))))
    ax = np.abs(x)
    q = 0.25 * ax
    if truncate_qx:
        q = (q.view(np.uint64) & _HI_MASK).view(np.float64)
    qx = np.where(ax > 0.3, np.where(ax > 0.78125, 0.28125, q), 0.0)
    hz = 0.5 * z - qx
    a = 1.0 - qx
    return a - (hz - (z * r - x * y))


def rem_pio2_medium(x, third_step=True):
    """(y0, y1, n & 3) for pi/4 < |x| < 1e6."""
    invpio2 = 6.36619772367581382433e-01
    pio2_1 = 1.57079632673412561417e+00
    pio2_2 = 6.07710050630396597660e-11
    pio2_2t = 2.02226624879595063154e-21
    pio2_3 = 2.02226624871116645580e-21
    pio2_3t = 8.47842766036889956997e-32
    fn = np.rint(x * invpio2)
    t = x - fn * pio2_1
    w = fn * pio2_2
    r = t - w
    w = fn * pio2_2t - ((t - r) - w)
    y0 = r - w
    if third_step:
        deep = np.abs(y0) * 562949953421312.0 < np.abs(x)
        t3 = r
        w3 = fn * pio2_3
        r3 = t3 - w3
        w3 = fn * pio2_3t - ((t3 - r3) - w3)
        r = np.where(deep, r3, r)
        w = np.where(deep, w3, w)
        y0 = np.where(deep, r3 - w3, y0)
    y1 = (r - y0) - w
    return y0, y1, fn.astype(np.int64) & 3


def fast_range(op, x):
    ax = np.abs(_f64(x))
    return ax < (EXP_MAX if op == "exp" else SINCOS_MAX)


def _sincos(x, quadrant_shift, **kw):
    x = _f64(x)
    kc = {k: v for k, v in kw.items() if k == "truncate_qx"}
    kr = {k: v for k, v in kw.items() if k == "third_step"}
    ax = np.abs(x)
    out = np.empty_like(x)
    small = ax <= PIO4
    xs = x[small]
    with np.errstate(all="ignore"):
        if quadrant_shift == 0:
            out[small] = np.where(np.abs(xs) < SIN_TINY, xs,
                                  k_sin(xs, 0.0, 0))
        else:
            out[small] = k_cos(xs, np.zeros_like(xs), **kc)
        med = ~small
        xm = x[med]
        assert (np.abs(xm) < SINCOS_MAX).all(), "outside the fast range"
        y0, y1, n = rem_pio2_medium(xm, **kr)
        n = (n + quadrant_shift) & 3
        s = k_sin(y0, y1, 1)
        c = k_cos(y0, y1, **kc)
        out[med] = np.select([n == 0, n == 1, n == 2], [s, c, -s], -c)
    return out


def fast_sin(x, **kw):
    return _sincos(x, 0, **kw)


def fast_cos(x, **kw):
    # cos x = sin(x + pi/2): quadrant n of cos is quadrant n+1 of sin
    return _sincos(x, 1, **kw)


def fast_exp(x):
    x = _f64(x)
    assert (np.abs(x) < EXP_MAX).all(), "outside the fast range"
    invln2 = 1.44269504088896338700e+00
    ln2HI = 6.93147180369123816490e-01
    ln2LO = 1.90821492927058770002e-10
    P1 = 1.66666666666666019037e-01
    P2 = -2.77777777770155933842e-03
    P3 = 6.61375632143793436117e-05
    P4 = -1.65339022054652515390e-06
    P5 = 4.13813679705723846039e-08
    with np.errstate(all="ignore"):
        fn = np.rint(x * invln2)
        k = fn.astype(np.int32)
        hi = x - fn * ln2HI
        lo = fn * ln2LO
        xr = hi - lo
        t = xr * xr
        c = xr - t * (P1 + t * (P2 + t * (P3 + t * (P4 + t * P5))))
        y = 1.0 - ((lo - (xr * c) / (2.0 - c)) - hi)
        big = np.ldexp(y, k)
        return np.where(np.abs(x) < EXP_TINY, 1.0 + x, big)


MODEL = {"sin": fast_sin, "cos": fast_cos, "exp": fast_exp}
