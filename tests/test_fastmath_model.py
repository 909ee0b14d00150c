"""The numpy model of csrc/fastmath.hpp (tests/fastmath_model.py) against
mpmath: <= 1 ulp of the true value on the sweep, on the doubles nearest
multiples of pi/2 and on the switch points.  No GPU: the device is tied to
the model bit for bit in test_gpu_math_ulp.py.

The two negative tests rebuild the defects this file was written to catch
and require that the same check rejects them."""
import os
import re

import numpy as np
import pytest

import fastmath_model as fm
import ulp_ref as U

_HPP = os.path.join(os.path.dirname(os.path.abspath(__file__)), os.pardir,
                    "distributedarrays_jl_amd", "csrc", "fastmath.hpp")


def _fast(op):
    x = U.vector(op, "f64")
    keep = fm.fast_range(op, x)
    return x[keep], U.reference_cached(op, "f64")[keep]


def _hard(op, which):
    x = U.pio2_hard(which)
    x = x[x > 0]
    return x, U.reference(op, x, "f64", use_mp=True)


@pytest.mark.parametrize("op", ["sin", "cos", "exp"])
def test_model_one_ulp_on_sweep_and_switch_points(op):
    x, ref = _fast(op)
    # the switch points are in the vector, on both sides
    for c in (0.7853981633974483, 0.3, 0.78125, 2.0 ** -27, 2.0 ** -28):
        for v in (c, np.nextafter(c, 0), np.nextafter(c, 1), -c):
            assert v in x
    assert (x < 0).sum() > 1000 and (np.abs(x) > 1e5).sum() > 100 \
        or op == "exp"
    w, at = U.worst(U.ulp_err(fm.MODEL[op](x), ref, "f64"), x)
    print("model %s: worst %.4f ulp at %r" % (op, w, float(at)))
    assert w <= 1.0 + U.REF_SLACK, (op, w, float(at))


@pytest.mark.parametrize("which", ["near", "deep"])
@pytest.mark.parametrize("op", ["sin", "cos"])
def test_model_one_ulp_near_multiples_of_half_pi(op, which):
    x, ref = _hard(op, which)
    for sign in (1.0, -1.0):     # sin odd, cos even: exact symmetries
        r = ref * sign if op == "sin" else ref
        w, at = U.worst(U.ulp_err(fm.MODEL[op](sign * x), r, "f64"), x)
        print("model %s %s: worst %.4f ulp at %r" % (op, which, w, at))
        assert w <= 1.0 + U.REF_SLACK, (op, which, w, float(at))


def test_check_rejects_untruncated_qx():
    """k_cos with all 53 bits of |x|/4 kept (the earlier revision): 1 - qx
    rounds and cos exceeds 1 ulp, already on (0.3, pi/4]."""
    x, ref = _fast("cos")
    small = (np.abs(x) > 0.3) & (np.abs(x) <= fm.PIO4)
    old = U.ulp_err(fm.fast_cos(x, truncate_qx=False), ref, "f64")
    new = U.ulp_err(fm.fast_cos(x), ref, "f64")
    assert old[small].max() > 1.0 + U.REF_SLACK
    assert new[small].max() <= 1.0
    xs, rs = _fast("sin")        # sin uses k_cos in quadrants 1 and 3
    assert U.ulp_err(fm.fast_sin(xs, truncate_qx=False), rs,
                     "f64").max() > 1.0 + U.REF_SLACK


def test_check_rejects_two_step_reduction():
    """Without the third Cody-Waite step both functions exceed 1 ulp at the
    doubles closest to a multiple of pi/2."""
    for op, at in (("sin", 826882.8943881015), ("cos", 413441.44719405076)):
        x, ref = _hard(op, "deep")
        assert at in x
        old = U.ulp_err(fm.MODEL[op](x, third_step=False), ref, "f64")
        assert old.max() > 1.0 + U.REF_SLACK, op
        j = int(np.flatnonzero(x == at)[0])
        assert old[j] > 1.0 and \
            U.ulp_err(fm.MODEL[op](x), ref, "f64")[j] <= 0.5 + U.REF_SLACK


def test_model_carries_the_header_constants():
    """Every floating constant of fastmath.hpp appears, digit for digit,
    in the model, and the two fdlibm details are in the header."""
    hpp = open(_HPP).read()
    model = open(fm.__file__).read()
    consts = re.findall(r"const double \w+ = (-?[0-9.]+e[-+][0-9]+);", hpp)
    assert len(consts) >= 25
    for c in consts:
        assert c in model, c
    for lit in ("0.7853981633974483", "7.450580596923828e-09",
                "3.725290298461914e-09", "562949953421312.0", "0.78125",
                "0.28125", "1.0e6", "708.0"):
        assert lit in hpp and lit in model, lit
    assert "__double2hiint(0.25 * ax)" in hpp      # qx cut to its high word
    assert "pio2_3t" in hpp                        # third reduction step


# ------------------------------------------- the header itself, on the host
_SHIM = r"""
#include <math.h>
#include <string.h>
#define __device__
#define __forceinline__ inline
static inline int __double2hiint(double d) {
    long long b; memcpy(&b, &d, 8); return (int)(b >> 32);
}
static inline double __hiloint2double(int hi, int lo) {
    unsigned long long b = ((unsigned long long)(unsigned)hi << 32)
                           | (unsigned)lo;
    double d; memcpy(&d, &b, 8); return d;
}
#include "fastmath.hpp"
extern "C" void fm_apply(int op, const double* x, double* y, long n) {
    for (long i = 0; i < n; ++i)
        y[i] = op == 0 ? da::fm::fast_sin(x[i])
             : op == 1 ? da::fm::fast_cos(x[i]) : da::fm::fast_exp(x[i]);
}
"""


@pytest.fixture(scope="module")
def host_header(tmp_path_factory):
    """fastmath.hpp compiled for the host CPU, contraction off as in the
    device build: the same IEEE operations in the same order."""
    import ctypes
    import shutil
    import subprocess
    cxx = shutil.which("c++") or shutil.which("g++") or \
        shutil.which("clang++")
    assert cxx, "no host C++ compiler"
    d = tmp_path_factory.mktemp("fm_host")
    (d / "shim.cpp").write_text(_SHIM)
    so = str(d / "fm_host.so")
    subprocess.run([cxx, "-O2", "-std=c++17", "-ffp-contract=off", "-shared",
                    "-fPIC", "-I", os.path.dirname(_HPP),
                    str(d / "shim.cpp"), "-o", so, "-lm"], check=True)
    lib = ctypes.CDLL(so)

    def apply(op, x):
        x = np.ascontiguousarray(x, dtype=np.float64)
        y = np.empty_like(x)
        lib.fm_apply(["sin", "cos", "exp"].index(op),
                     x.ctypes.data_as(ctypes.c_void_p),
                     y.ctypes.data_as(ctypes.c_void_p),
                     ctypes.c_long(x.size))
        return y
    return apply


@pytest.mark.parametrize("op", ["sin", "cos", "exp"])
def test_header_on_host_is_the_model_and_within_one_ulp(host_header, op):
    """The header's own text, run on the CPU, gives the model's bits and
    stays <= 1 ulp; this is the case that fails on a k_cos whose qx keeps
    all its bits or a reduction without the third step."""
    sets = [_fast(op)]
    if op != "exp":
        sets += [_hard(op, "near"), _hard(op, "deep")]
    for x, ref in sets:
        got = host_header(op, x)
        w, at = U.worst(U.ulp_err(got, ref, "f64"), x)
        assert w <= 1.0 + U.REF_SLACK, (op, w, float(at))
        assert np.array_equal(got.view(np.uint64),
                              fm.MODEL[op](x).view(np.uint64)), op
