"""The flat mapreduce tree (stage 1 -> block tree -> cross-block fold)
with data that cannot pass by accident: sentinels and NaNs planted on
wave/block edges, in the last block and in the scalar tail; a sequence
whose wrapped sum changes if any element is dropped or read twice; and
predicate counts above 2^24, which a float accumulator cannot represent."""
import ctypes

import numpy as np
import pytest

import kernel_checks as kc
import kernel_ref as kr

pytestmark = pytest.mark.gpu

COUNT_N = (1 << 24) + 3


@pytest.fixture(scope="module")
def dja():
    import distributedarrays_jl_amd as dja
    dja.comm.init()
    return dja


@pytest.mark.parametrize("dt", ["f64", "f32", "i64"])
def test_planted_extrema(dja, dt):
    kc.check_planted_extrema(dja, dt, kc.TREE_N)


@pytest.mark.parametrize("dt", ["f64", "f32"])
def test_planted_nan(dja, dt):
    kc.check_planted_nan(dja, dt, kc.TREE_N)


@pytest.mark.parametrize("n", [255, 256, 257, 511, 513, kc.TREE_N])
def test_each_element_contributes_once(dja, n):
    kc.check_once_only(dja, n)


def _exact_counts(dja, dt):
    n = COUNT_N
    d = dja.distribute(np.ones(n, dtype=kr.NP[dt]))
    try:
        got = (dja.dcount("nonzero", d), dja.dcount("isfinite", d),
               dja.dnorm(d, 0))
        print("%s counts of %d ones: %r" % (dt, n, got))
        assert got[0] == n and isinstance(got[0], int)
        assert got[1] == n
        assert got[2] == float(n) and isinstance(got[2], float)
        kc.poke(d, 5, np.nan)
        kc.poke(d, n - 1, np.nan)      # the scalar tail
        kc.poke(d, n // 2, 0.0)
        got = (dja.dcount("isnan", d), dja.dcount("nonzero", d),
               dja.dcount("isfinite", d))
        print("%s counts after planting: %r" % (dt, got))
        assert got == (2, n - 1, n - 2)
    finally:
        d.close()


def test_exact_counts_f32(dja):
    """2^24+3 ones in f32: a float accumulator returns a multiple of 2 or 4
    (the float-accumulated mapreduce("nonzero", "add") path that dcount
    used before da_count measures 16777220 on an MI355X); the count must be
    the exact integer 16777219."""
    _exact_counts(dja, "f32")


def test_exact_counts_f64_control(dja):
    _exact_counts(dja, "f64")


def test_count_i64_and_small_sizes(dja):
    x = kr.small_ints(100001, 9, 8)
    d = dja.distribute(x)
    assert dja.dcount("nonzero", d) == int(np.count_nonzero(x))
    assert dja.dcount("isfinite", d) == x.size
    assert dja.dcount("isnan", d) == 0
    d.close()
    for n in (1, 2, 3, 257):
        y = np.zeros(n, dtype=np.float32)
        y[n - 1] = np.inf
        d = dja.distribute(y)
        assert dja.dcount("nonzero", d) == 1
        assert dja.dcount("isfinite", d) == n - 1
        d.close()


def test_da_count_rejects_non_predicates(dja):
    from distributedarrays_jl_amd._ffi import lib, DArrayError
    buf = kr.Dev.of(np.ones(16))
    out = ctypes.c_int64(-5)
    try:
        for f in ("identity", "abs", "abs2"):
            assert lib.da_count(kr.MAPOP[f], buf.p, 16, kr.DT["f64"],
                                ctypes.byref(out)) < 0
        assert out.value == -5
        assert lib.da_count(kr.MAPOP["nonzero"], buf.p, 0, kr.DT["f64"],
                            ctypes.byref(out)) == 0
        assert out.value == 0          # empty chunk counts zero
        with pytest.raises(DArrayError):
            d = dja.distribute(np.ones(4))
            try:
                dja.dcount("abs", d)
            finally:
                d.close()
    finally:
        buf.free()
