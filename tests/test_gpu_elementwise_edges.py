"""Edges of every kernel_elementwise launcher at ABI level (world 1): all
lengths around a lane vector, a wave and a workgroup, one length that sends
a capped grid round its loop again, a sentinel guard after every
destination, every dtype each launcher accepts.  Default switches, so the
vector-of-4 kernels; tests/variant_child.py reruns the same routine under
DA_NT=1, DA_MAP_W=2 and DA_BC_W=2.  The checks are in
kernel_checks.check_elementwise_edges; everything is compared bit for bit
except the f64 normals (rtol = atol = 1e-12)."""
import pytest

import kernel_checks as kc

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dja():
    import distributedarrays_jl_amd as dja
    dja.comm.init()
    return dja


@pytest.fixture(autouse=True)
def no_leak(dja):
    before = dja.bytes_in_use()
    yield
    assert dja.bytes_in_use() == before


@pytest.mark.parametrize("family", kc.EDGE_FAMILIES)
def test_edges(dja, family):
    kc.check_elementwise_edges(dja, kc.EDGE_SIZES, None, families=(family,))


@pytest.mark.parametrize("family", [f for f in kc.EDGE_FAMILIES
                                    if f not in ("transpose", "diag_scale")])
def test_wrap(dja, family):
    kc.check_elementwise_edges(dja, (), kc.EDGE_WRAP, families=(family,))
