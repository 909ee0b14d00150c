"""Host side of da_scan, no GPU: the kernel-family selector at both sides
of each threshold, the argument checks (which run before the da_init
check and touch no memory), and the agreement of the header, the Python
binding and the INTEGRATION.md stub on the new names."""
import ctypes
import os
import re
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HDR = os.path.join(ROOT, "include", "darray_hip.h")

TILE = 2048          # SCAN_TILE: elements per tile, every dtype
BLOCK_LINES = 512    # SCAN_BLOCK_LINES: lines from which `block` is chosen


@pytest.fixture(scope="module")
def ffi():
    from distributedarrays_jl_amd import _ffi
    return _ffi


def variant(ffi, *shape):
    return ffi.SCAN_VARIANTS[ffi.lib.dbg_scan_variant(*shape)]


def test_selector_thresholds(ffi):
    # inner > 1 is always cols, whatever the rest
    for shape in [(2, 1, 1), (2, 1 << 27, 1), (64, 65, 3), (257, 2, 1),
                  (2, TILE + 1, 1), (2, 5, BLOCK_LINES), (1 << 20, 1, 1)]:
        assert variant(ffi, *shape) == "cols", shape
    # inner == 1: one workgroup per line while a line is at most one tile
    assert variant(ffi, 1, 1, 1) == "block"
    assert variant(ffi, 1, TILE - 1, 1) == "block"
    assert variant(ffi, 1, TILE, 1) == "block"
    assert variant(ffi, 1, TILE + 1, 1) == "spans"
    assert variant(ffi, 1, 1 << 28, 1) == "spans"
    # ... or when there are enough lines to fill the device
    assert variant(ffi, 1, TILE + 1, BLOCK_LINES - 1) == "spans"
    assert variant(ffi, 1, TILE + 1, BLOCK_LINES) == "block"
    assert variant(ffi, 1, 16384, 16384) == "block"
    assert variant(ffi, 1, TILE, BLOCK_LINES - 1) == "block"
    # empty views answer too (the launcher never sees them)
    assert variant(ffi, 1, 0, 1) in ffi.SCAN_VARIANTS
    assert variant(ffi, 0, 0, 0) in ffi.SCAN_VARIANTS


def _fresh():
    """The library handle.  Every call made through it here is rejected by
    the argument check, whether or not the library is initialised."""
    from distributedarrays_jl_amd import _ffi
    return _ffi.lib


def _err(lib, rc):
    return (lib.da_errstr(rc) or b"").decode()


@pytest.fixture()
def bufs():
    # real host memory behind the pointers: a check that did touch them
    # would read or write these bytes, not fault
    a = (ctypes.c_uint8 * 256)(*([0xA5] * 256))
    b = (ctypes.c_uint8 * 256)(*([0x5A] * 256))
    return a, b


# Calls that PASS the argument check must only ever meet the da_init
# check here (their pointers are host memory), so they run in a child
# process that certainly never initialised the library — in a whole-suite
# run on a GPU machine this process may have.
_CHILD_PRELUDE = """
import ctypes, sys
sys.path.insert(0, %r)
from distributedarrays_jl_amd import _ffi
lib = _ffi.lib
err = lambda rc: (lib.da_errstr(rc) or b'').decode()
a = (ctypes.c_uint8 * 256)(*([0xA5] * 256))
b = (ctypes.c_uint8 * 256)(*([0x5A] * 256))
pa, pb = ctypes.addressof(a), ctypes.addressof(b)
assert lib.da_synchronize() < 0
""" % ROOT
_CHILD_EPILOGUE = """
assert bytes(a) == b'\\xa5' * 256 and bytes(b) == b'\\x5a' * 256
print('child ok')
"""


def _child(body):
    r = subprocess.run([sys.executable, "-c",
                        _CHILD_PRELUDE + body + _CHILD_EPILOGUE],
                       capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "child ok" in r.stdout, \
        r.stdout[-1000:] + r.stderr[-3000:]


def test_scan_before_init_names_da_init():
    _child("""
rc = lib.da_scan(0, pa, pb, 1, 4, 1, 0, None)
assert rc < 0 and 'da_init' in err(rc), err(rc)
# in place and with a carry: still only the init check objects
rc = lib.da_scan(3, pa, pa, 2, 4, 2, 1, pb)
assert rc < 0 and 'da_init' in err(rc), err(rc)
# an empty view is judged by the same entry check
rc = lib.da_scan(0, None, None, 1, 0, 1, 0, None)
assert rc < 0 and 'da_init' in err(rc), err(rc)
# abutting dst / src and dst / carry are no overlap
rc = lib.da_scan(0, pa, pa + 32, 1, 4, 1, 0, None)
assert rc < 0 and 'da_init' in err(rc), err(rc)
rc = lib.da_scan(0, pa, pb, 2, 4, 2, 1, pa + 64)
assert rc < 0 and 'da_init' in err(rc), err(rc)
""")


@pytest.mark.parametrize("args,word", [
    ((4, 1, 4, 1, 0), "redop"),
    ((-1, 1, 4, 1, 0), "redop"),
    ((0, 1, 4, 1, 3), "dtype"),
    ((0, 1, 4, 1, -1), "dtype"),
    ((0, 1 << 32, 1 << 32, 1, 0), "overflow"),
    ((0, 1 << 21, 1 << 21, 1 << 22, 0), "overflow"),
    ((0, 1, 1 << 62, 1, 2), "overflow"),        # the byte count overflows
])
def test_bad_arguments_rejected_without_touching_memory(ffi, bufs, args,
                                                        word):
    lib = _fresh()
    a, b = bufs
    redop, inner, axis, outer, dtype = args
    rc = lib.da_scan(redop, ctypes.addressof(a), ctypes.addressof(b), inner,
                     axis, outer, dtype, None)
    assert rc < 0
    msg = _err(lib, rc)
    assert "da_scan" in msg and word in msg, msg
    assert "da_init" not in msg
    assert bytes(a) == b"\xa5" * 256 and bytes(b) == b"\x5a" * 256


def test_null_and_overlap_rejected(ffi, bufs):
    lib = _fresh()
    a, b = bufs
    pa, pb = ctypes.addressof(a), ctypes.addressof(b)
    rc = lib.da_scan(0, None, pb, 1, 4, 1, 0, None)
    assert rc < 0 and "null" in _err(lib, rc)
    rc = lib.da_scan(0, pa, None, 1, 4, 1, 0, None)
    assert rc < 0 and "null" in _err(lib, rc)
    # dst one element into src
    rc = lib.da_scan(0, pa + 8, pa, 1, 4, 1, 0, None)
    assert rc < 0 and "overlaps src" in _err(lib, rc)
    rc = lib.da_scan(0, pa, pa + 24, 1, 4, 1, 0, None)
    assert rc < 0 and "overlaps src" in _err(lib, rc)
    # carry (inner*outer elements) inside dst
    rc = lib.da_scan(0, pa, pb, 2, 4, 2, 1, pa + 60)
    assert rc < 0 and "overlaps carry" in _err(lib, rc)
    assert bytes(a) == b"\xa5" * 256 and bytes(b) == b"\x5a" * 256


def test_names_agree(ffi):
    txt = open(HDR).read()
    m = re.search(r"enum da_scan_variant \{(.*?)\};", txt, re.S)
    assert m, "enum da_scan_variant missing from the header"
    names = re.findall(r"DA_SCAN_(\w+)", m.group(1))
    assert tuple(n.lower() for n in names) == ffi.SCAN_VARIANTS
    assert re.search(r"^int\s+da_scan\s*\(", txt, re.M)
    assert re.search(r"\bint\s+dbg_scan_variant\s*\(", txt)
    assert "da_scan" in ffi._sigs
    assert hasattr(ffi.lib, "da_scan") and hasattr(ffi.lib,
                                                   "dbg_scan_variant")
    # the header's parameter count is the binding's
    proto = re.search(r"^int\s+da_scan\s*\((.*?)\);", txt, re.M | re.S)
    assert len(proto.group(1).split(",")) == len(ffi._sigs["da_scan"][0])
    integ = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    assert ":da_scan" in integ and ":dbg_scan_variant" in integ
    for k, n in enumerate(names):
        assert "%d = DA_SCAN_%s" % (k, n) in integ
    stub = re.search(r"\(:da_scan, libdarray\), Cint,\s*\((.*?)\)", integ,
                     re.S)
    assert len(stub.group(1).split(",")) == len(ffi._sigs["da_scan"][0])


def test_python_api_exported():
    import distributedarrays_jl_amd as dja
    for name in ("daccumulate", "daccumulate_", "dcumsum", "dcumprod",
                 "dcummax", "dcummin"):
        assert name in dja.__all__ and callable(getattr(dja, name))
