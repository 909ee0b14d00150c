"""Host side of da_expr_reduce_dims, no GPU: the schedule selector at both
sides of each threshold and on empty shapes, the argument checks (which run
before the da_init check and touch no memory), the hipRTC codegen of every
dtype x schedule x fold, and the agreement of the header, the Python binding
and the INTEGRATION.md stub on the new names."""
import ctypes
import os
import re
import subprocess
import sys

import pytest

from distributedarrays_jl_amd._opcodes import MAP_OP, MAP2_OP

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HDR = os.path.join(ROOT, "include", "darray_hip.h")

BLOCK_R = 512        # EDIMS_BLOCK_R: shortest fold a workgroup takes
SPLIT_BLOCKS = 1024  # EDIMS_SPLIT_BLOCKS: split while fewer workgroups
MAXBLOCKS = 4096     # EDIMS_MAXBLOCKS: gridDim.x cap
COUNT = -1           # DA_EXPR_COUNT


@pytest.fixture(scope="module")
def ffi():
    from distributedarrays_jl_amd import _ffi
    return _ffi


def variant(ffi, shape, dims):
    """(schedule name, slices, gridDim.x) for a chunk shape and reduced
    dims."""
    arr = (ctypes.c_uint64 * len(shape))(*shape)
    mask = sum(1 << a for a in dims)
    nb, gx = ctypes.c_uint32(77), ctypes.c_uint32(77)
    rc = ffi.lib.dbg_expr_dims_variant(arr, len(shape), mask,
                                       ctypes.byref(nb), ctypes.byref(gx))
    assert rc >= 0, (shape, dims, rc)
    return ffi.EXPR_DIMS_VARIANTS[rc], nb.value, gx.value


def test_schedule_follows_the_leading_dimension(ffi):
    # leading dimension kept: a thread per output
    assert variant(ffi, (33, 7), (1,)) == ("lanes", 1, 1)
    assert variant(ffi, (5, 4, 3), (1, 2)) == ("lanes", 1, 1)
    assert variant(ffi, (5, 4, 3), (1,)) == ("lanes", 1, 1)
    assert variant(ffi, (33, 7), ()) == ("lanes", 1, 1)
    # leading dimension reduced: a wave per output below BLOCK_R terms
    assert variant(ffi, (33, 7), (0,)) == ("wave", 1, 2)
    assert variant(ffi, (33, 7), (0, 1)) == ("wave", 1, 1)
    assert variant(ffi, (5, 4, 3), (0, 2)) == ("wave", 1, 1)
    assert variant(ffi, (3, 2, 5, 4), (1, 3)) == ("lanes", 1, 1)
    # extents of 1 do not lead
    assert variant(ffi, (1, 33, 7), (1,)) == ("wave", 1, 2)
    assert variant(ffi, (1, 33, 7), (0,)) == ("lanes", 1, 1)
    assert variant(ffi, (1, 33, 7), (0, 2)) == ("lanes", 1, 1)
    assert variant(ffi, (1, 1), (0,)) == ("lanes", 1, 1)
    # wave / block
    assert variant(ffi, (BLOCK_R - 1, 3), (0,)) == ("wave", 1, 1)
    assert variant(ffi, (BLOCK_R, 3), (0,)) == ("block", 1, 3)
    assert variant(ffi, (16, BLOCK_R // 16, 3), (0, 1)) == ("block", 1, 3)
    assert variant(ffi, (16, 3, BLOCK_R // 16), (0, 2))[0] == "block"
    assert variant(ffi, (257, 3), (0,)) == ("wave", 1, 1)
    assert variant(ffi, (3, 257), (1,)) == ("lanes", 29, 1)


def test_split_thresholds(ffi):
    # lanes: slices of at least 8 terms while K gives fewer than
    # SPLIT_BLOCKS workgroups of 256 outputs
    assert variant(ffi, (256, 15), (1,)) == ("lanes", 1, 1)
    assert variant(ffi, (256, 16), (1,)) == ("lanes", 2, 1)
    assert variant(ffi, (256, 8 * 1024), (1,)) == ("lanes", 1024, 1)
    assert variant(ffi, (256, 8 * 4096), (1,)) == ("lanes", 1024, 1)
    half = 256 * SPLIT_BLOCKS // 2
    assert variant(ffi, (half, 16), (1,)) == ("lanes", 2, 512)
    assert variant(ffi, (half + 1, 16), (1,)) == ("lanes", 1, 513)
    # slices are re-counted from the rounded-up slice length: none is empty
    assert variant(ffi, (3, 257), (1,)) == ("lanes", 29, 1)   # 9 terms each
    assert variant(ffi, (256, 17), (1,)) == ("lanes", 2, 1)
    # block: slices of at least 1024 terms, K workgroups
    assert variant(ffi, (2047, 2), (0,)) == ("block", 1, 2)
    assert variant(ffi, (2048, 2), (0,)) == ("block", 2, 2)
    assert variant(ffi, (2048, SPLIT_BLOCKS // 2), (0,)) == ("block", 2, 512)
    assert variant(ffi, (2048, SPLIT_BLOCKS // 2 + 1), (0,)) == \
        ("block", 1, 513)
    assert variant(ffi, (1 << 20,), (0,)) == ("block", 1024, 1)
    # wave never splits: under BLOCK_R terms there is nothing to cut
    assert variant(ffi, (BLOCK_R - 1,), (0,)) == ("wave", 1, 1)


def test_grid_cap(ffi):
    assert variant(ffi, (256 * MAXBLOCKS, 2), (1,)) == \
        ("lanes", 1, MAXBLOCKS)
    assert variant(ffi, (256 * MAXBLOCKS + 1, 2), (1,)) == \
        ("lanes", 1, MAXBLOCKS)
    assert variant(ffi, (256 * MAXBLOCKS - 256, 2), (1,)) == \
        ("lanes", 1, MAXBLOCKS - 1)
    assert variant(ffi, (2, 4 * MAXBLOCKS), (0,)) == ("wave", 1, MAXBLOCKS)
    assert variant(ffi, (2, 4 * MAXBLOCKS + 1), (0,)) == \
        ("wave", 1, MAXBLOCKS)
    assert variant(ffi, (2, 4 * MAXBLOCKS - 4), (0,)) == \
        ("wave", 1, MAXBLOCKS - 1)
    assert variant(ffi, (BLOCK_R, MAXBLOCKS - 1), (0,)) == \
        ("block", 1, MAXBLOCKS - 1)
    assert variant(ffi, (BLOCK_R, MAXBLOCKS + 1), (0,)) == \
        ("block", 1, MAXBLOCKS)


def test_empty_shapes(ffi):
    # no outputs / no terms: nothing to schedule (nb == 0, gx == 0)
    assert variant(ffi, (0, 4), (0,)) == ("lanes", 0, 0)
    assert variant(ffi, (0, 4), (1,)) == ("lanes", 0, 0)
    assert variant(ffi, (5, 0, 3), (1,)) == ("lanes", 0, 0)
    assert variant(ffi, (0,), (0,)) == ("lanes", 0, 0)
    assert variant(ffi, (0,), ()) == ("lanes", 0, 0)


def _err(lib, rc):
    return (lib.da_errstr(rc) or b"").decode()


def test_selector_rejects_bad_shapes(ffi):
    lib = ffi.lib
    one = (ctypes.c_uint64 * 4)(2, 2, 2, 2)
    for nd, mask, word in ((0, 0, "nd"), (5, 0, "nd"), (-1, 0, "nd"),
                           (2, 4, "mask"), (1, 2, "mask"), (4, 16, "mask")):
        rc = lib.dbg_expr_dims_variant(one, nd, mask, None, None)
        assert rc < 0 and word in _err(lib, rc), (nd, mask, _err(lib, rc))
    rc = lib.dbg_expr_dims_variant(None, 2, 1, None, None)
    assert rc < 0 and "null" in _err(lib, rc)
    # 2^32 elements and more: the 32-bit index decode does not reach them
    for shape in ((1 << 32,), (1 << 16, 1 << 16), (1 << 31, 2),
                  (1 << 40, 1), (3, 1 << 31)):
        arr = (ctypes.c_uint64 * len(shape))(*shape)
        for mask in (0, 1):
            rc = lib.dbg_expr_dims_variant(arr, len(shape), mask, None, None)
            assert rc < 0 and "2^32" in _err(lib, rc), shape
    arr = (ctypes.c_uint64 * 2)((1 << 16) - 1, (1 << 16) + 1)
    assert lib.dbg_expr_dims_variant(arr, 2, 1, None, None) >= 0


# ------------------------------------------------------- argument checks
PROG = [(1 << 8) | 0, (1 << 8) | 1, (3 << 8) | MAP2_OP["sub"],
        (0 << 8) | MAP_OP["abs2"]]
IPROG = [(1 << 8) | 0, (0 << 8) | MAP_OP["abs"], (2 << 8) | 0,
         (3 << 8) | MAP2_OP["mul"], (1 << 8) | 1, (3 << 8) | MAP2_OP["add"]]


class Call:
    """A well-formed da_expr_reduce_dims call over host memory; tests break
    one argument at a time."""

    def __init__(self):
        self.a = (ctypes.c_uint8 * 256)(*([0xA5] * 256))
        self.b = (ctypes.c_uint8 * 256)(*([0x5A] * 256))
        self.prog = (ctypes.c_int32 * len(PROG))(*PROG)
        self.kw = dict(
            prog=self.prog, plen=len(PROG),
            dims=(ctypes.c_uint64 * 2)(4, 4), nd=2,
            srcs=(ctypes.c_void_p * 2)(ctypes.addressof(self.a),
                                       ctypes.addressof(self.a) + 128),
            strides=None, nsrcs=2, consts=(ctypes.c_double * 1)(0.0),
            nconsts=0, dtype=0, mask=1, redop=0,
            dst=ctypes.addressof(self.b))

    def run(self, lib, **over):
        k = dict(self.kw, **over)
        return lib.da_expr_reduce_dims(
            k["prog"], k["plen"], k["dims"], k["nd"], k["srcs"],
            k["strides"], k["nsrcs"], k["consts"], k["nconsts"], k["dtype"],
            k["mask"], k["redop"], k["dst"])

    def untouched(self):
        return bytes(self.a) == b"\xa5" * 256 and \
            bytes(self.b) == b"\x5a" * 256


@pytest.mark.parametrize("over,word", [
    (dict(mask=4), "mask"),
    (dict(mask=0xffffffff), "mask"),
    (dict(nd=0), "nd"),
    (dict(nd=5), "nd"),
    (dict(redop=4), "redop"),
    (dict(redop=-2), "redop"),
    (dict(dtype=3), "dtype"),
    (dict(dtype=-1), "dtype"),
    (dict(prog=None), "null"),
    (dict(dims=None), "null"),
    (dict(srcs=None), "null"),
    (dict(dst=None), "null"),
    (dict(consts=None, nconsts=1), "null"),
    (dict(plen=0), "program length"),
    (dict(plen=2), "leaves"),
    (dict(nsrcs=1), "oob"),
    (dict(nsrcs=7), "too many"),
    (dict(dims=(ctypes.c_uint64 * 2)(1 << 16, 1 << 16)), "2^32"),
    (dict(strides=(ctypes.c_uint64 * 4)(1, 4, 1 << 32, 0)), "stride"),
])
def test_bad_arguments_rejected_without_touching_memory(ffi, over, word):
    lib = ffi.lib
    c = Call()
    rc = c.run(lib, **over)
    assert rc < 0
    msg = _err(lib, rc)
    assert "da_expr_reduce_dims" in msg and word in msg, msg
    assert "da_init" not in msg
    assert c.untouched()


def test_count_and_every_fold_pass_the_check_then_need_init():
    """Calls that pass the argument check meet only the da_init check; they
    run in a child that certainly never initialised the library."""
    body = """
import ctypes, sys
sys.path.insert(0, %r)
sys.path.insert(0, %r)
from distributedarrays_jl_amd import _ffi
import test_expr_dims_host as t
lib = _ffi.lib
assert lib.da_synchronize() < 0
c = t.Call()
for redop in (-1, 0, 1, 2, 3):
    for dtype in (0, 1, 2):
        for mask in (0, 1, 2, 3):
            rc = c.run(lib, redop=redop, dtype=dtype, mask=mask)
            assert rc < 0 and 'da_init' in t._err(lib, rc), t._err(lib, rc)
# no outputs: the destination may be null, still only the init check
rc = c.run(lib, dims=(ctypes.c_uint64 * 2)(4, 0), dst=None)
assert rc < 0 and 'da_init' in t._err(lib, rc), t._err(lib, rc)
# the size limit is judged before the program could reach the JIT
rc = c.run(lib, dims=(ctypes.c_uint64 * 2)(1 << 31, 2))
assert rc < 0 and '2^32' in t._err(lib, rc)
assert c.untouched()
print('child ok')
""" % (ROOT, os.path.join(ROOT, "tests"))
    r = subprocess.run([sys.executable, "-c", body], capture_output=True,
                       text=True, timeout=120)
    assert r.returncode == 0 and "child ok" in r.stdout, \
        r.stdout[-1000:] + r.stderr[-3000:]


# ----------------------------------------------------------------- codegen
@pytest.mark.parametrize("dtype", [0, 1, 2])
def test_dims_codegen_compiles(ffi, dtype):
    """hipRTC is a pure compiler: every schedule x fold (and the count) of
    each dtype generates source it accepts, with no GPU; the fold, the
    schedule and the dimension counts are constants of the source."""
    lib = ffi.lib
    dbg = lib.dbg_expr_dims_jit_compile
    dbg.argtypes = [ctypes.POINTER(ctypes.c_int32)] + [ctypes.c_int] * 7 + \
        [ctypes.c_char_p, ctypes.c_int]
    dbg.restype = ctypes.c_int
    p = IPROG if dtype == 2 else PROG
    arr = (ctypes.c_int32 * len(p))(*p)
    src = ctypes.create_string_buffer(16384)
    seen = set()
    for sched in (0, 1, 2):
        for rop in (0, 1, 2, 3, COUNT):
            for nk, nr in ((1, 1), (0, 4), (2, 2)):
                rc = dbg(arr, len(p), dtype, 2, rop, sched, nk, nr, src,
                         16384)
                assert rc == 0, "dtype %d sched %d redop %d: %r\n%s" % (
                    dtype, sched, rop, lib.da_expr_jit_errstr(),
                    src.value.decode()[-1500:])
                assert src.value not in seen
                seen.add(src.value)
    text = src.value
    assert b'#include "expr_dims_core.hpp"' in text
    assert b"da::expr_dims_body<" in text
    assert b"da::fanin_finish(" not in text and b"atomic" not in text
    assert dbg(arr, len(p), dtype, 2, 4, 0, 1, 1, src, 16384) != 0
    assert dbg(arr, len(p), dtype, 2, 0, 3, 1, 1, src, 16384) != 0
    assert dbg(arr, len(p), dtype, 2, 0, 0, 5, 1, src, 16384) != 0
    assert dbg(arr, len(p), 3, 2, 0, 0, 1, 1, src, 16384) != 0


# ------------------------------------------------------------------- names
def test_names_agree(ffi):
    txt = open(HDR).read()
    m = re.search(r"enum da_expr_dims_variant \{(.*?)\};", txt, re.S)
    assert m, "enum da_expr_dims_variant missing from the header"
    names = re.findall(r"DA_EDIMS_(\w+)", m.group(1))
    assert tuple(n.lower() for n in names) == ffi.EXPR_DIMS_VARIANTS
    assert re.search(r"#define DA_EXPR_COUNT\s+\(-1\)", txt)
    assert ffi.EXPR_COUNT == -1
    assert re.search(r"\bint\s+dbg_expr_dims_variant\s*\(", txt)
    assert "da_expr_reduce_dims" in ffi._sigs
    assert hasattr(ffi.lib, "da_expr_reduce_dims")
    assert hasattr(ffi.lib, "dbg_expr_dims_variant")
    proto = re.search(r"^int\s+da_expr_reduce_dims\s*\((.*?)\);", txt,
                      re.M | re.S)
    assert len(proto.group(1).split(",")) == \
        len(ffi._sigs["da_expr_reduce_dims"][0])
    integ = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    assert ":da_expr_reduce_dims" in integ
    assert ":dbg_expr_dims_variant" in integ
    for k, n in enumerate(names):
        assert "%d = DA_EDIMS_%s" % (k, n) in integ
    stub = re.search(r"\(:da_expr_reduce_dims, libdarray\), Cint,\s*\((.*?)\)",
                     integ, re.S)
    assert len(stub.group(1).split(",")) == \
        len(ffi._sigs["da_expr_reduce_dims"][0])


def test_python_api_exported():
    import inspect
    import distributedarrays_jl_amd as dja
    from distributedarrays_jl_amd import expr as E
    for name in ("dvar_dims", "dstd_dims", "dcount_dims", "dall_dims",
                 "dany_dims"):
        assert name in dja.__all__ and callable(getattr(dja, name))
    for f in (E.reduce, E.count, dja.mapreduce):
        p = inspect.signature(f).parameters["dims"]
        assert p.default is None
