"""Host side of comparisons and masks, no GPU: the argument checks of
da_compact / da_expand (they run before the da_init check and touch no
memory), the agreement of the header, the Python binding, the opcode table
and the INTEGRATION.md stubs on the new names and values, and the exact
program words the expression compiler emits for comparisons."""
import ctypes
import os
import re
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HDR = os.path.join(ROOT, "include", "darray_hip.h")

F64, F32, I64 = 0, 1, 2


@pytest.fixture(scope="module")
def ffi():
    from distributedarrays_jl_amd import _ffi
    return _ffi


def _err(lib, rc):
    return (lib.da_errstr(rc) or b"").decode()


@pytest.fixture()
def bufs():
    # real host memory behind the pointers: a check that did touch them
    # would read or write these bytes, not fault
    a = (ctypes.c_uint8 * 256)(*([0xA5] * 256))
    b = (ctypes.c_uint8 * 256)(*([0x5A] * 256))
    c = (ctypes.c_uint8 * 256)(*([0x3C] * 256))
    yield a, b, c
    assert bytes(a) == b"\xa5" * 256
    assert bytes(b) == b"\x5a" * 256
    assert bytes(c) == b"\x3c" * 256


# Calls that PASS the argument check must only ever meet the da_init check
# here (their pointers are host memory), so they run in a child process
# that certainly never initialised the library.
_CHILD_PRELUDE = """
import ctypes, sys
sys.path.insert(0, %r)
from distributedarrays_jl_amd import _ffi
lib = _ffi.lib
err = lambda rc: (lib.da_errstr(rc) or b'').decode()
a = (ctypes.c_uint8 * 256)(*([0xA5] * 256))
b = (ctypes.c_uint8 * 256)(*([0x5A] * 256))
c = (ctypes.c_uint8 * 256)(*([0x3C] * 256))
pa, pb, pc = (ctypes.addressof(x) for x in (a, b, c))
assert lib.da_synchronize() < 0
""" % ROOT
_CHILD_EPILOGUE = """
assert bytes(a) == b'\\xa5' * 256 and bytes(b) == b'\\x5a' * 256
assert bytes(c) == b'\\x3c' * 256
print('child ok')
"""


def _child(body):
    r = subprocess.run([sys.executable, "-c",
                        _CHILD_PRELUDE + body + _CHILD_EPILOGUE],
                       capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "child ok" in r.stdout, \
        r.stdout[-1000:] + r.stderr[-3000:]


def test_good_calls_before_init_name_da_init():
    _child("""
# dst, src, mask apart
rc = lib.da_compact(pa, 4, pb, 0, pc, 2, 4, 0)
assert rc < 0 and 'da_init' in err(rc), err(rc)
# src == mask: both are only read
rc = lib.da_compact(pa, 4, pb, 0, pb, 0, 4, 0)
assert rc < 0 and 'da_init' in err(rc), err(rc)
# findall: no src
rc = lib.da_compact(pa, 4, None, 2, pb, 1, 4, 7)
assert rc < 0 and 'da_init' in err(rc), err(rc)
# abutting dst / src is no overlap
rc = lib.da_compact(pa, 4, pa + 32, 0, pb, 0, 4, 0)
assert rc < 0 and 'da_init' in err(rc), err(rc)
# n == 0 and dst_cap == 0 are judged by the same entry check
rc = lib.da_compact(None, 0, None, 0, None, 0, 0, 0)
assert rc < 0 and 'da_init' in err(rc), err(rc)
rc = lib.da_compact(None, 0, pb, 0, pc, 0, 4, 0)
assert rc < 0 and 'da_init' in err(rc), err(rc)
# da_expand: apart; dst == mask exactly; a broadcast source; nothing to do
rc = lib.da_expand(pa, 0, pb, 2, 4, pc, 4, 0)
assert rc < 0 and 'da_init' in err(rc), err(rc)
rc = lib.da_expand(pa, 0, pa, 2, 4, pc, 4, 0)
assert rc < 0 and 'da_init' in err(rc), err(rc)
rc = lib.da_expand(pa, 1, pa, 1, 8, pc, 1, 1)
assert rc < 0 and 'da_init' in err(rc), err(rc)
rc = lib.da_expand(None, 0, None, 0, 0, None, 0, 0)
assert rc < 0 and 'da_init' in err(rc), err(rc)
rc = lib.da_expand(pa, 0, pb, 0, 4, None, 0, 0)
assert rc < 0 and 'da_init' in err(rc), err(rc)
""")


def test_n_zero_is_no_argument_error(ffi, bufs):
    """n == 0 passes every argument check whatever the pointers are and
    launches nothing: what comes back is 0, or the da_init complaint where
    the library was never initialised, never an argument error."""
    lib = ffi.lib
    for rc in (lib.da_compact(None, 0, None, F64, None, F64, 0, 0),
               lib.da_expand(None, F64, None, F64, 0, None, 0, 0)):
        assert rc == 0 or "da_init" in _err(lib, rc)


@pytest.mark.parametrize("dtype,mdtype,word", [
    (3, F64, "bad dtype"), (-1, F64, "bad dtype"),
    (F64, 3, "bad mask_dtype"), (F32, -1, "bad mask_dtype"),
])
def test_bad_dtypes_rejected(ffi, bufs, dtype, mdtype, word):
    lib = ffi.lib
    a, b, c = bufs
    pa, pb, pc = (ctypes.addressof(x) for x in (a, b, c))
    rc = lib.da_compact(pa, 4, pb, dtype, pc, mdtype, 4, 0)
    assert rc < 0
    msg = _err(lib, rc)
    assert "da_compact" in msg and word in msg and "da_init" not in msg
    rc = lib.da_expand(pa, dtype, pc, mdtype, 4, pb, 4, 0)
    assert rc < 0
    msg = _err(lib, rc)
    assert "da_expand" in msg and word in msg and "da_init" not in msg


def test_null_pointers_rejected(ffi, bufs):
    lib = ffi.lib
    a, b, c = bufs
    pa, pb, pc = (ctypes.addressof(x) for x in (a, b, c))
    rc = lib.da_compact(None, 4, pb, F64, pc, F64, 4, 0)
    assert rc < 0 and "null dst" in _err(lib, rc)
    rc = lib.da_compact(pa, 4, pb, F64, None, F64, 4, 0)
    assert rc < 0 and "null mask" in _err(lib, rc)
    rc = lib.da_expand(None, F64, pc, F64, 4, pb, 4, 0)
    assert rc < 0 and "null" in _err(lib, rc)
    rc = lib.da_expand(pa, F64, None, F64, 4, pb, 4, 0)
    assert rc < 0 and "null" in _err(lib, rc)
    rc = lib.da_expand(pa, F64, pc, F64, 4, None, 4, 0)
    assert rc < 0 and "null src" in _err(lib, rc)


def test_overlap_rejected(ffi, bufs):
    lib = ffi.lib
    a, b, c = bufs
    pa, pb, pc = (ctypes.addressof(x) for x in (a, b, c))
    # dst one element into src / equal to src
    rc = lib.da_compact(pa + 8, 4, pa, F64, pb, F64, 4, 0)
    assert rc < 0 and "overlaps src" in _err(lib, rc)
    rc = lib.da_compact(pa, 4, pa, F64, pb, F64, 4, 0)
    assert rc < 0 and "overlaps src" in _err(lib, rc)
    # dst inside the mask (an f32 mask is half as long)
    rc = lib.da_compact(pa + 12, 4, pb, F64, pa, F32, 4, 0)
    assert rc < 0 and "overlaps mask" in _err(lib, rc)
    rc = lib.da_compact(pa, 4, None, I64, pa, I64, 4, 0)
    assert rc < 0 and "overlaps mask" in _err(lib, rc)
    # da_expand: dst == mask exactly passes (see the child above); a
    # partial overlap, or equal pointers with unequal element sizes, do not
    rc = lib.da_expand(pa + 8, F64, pa, F64, 4, pb, 4, 0)
    assert rc < 0 and "overlaps mask" in _err(lib, rc)
    rc = lib.da_expand(pa, F64, pa, F32, 4, pb, 4, 0)
    assert rc < 0 and "overlaps mask" in _err(lib, rc)
    rc = lib.da_expand(pa, F64, pb, F64, 4, pa + 24, 4, 0)
    assert rc < 0 and "overlaps src" in _err(lib, rc)
    # a broadcast source is one element long
    rc = lib.da_expand(pa, F64, pb, F64, 4, pa + 24, 4, 1)
    assert rc < 0 and "overlaps src" in _err(lib, rc)


@pytest.mark.parametrize("n,cap", [(1 << 61, 4), (1 << 62, 4),
                                   (4, 1 << 61), ((1 << 64) - 1, 1)])
def test_byte_count_overflow_rejected(ffi, bufs, n, cap):
    lib = ffi.lib
    a, b, c = bufs
    pa, pb, pc = (ctypes.addressof(x) for x in (a, b, c))
    rc = lib.da_compact(pa, cap, pb, F64, pc, I64, n, 0)
    assert rc < 0
    msg = _err(lib, rc)
    assert "da_compact" in msg and "overflows" in msg, msg
    rc = lib.da_expand(pa, I64, pc, F64, n, pb, cap, 0)
    assert rc < 0
    msg = _err(lib, rc)
    assert "da_expand" in msg and "overflows" in msg, msg


# ------------------------------------------------------------- names
def test_names_and_values_agree(ffi):
    from distributedarrays_jl_amd import _opcodes
    txt = open(HDR).read()
    m = re.search(r"enum da_cmpop \{(.*?)\};", txt, re.S)
    assert m, "enum da_cmpop missing from the header"
    body = m.group(1)
    assert re.search(r"DA_CMP_EQ\s*=\s*64\b", body)
    names = [n for n in re.findall(r"DA_CMP_(\w+)", body) if n != "_END"]
    assert names == ["EQ", "NE", "LT", "LE", "GT", "GE"]
    assert _opcodes.CMP_OPS == {n.lower(): 64 + k
                                for k, n in enumerate(names)}
    # the binary table is untouched and the two do not collide
    assert _opcodes.MAP2_OPS[-1] == "atan2" and len(_opcodes.MAP2_OPS) == 14
    assert not set(_opcodes.CMP_OPS) & set(_opcodes.MAP2_OPS)
    assert min(_opcodes.CMP_OPS.values()) >= len(_opcodes.MAP2_OPS)
    assert re.search(r"#define\s+DA_COMPACT_TILE\s+2048\b", txt)
    assert ffi.COMPACT_TILE == 2048
    integ = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    assert "DA_COMPACT_TILE = 2048" in integ
    for k, n in enumerate(names):
        assert "DA_CMP_%s = %d" % (n, 64 + k) in integ
    for fn in ("da_compact", "da_expand"):
        assert fn in ffi._sigs and hasattr(ffi.lib, fn)
        proto = re.search(r"^int\s+%s\s*\((.*?)\);" % fn, txt, re.M | re.S)
        assert proto, fn
        assert len(proto.group(1).split(",")) == len(ffi._sigs[fn][0])
        stub = re.search(r"\(:%s, libdarray\), Cint,\s*\((.*?)\)" % fn,
                         integ, re.S)
        assert stub, fn
        assert len(stub.group(1).split(",")) == len(ffi._sigs[fn][0])


def test_python_api_exported():
    import distributedarrays_jl_amd as dja
    for name in ("dfilter", "dfindall", "dsetmask_"):
        assert name in dja.__all__ and callable(getattr(dja, name))


# --------------------------------------------------- expression compile
class _Meta:
    """A DArray stand-in for the compiler: it only looks at identity."""
    lidx = ()

    def __init__(self, dtype="f64", dims=(8,)):
        self.dtype, self.dims, self.ndims = dtype, dims, len(dims)


def test_compile_words():
    from distributedarrays_jl_amd import expr as E
    a, b = _Meta(), _Meta()
    ARG0, ARG1, C0 = (1 << 8) | 0, (1 << 8) | 1, (2 << 8) | 0
    codes = {"eq": 64, "ne": 65, "lt": 66, "le": 67, "gt": 68, "ge": 69}
    for name, code in codes.items():
        f = getattr(E, name)
        prog, args, consts = E.compile_expr(f(E.ref(a), 0.5))
        assert prog == [ARG0, C0, (3 << 8) | code], name
        assert args == [a] and consts == [0.5]
        prog, args, consts = E.compile_expr(f(E.ref(a), E.ref(b)))
        assert prog == [ARG0, ARG1, (3 << 8) | code], name
        assert args == [a, b] and consts == []
    ops = {"lt": lambda x, y: x < y, "le": lambda x, y: x <= y,
           "gt": lambda x, y: x > y, "ge": lambda x, y: x >= y}
    for name, f in ops.items():
        prog, _, consts = E.compile_expr(f(E.ref(a), 0.5))
        assert prog == [ARG0, C0, (3 << 8) | codes[name]], name
        assert consts == [0.5]
    # a scalar on the left is reflected by Python: 0.5 < x is x > 0.5
    prog, _, _ = E.compile_expr(0.5 < E.ref(a))
    assert prog == [ARG0, C0, (3 << 8) | codes["gt"]]
    # comparisons compose with the arithmetic ops
    prog, _, _ = E.compile_expr((E.ref(a) > 0.5) * E.ref(b))
    assert prog == [ARG0, C0, (3 << 8) | 68, ARG1, (3 << 8) | 2]


def test_eq_stays_identity_and_hashable():
    from distributedarrays_jl_amd import expr as E
    e = E.ref(_Meta())
    assert (e == e) is True
    assert (e == E.ref(_Meta())) is False
    assert (e != e) is False
    assert len({e, e}) == 1 and hash(e) == hash(e)
    assert isinstance(E.eq(e, 1.0), E.Binary)
    assert isinstance(E.ne(e, 1.0), E.Binary)


def test_i64_trees_validate_and_unknown_names_raise():
    from distributedarrays_jl_amd import expr as E
    from distributedarrays_jl_amd._ffi import DArrayError
    a, b = _Meta("i64"), _Meta("i64")
    for name in ("eq", "ne", "lt", "le", "gt", "ge"):
        e = getattr(E, name)(E.ref(a) + 1, E.ref(b))
        prog, args, consts = E.compile_expr(e)
        E._validate(a, prog, args, consts)      # raised IndexError before
    # float-only ops are still refused for i64 next to a comparison
    prog, args, consts = E.compile_expr(E.lt(E.ref(a) / E.ref(b), 1))
    with pytest.raises(DArrayError):
        E._validate(a, prog, args, consts)
    with pytest.raises(DArrayError):
        E.Binary("spaceship", E.ref(a), E.ref(b))
    with pytest.raises(DArrayError):
        E.Binary("cmp", E.ref(a), E.lit(1))
