"""How a flat reduce hands its scalar to the host: the single-launch kernels
store the value and then release-store a per-launch sequence number into a
pinned slot, and the host polls the sequence word for DA_RED_SPIN_US
microseconds (default 2000) before it falls back to the stream sync.

Checked here: no call ever returns another call's value (a sequence seen
before its value, or a value of the previous launch, is a wrong integer);
which of the two paths answered (da_dbg_reduce_waits); DA_RED_SPIN_US=0 is
the stream sync for every call; a budget that runs out mid-kernel still
returns the right value; result bits do not depend on the wait.

Every expected value is an exact integer (reduce_wait_child.py), so every
comparison is ==.  Sizes are from the project's edge set: 1 (one block, the
shortest kernel: the host is already spinning when it ends), 257, 2^20+1
(grid cap, second grid-stride pass, tail), 2^22+1 (the longest kernel of
the set, for the budget that expires)."""
import os
import subprocess
import sys

import pytest

import reduce_wait_child as rw

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
CHILD_TIMEOUT = 120
SWITCHES = ("DA_RED_SPIN_US", "DA_RED_FUSED", "DA_RV4", "DA_EXPR_JIT")
_faulted = []     # children that died; non-empty stops further children


@pytest.fixture(scope="module")
def dja():
    import distributedarrays_jl_amd as dja
    dja.comm.init()
    return dja


def run_child(script, args, env_extra, tag):
    """One child at a time, under its own timeout; after a child that died
    no further child is started."""
    if _faulted:
        pytest.fail("an earlier child faulted (%s); not starting further "
                    "GPU processes" % _faulted[0])
    env = dict(os.environ)
    for k in SWITCHES:
        env.pop(k, None)
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


def parse(out):
    """(values, (polled, synced, calls)) of a reduce_wait_child run; every
    value is checked against the expectation printed next to it."""
    lines = out.splitlines()
    assert lines[-1] == "wait done", out[-500:]
    w = lines[-2].split()
    assert w[0] == "waits", lines[-2]
    vals = []
    for ln in lines[:-2]:
        tag, got, want = ln.rsplit(" ", 2)
        assert int(got) == int(want), ln
        vals.append((tag, int(got)))
    return vals, tuple(int(v) for v in w[1:])


@pytest.mark.parametrize("n", [1, 257, (1 << 20) + 1])
def test_no_stale_result(dja, n):
    """200 alternating i64 sums, each followed by one of the other three
    publishing kernels or an f32 sum: 400 results, each its own."""
    p0, s0 = rw.waits()
    res = rw.sequence(dja, n, 200)
    p1, s1 = rw.waits()
    assert len(res) == 400
    for tag, got, want in res:
        assert got == want, (tag, got, want)
    assert (p1 - p0) + (s1 - s0) == 400


@pytest.mark.parametrize("n", [2, 513, (1 << 20) + 1])
def test_default_results_come_from_the_poll(dja, n):
    """The default budget (2000 us) is far above these kernels' run time
    (tens of microseconds at most), so every result is polled, none
    synced."""
    assert "DA_RED_SPIN_US" not in os.environ
    p0, s0 = rw.waits()
    res = rw.sequence(dja, n, 20)
    p1, s1 = rw.waits()
    for tag, got, want in res:
        assert got == want, (tag, got, want)
    print("n=%d polled +%d synced +%d" % (n, p1 - p0, s1 - s0))
    assert p1 - p0 == len(res) == 40
    assert s1 - s0 == 0


def test_spin_zero_is_the_stream_sync(dja):
    """DA_RED_SPIN_US=0 in a fresh process: never polled, every call
    synced, the values of the default path."""
    sizes = [1, 257, (1 << 20) + 1]
    out = run_child("reduce_wait_child.py", ["8"] + [str(n) for n in sizes],
                    {"DA_RED_SPIN_US": "0"}, "wait DA_RED_SPIN_US=0")
    vals, (polled, synced, calls) = parse(out)
    assert calls == len(vals) == 16 * len(sizes)
    assert polled == 0
    assert synced == calls
    here = []
    for n in sizes:
        here += [(tag, got) for tag, got, _ in rw.sequence(dja, n, 8)]
    assert vals == here


def test_budget_expiry_falls_back_to_the_sync():
    """DA_RED_SPIN_US=1 at 2^22+1: the budget can run out while the kernel
    runs; whichever path answers, the value is right and every call is
    counted once.  No assertion about the split."""
    out = run_child("reduce_wait_child.py", ["12", str((1 << 22) + 1)],
                    {"DA_RED_SPIN_US": "1"}, "wait DA_RED_SPIN_US=1")
    vals, (polled, synced, calls) = parse(out)
    print("budget 1 us: polled %d synced %d of %d" % (polled, synced, calls))
    assert calls == len(vals) == 24
    assert polled + synced == calls


@pytest.mark.parametrize("script", ["reduce_bits_child.py",
                                    "expr_reduce_bits_child.py"])
def test_bits_do_not_depend_on_the_wait(script):
    one = run_child(script, [], {}, script + " default")
    two = run_child(script, [], {"DA_RED_SPIN_US": "0"},
                    script + " DA_RED_SPIN_US=0")
    assert one.endswith("bits done\n") and one.count("\n") == 19, one
    assert one == two
