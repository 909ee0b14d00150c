"""The host waiter of the flat reduce (csrc/reduce_wait.hpp: the poll loop
and its budget) has no HIP dependency, so it is checked on the CPU:
tests/reduce_wait_host.cpp, a stand-alone program in which a thread plays
the device, is built with -fsanitize=thread and run.  It covers a late
publish, 2000 back-to-back publishes of 8- and 4-byte values, a result
that is never published (the waiter must time out within its budget plus a
margin, not hang) and a budget of zero.

On a host whose address-space layout the sanitizer's runtime cannot live
with, the program dies before main with "FATAL: ThreadSanitizer:
unexpected memory mapping" (older runtimes under a high mmap randomisation
setting).  Nothing of the program has run then, so it is started again
with address randomisation off for that one process (setarch -R); if that
is not possible either, the same program is built without the sanitizer
and must still pass: its value, timeout and no-hang checks do not need the
sanitizer, only the race report does."""
import os
import platform
import shutil
import subprocess

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
CSRC = os.path.join(ROOT, "distributedarrays_jl_amd", "csrc")
NO_START = "unexpected memory mapping"


def host_compiler():
    for name in (os.environ.get("CXX"), "c++", "g++", "clang++"):
        path = shutil.which(name) if name else None
        if path:
            return path
    return None


def build(cxx, exe, sanitize):
    cmd = [cxx, "-std=c++17", "-O1", "-g", "-pthread", "-I", CSRC,
           os.path.join(HERE, "reduce_wait_host.cpp"), "-o", exe]
    if sanitize:
        cmd.insert(1, "-fsanitize=thread")
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, "compile failed:\n%s" % r.stderr[-3000:]


def run(cmd):
    return subprocess.run(cmd, capture_output=True, text=True, timeout=120)


def check(r, how):
    assert r.returncode == 0, "%s: exit %d\n%s\n%s" % (
        how, r.returncode, r.stdout[-1000:], r.stderr[-3000:])
    assert "ThreadSanitizer" not in r.stderr, r.stderr[-3000:]
    assert r.stdout.startswith("reduce_wait_host ok"), r.stdout


def test_waiter_under_thread_sanitizer(tmp_path):
    cxx = host_compiler()
    if cxx is None:
        pytest.skip("no host C++ compiler")
    exe = str(tmp_path / "reduce_wait_host")
    build(cxx, exe, sanitize=True)
    r = run([exe])
    how = "thread sanitizer"
    if r.returncode != 0 and NO_START in r.stderr:
        setarch = shutil.which("setarch")
        if setarch:
            r = run([setarch, platform.machine(), "-R", exe])
            how = "thread sanitizer, address randomisation off"
        if r.returncode != 0 and (NO_START in r.stderr or not r.stdout):
            print("the sanitizer's runtime cannot start on this host (%s); "
                  "running the program without it" % r.stderr.strip()[-200:])
            plain = str(tmp_path / "reduce_wait_host_plain")
            build(cxx, plain, sanitize=False)
            r = run([plain])
            how = "no sanitizer (its runtime cannot start here)"
    print("reduce_wait_host ran with: %s" % how)
    check(r, how)
