"""Parity check of every env-gated kernel variant (documented experiments
must not rot).  The variant table and the checks live with the suite —
tests/variant_child.py, run by tests/test_gpu_variants.py; this tool walks
the same table by hand: one fresh child process per variant, one at a
time, stopping at the first child that dies."""
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
from variant_child import VARIANTS, variant_id  # noqa: E402

CHILD = os.path.join(ROOT, "tests", "variant_child.py")


def main():
    fails = 0
    for env, check_set in VARIANTS:
        e = dict(os.environ)
        e.update(env)
        tag = variant_id(env)
        try:
            r = subprocess.run([sys.executable, CHILD, check_set], env=e,
                               capture_output=True, text=True, timeout=180)
        except subprocess.TimeoutExpired:
            print("HUNG", tag, "- stopping")
            sys.exit(2)
        if r.returncode != 0:
            print("FAIL", tag, r.stderr[-300:])
            fails += 1
            if r.returncode < 0 or r.returncode in (134, 139):
                print("child died (%d) - stopping" % r.returncode)
                sys.exit(2)
        else:
            print("ok  ", tag)
    sys.exit(1 if fails else 0)


if __name__ == "__main__":
    main()
