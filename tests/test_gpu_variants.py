"""Every env-gated kernel variant, inside the suite.  The switches
(DA_RED_FUSED, DA_RV4, DA_RBLOCKS, DA_NT, ...) are read once per
process, so each variant runs tests/variant_child.py in a fresh child with
the switch in ITS environment; this process's environment and program are
never changed.  Children run strictly one at a time.  If one dies by a
signal, aborts, segfaults or reaches its time limit, no further child is
started: the remaining variants skip with that reason."""
import os
import subprocess
import sys

import pytest

from variant_child import VARIANTS, variant_id

pytestmark = pytest.mark.gpu

CHILD = os.path.join(os.path.dirname(os.path.abspath(__file__)),
                     "variant_child.py")
CHILD_TIMEOUT = 120
_faulted = []     # ids of children that died; non-empty stops the module


def _died(returncode):
    return returncode < 0 or returncode in (134, 139)


@pytest.mark.parametrize("env,check_set", VARIANTS,
                         ids=[variant_id(e) for e, _ in VARIANTS])
def test_variant(env, check_set):
    if _faulted:
        pytest.skip("an earlier variant child faulted (%s); not starting "
                    "further GPU processes" % _faulted[0])
    child_env = dict(os.environ)
    child_env.update(env)
    tag = variant_id(env)
    try:
        r = subprocess.run([sys.executable, CHILD, check_set], env=child_env,
                           capture_output=True, text=True,
                           timeout=CHILD_TIMEOUT)
    except subprocess.TimeoutExpired as e:
        _faulted.append(tag)
        err = e.stderr or ""
        if isinstance(err, bytes):
            err = err.decode(errors="replace")
        pytest.fail("variant %s: child exceeded %d s\n%s"
                    % (tag, CHILD_TIMEOUT, err[-2000:]))
    if _died(r.returncode):
        _faulted.append(tag)
    assert r.returncode == 0, "variant %s: child exit %d\n%s" % (
        tag, r.returncode, r.stderr[-2000:])
    assert "variant ok: %s" % check_set in r.stdout
