"""The device pool on the GPU: two rounds of build + self-query + free in one process reuse the
first round's blocks, and a trim leaves nothing cached.  One child process with the test build of
the library and KMHG_POOL_TRACE=1 (tests/pool_trace_child.py), whose stderr carries one line per
device allocation."""
import os
import subprocess
import sys

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))

# device allocations traced after the marker, measured with this child on the commit before the
# pool moved into kmhg_pool.h (profiles/pool1_trace_compare.txt; 22 before the marker)
ALLOCS_SECOND_ROUND = 0


@pytest.mark.gpu
def test_second_round_reuses_the_pool_and_trim_empties_it():
    sys.path.insert(0, HERE)
    from pool_trace_child import MARKER
    env = dict(os.environ, KMHG_LIB_VARIANT="test", KMHG_POOL_TRACE="1")
    r = subprocess.run(["timeout", "-k", "10", "120", sys.executable,
                        os.path.join(HERE, "pool_trace_child.py")], env=env,
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    out = [l.split() for l in r.stdout.split("\n") if l]
    assert [l[0] for l in out] == ["round", "round", "cached"], r.stdout
    err = r.stderr.split("\n")
    assert err.count(MARKER) == 1, r.stderr[-4000:]
    at = err.index(MARKER)
    first = sum("kmhg pool: hipMalloc" in l for l in err[:at])
    second = sum("kmhg pool: hipMalloc" in l for l in err[at:])
    print("hipMalloc lines: first round", first, "second round", second)
    assert first > 0                                  # the trace is on
    assert out[2][1] == "0", r.stdout                 # cached bytes after the trim
    assert out[0][2:] == out[1][2:], r.stdout         # (U, N, P) of both rounds
    assert second == ALLOCS_SECOND_ROUND
