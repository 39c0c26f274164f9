"""kmer.max.occ's host-testable pieces, on the CPU.

kmer_hasher_amd/csrc/kmhg_querycall.h holds the occurrence cap's rules once: the argument rule
with the entry's words (max_occ_refusal), how a query call carries the value (with_max_occ), and
the rule of one window record under a cap (qrec_kept, qrec_rows) -- the two functions k_qrec_mask
of kmhg_kernels.hip evaluates per window.  tools/asan/maxocc_check, a stand-alone program built
with ASan + UBSan, drives them."""
import os
import subprocess

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
EXE = os.path.join(ROOT, "tools", "asan", "maxocc_check")


@pytest.fixture(scope="module")
def exe():
    # flock: pytest-xdist workers each run this fixture; one make at a time
    r = subprocess.run(["flock", os.path.join(ROOT, "tools", "asan", ".build.lock"),
                        "make", "-s", "-C", os.path.join(ROOT, "tools", "asan"), "maxocc_check"],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    return EXE


def run(exe, *args):
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0:exitcode=99",
               UBSAN_OPTIONS="print_stacktrace=1")
    r = subprocess.run([exe, *map(str, args)], capture_output=True, text=True, env=env,
                       timeout=300)
    assert r.returncode == 0, (args, r.returncode, r.stdout[-500:], r.stderr[-3000:])
    assert "Sanitizer" not in r.stderr and "runtime error" not in r.stderr, r.stderr[-3000:]
    return [l for l in r.stdout.split("\n") if l]


def test_argument_refusals_and_the_call_carries_the_value(exe):
    """0, 1, 2^31-1 legal; -1, 2^31 and int64's extremes refused in the entry's words."""
    got = run(exe, "refusals")
    assert len(got) == 1 and got[0].startswith("ok ") and int(got[0][3:]) >= 16


def test_record_rule_at_the_boundary(exe):
    """count = max_occ kept with all its rows, max_occ + 1 dropped, at max_occ = 1 .. 2^31-1; a
    no-hit or single-hit record is kept under every cap."""
    got = run(exe, "records")
    assert len(got) == 1 and got[0].startswith("ok ") and int(got[0][3:]) >= 5_000


def test_tile_total_is_what_the_windows_keep(exe):
    got = run(exe, "tile")
    assert len(got) == 1 and got[0].startswith("ok ") and int(got[0][3:]) >= 98
