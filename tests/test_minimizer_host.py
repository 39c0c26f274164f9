"""Minimizer sampling's host-testable pieces, on the CPU.

kmer_hasher_amd/csrc/kmhg_minimizer.h holds the rule once: the argument rule with the entries'
words (minimizer_w_refusal), whether a window is selected given its neighbours' hashes
(minimizer_selected, which k_minimizer_mask of kmhg_minimizer.hip evaluates per window) and the
host mask of a string (minimizer_mask_host, kmhg_minimizer_mask).  tools/asan/minimizer_check, a
stand-alone program built with ASan + UBSan, drives them."""
import os
import subprocess

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
EXE = os.path.join(ROOT, "tools", "asan", "minimizer_check")


@pytest.fixture(scope="module")
def exe():
    # flock: pytest-xdist workers each run this fixture; one make at a time
    r = subprocess.run(["flock", os.path.join(ROOT, "tools", "asan", ".build.lock"),
                        "make", "-s", "-C", os.path.join(ROOT, "tools", "asan"), "minimizer_check"],
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


def test_argument_refusals(exe):
    """w = 1 and 256 legal; 0, 257, negatives refused in the entries' words; a refused host mask
    writes nothing."""
    got = run(exe, "refusals")
    assert len(got) == 1 and got[0].startswith("ok ") and int(got[0][3:]) >= 20


def test_host_mask_on_the_edge_strings(exe):
    """Random strings, single Ns and runs of Ns, an N before the last window, "A" x 300, a
    period-3 repeat, mixed case; forward and rc; w = 1, 2, 5, 19, 255, 256 and Nw - 1, Nw,
    Nw + 1 on short pieces -- against a span-by-span restatement, into exactly Nw bytes."""
    got = run(exe, "edges")
    assert len(got) == 1 and got[0].startswith("ok ") and int(got[0][3:]) >= 600


def test_plan_of_a_sampled_request(exe):
    """A part with w > 1 is refused ("part builds index every window (w must be 1)"), a key stream
    too; a sampled sequence compacts first, without bucket ids, Pack8, codes or tags, in the
    unsampled geometry; w = 1 plans what the unsampled request plans."""
    got = run(exe, "plan")
    assert len(got) == 1 and got[0].startswith("ok ") and int(got[0][3:]) >= 15
