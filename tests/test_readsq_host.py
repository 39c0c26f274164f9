"""The batched read query's host side, on the CPU.

kmer_hasher_amd/csrc/kmhg_readsq.h -- the call and its refusals, the offsets' rule, the map from a
virtual entry to (read, strand, window), the window rule of one read on either strand with its
mirrored end-drop, the row arithmetic and the vote's cell, key and winner packing, all of which the
kernels of kmhg_readsq.hip evaluate through the same functions -- runs in tools/asan/readsq_check,
a stand-alone program built with ASan + UBSan, against plain restatements (a linear scan over the
reads, the reference's walk on an explicitly reversed and complemented read, floor division).
Nothing is loaded into Python under a sanitizer."""
import os
import subprocess

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
EXE = os.path.join(ROOT, "tools", "asan", "readsq_check")


@pytest.fixture(scope="module")
def exe():
    # flock: pytest-xdist workers each run this fixture; one make at a time
    r = subprocess.run(["flock", os.path.join(ROOT, "tools", "asan", ".build.lock"),
                        "make", "-s", "-C", os.path.join(ROOT, "tools", "asan"), "readsq_check"],
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
    out = [l for l in r.stdout.split("\n") if l]
    assert len(out) == 1 and out[0].startswith("ok "), out
    return int(out[0][3:])


@pytest.mark.parametrize("k", [1, 15, 31])
def test_entry_map_matches_a_linear_scan(exe, k):
    """Empty reads, reads of k - 1, k and k + 1 bases, 5,000 one-base reads, one read of three
    tiles; good offsets pass, broken ones are refused and place nothing outside the buffers."""
    assert run(exe, "map", k) > 100_000


@pytest.mark.parametrize("k,seed", [(1, 1), (5, 2), (15, 3), (31, 4)])
def test_window_rule_on_both_strands(exe, k, seed):
    """The reverse strand from the forward bases == the rule on an explicitly reversed read; the
    mirrored end-drop: forward window 0 dropped iff the read has k bases or read[k] is N."""
    assert run(exe, "window", k, seed) > 10_000


def test_every_refusal(exe):
    assert run(exe, "refusals") >= 30


def test_vote_cell_key_and_winner(exe):
    assert run(exe, "votes", 9) > 100_000
