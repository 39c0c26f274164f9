"""The row-free segment route's host-testable pieces, on the CPU.

kmer_hasher_amd/csrc/kmhg_segrec.h (the list search with a hint, the membership in a window's
record, the start / end classes the kernels of kmhg_segrec.hip compute per hit, and the refusal
rule on the 64-bit totals) is driven by tools/asan/segrec_check, a stand-alone program built with
ASan + UBSan: a host loop over the same functions (classify every hit of every window, pair by
std::sort) against a std::set restatement of the definition in include/kmhgpu.h, every list in an
exact-size allocation.  No Python code is loaded under a sanitizer."""
import os
import subprocess

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
EXE = os.path.join(ROOT, "tools", "asan", "segrec_check")


@pytest.fixture(scope="module")
def exe():
    # flock: pytest-xdist workers each run this fixture; one make at a time
    r = subprocess.run(["flock", os.path.join(ROOT, "tools", "asan", ".build.lock"),
                        "make", "-s", "-C", os.path.join(ROOT, "tools", "asan"), "segrec_check"],
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


def test_crafted_records_match_the_definition(exe):
    """The search from every hint (out-of-range ones too) on consecutive, strided and extreme
    lists, and on lists that are not ascending; empty, single and list windows; equal, shifted
    and disjoint neighbour lists; j = 1 and j = 2^31 - 1; the refusal rule with totals around
    2^31 and 2^32 (unequal totals that agree modulo 2^32 do not pair)."""
    got = run(exe, "crafted")
    assert len(got) == 1 and got[0].startswith("ok ") and int(got[0][3:]) >= 55


@pytest.mark.parametrize("seed", [1, 2, 3])
def test_random_records_match_the_definition(exe, seed):
    # up to 30 windows over up to 60 positions at 1 .. 100 % density, at either end of the range
    assert run(exe, "random", seed, 3000) == ["ok 3000"]
