"""The radix digits' 32-bit magic multipliers, on the CPU.

A build of fewer than 2^16 buckets takes its radix digits floor(b / div) mod R with m =
ceil(2^32 / d) and one 32-bit high multiply per division (kmer_hasher_amd/csrc/kmhg_plan.h:
magic32, digit32_ok, div_magic32, digit32 -- the functions the kernels of kmhg_build_v2.hip
call).  tools/asan/digit_check is a stand-alone program built with ASan + UBSan that runs them
for every dividend below 2^16 against plain division and against the general 64-bit form."""
import os
import subprocess

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
EXE = os.path.join(ROOT, "tools", "asan", "digit_check")


@pytest.fixture(scope="module")
def exe():
    # flock: pytest-xdist workers each run this fixture; one make at a time
    r = subprocess.run(["flock", os.path.join(ROOT, "tools", "asan", ".build.lock"),
                        "make", "-s", "-C", os.path.join(ROOT, "tools", "asan"), "digit_check"],
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


def test_every_divisor_up_to_the_widest_radix(exe):
    """d in [1, 320] and the bound's edge (2^15, 2^15 + 1, 2^16 - 1, 2^16, ...): the multiplier is
    ceil(2^32 / d) and the quotient equals x / d for every x < 2^16."""
    got = run(exe, "divisors")
    assert len(got) == 1 and got[0].startswith("ok ") and int(got[0][3:]) >= 320


def test_every_digit_of_one_and_two_pass_plans(exe):
    """Every (div, R) a one- or two-pass plan produces for 1 .. 13,824 buckets (at the widest
    radix 320, 256 and 118): digit and high quotient equal the 64-bit form's and plain division's
    for every bucket id below 2^16."""
    got = run(exe, "plans")
    assert len(got) == 1 and got[0].startswith("ok ") and int(got[0][3:]) >= 300


def test_predicate_refuses_large_bucket_counts(exe):
    """digit32_ok refuses 2^16 buckets or more and divisors beyond 2^16; the plan sets the flag
    for the 10 Mbp build and its parts and not for a 100 Mbp build."""
    assert run(exe, "predicate") == ["ok"]
