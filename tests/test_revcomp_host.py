"""The reverse-complement query's host-side pieces, on the CPU.

kmer_hasher_amd/csrc/kmhg_revcomp.h (the 16-char word transform the probe's mirrored stage fill
applies, and the arithmetic that anchors the rc tiling at the sequence end) runs in
tools/asan/revcomp_check, a stand-alone program built with ASan + UBSan, against a char-by-char
restatement of the definition in include/kmhgpu.h.  tests/revcomp_ref.py's rc_host -- the helper
every GPU rc test feeds to the forward oracle -- is pinned on literals, and the clean-room oracle
is pinned against the compiled reference on a reverse-complemented input."""
import os
import subprocess

import numpy as np
import pytest

from oracle import oracle as O
from revcomp_ref import rc_host

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
EXE = os.path.join(ROOT, "tools", "asan", "revcomp_check")


@pytest.fixture(scope="module")
def exe():
    # flock: pytest-xdist workers each run this fixture; one make at a time
    r = subprocess.run(["flock", os.path.join(ROOT, "tools", "asan", ".build.lock"),
                        "make", "-s", "-C", os.path.join(ROOT, "tools", "asan"), "revcomp_check"],
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


@pytest.mark.parametrize("seed", [1, 2, 3])
def test_word_transform_matches_the_definition_and_is_an_involution(exe, seed):
    # 16-char words over ACGT, acgt, N, n and both cases of RYKMSWBDHV plus '-' and '.'
    got = run(exe, "words", seed, 100_000)
    assert got == ["ok 400000"]


def test_rc_stage_is_anchored_at_the_sequence_end(exe):
    """Every L up to 4 tiles' worth of residues and every tile start: forward blocks 16-aligned,
    the first window HALO .. HALO + 15 chars into the stage, stage words = the packed rc string."""
    got = run(exe, "stage", 130)
    assert len(got) == 1 and got[0].startswith("ok ") and int(got[0][3:]) > 10_000


def test_rc_host_literals():
    assert rc_host("ACGTA") == "TACGT"
    assert rc_host(b"ACGTA") == b"TACGT"
    assert rc_host("ACNGnT") == "ANCNGT"                 # N and n stay N, in place
    assert rc_host("R") == "G"                           # by the 2-bit code, no IUPAC rule
    assert rc_host("acgt") == "ACGT"                     # lower case: its code, upper-case out
    a = np.frombuffer(b"AACCGGTTN", np.uint8)
    assert rc_host(a).tobytes() == b"NAACCGGTT"
    assert rc_host(rc_host("ACGTNNACGGT")) == "ACGTNNACGGT"


def test_rc_host_is_the_usage_scripts_rule_except_for_n():
    """test.R's rev.comp: reverse, then "ACTG"[(code + 2) %% 4]; it would turn N (code 3) into
    C.  Every byte but N / n follows it."""
    for c in range(1, 256):
        want = "ACTG"[(((c >> 1) & 3) + 2) % 4]
        got = rc_host(bytes([c])).decode("latin-1")
        if c in (ord("N"), ord("n")):
            assert got == "N" and want == "C"
        else:
            assert got == want


def test_oracle_agrees_with_reference_on_a_reverse_complement(testfa):
    """The clean-room oracle is the checker of the GPU rc tests; here it is pinned against the
    compiled reference on the same class of input (a reverse-complemented query)."""
    if not O.ref_available():
        pytest.skip("reference build not available")
    q = rc_host(testfa)
    ref = O.RefIndex(testfa, 15)
    want = ref.query(q, 15)
    ref.close()
    got = O.OracleIndex(testfa, 15).query(q, 15)
    assert len(want) > 0 and np.array_equal(got, want)
