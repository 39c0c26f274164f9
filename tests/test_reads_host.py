"""The host side of read counting (kmer_hasher_amd/csrc/kmhg_reads.h) on the CPU: the decoding of a
call's parameter vector, the split of packed reads into device batches, the reader's loop with its
flush, reads_longer_than and the spectrum's argument scan, through tools/asan/host_check (ASan +
UBSan), a stand-alone program built from the header the engine compiles.  Every expected value is
computed here with Python integers and floats."""
import math
import os
import subprocess

import fq_sh_inputs as I
import numpy as np
import pytest

from oracle import oracle as O

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
EXE = os.path.join(ROOT, "tools", "asan", "host_check")
EINVAL, EOVERFLOW = 1, 4            # include/kmhgpu.h
M64 = (1 << 64) - 1

K_RANGE = "k must be a positive integer less than 1+MAX_K"
K_32 = "k must be at most 31 for the suffix hash"
SOURCE_N = "Source_n must be in the range 1 - 4"
SOURCE_I = "source_i must be less than source_n"
PREFIX_2K = "prefix_bits must not exceed 2k"
SUFFIX_BITS = "suffix bits (2k - prefix_bits) must be in 0 .. 32"
MAX_MEMORY = "max_memory is too small for the prefix array of the suffix hash"


@pytest.fixture(scope="module")
def exe():
    # flock: pytest-xdist workers each run this fixture; one make at a time
    r = subprocess.run(["flock", os.path.join(ROOT, "tools", "asan", ".build.lock"),
                        "make", "-s", "-C", os.path.join(ROOT, "tools", "asan")],
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


def fnv(b: bytes, h: int = 1469598103934665603) -> int:
    for x in b:
        h = ((h ^ x) * 1099511628211) & M64
    return h


def fields(line):
    return dict(w.split("=", 1) for w in line.split(" "))


def refusal(code, msg):
    return f"err={code} msg={msg}"


# ---------------------------------------------------------------------------- read-call
def u32(x):
    return x & 0xFFFFFFFF


def qll(q):
    """q_to_ll: -708 below '"', else log(1 - 10^(-(q-33)/10)) through 15 significant digits"""
    return -708.0 if q < 34 else float("%.15g" % math.log(1.0 - 10.0 ** (-(q - 33) / 10.0)))


def rp_model(p):
    """read_call_rp restated: the refusal (code, text), or the decoded fields"""
    k, pb, min_q, _, max_reads, _, source_n, source_i = p
    if k < 1 or k > 32:
        return EINVAL, K_RANGE
    if u32(source_n) > 4 or u32(source_n) < 1:
        return EINVAL, SOURCE_N
    if u32(source_i) >= u32(source_n):
        return EINVAL, SOURCE_I
    if k == 32:
        return EINVAL, K_32
    if 2 * k < 32 and min(u32(pb), 36) > 2 * k:
        return EINVAL, PREFIX_2K
    return {"k": k, "sources": source_n, "single": 0, "sh1": 0,
            "min_ll": qll((33 + (min_q & 0xFF)) & 0xFF), "mq": 0, "source": source_i,
            "max_reads": max_reads & M64}


def sh1_model(p):
    k, _, pb, max_memory, min_quality, max_read_n = p
    if k < 1 or k > 32:
        return EINVAL, K_RANGE
    if k == 32:
        return EINVAL, K_32
    if u32(2 * k - u32(pb)) > 32:
        return EINVAL, SUFFIX_BITS
    if u32(pb) > 60 or (8 << u32(pb)) > ((max_memory & M64) << 30) & M64:
        return EINVAL, MAX_MEMORY
    mq = (min_quality + 33) & 0xFF
    return {"k": k, "sources": 1, "single": 1, "sh1": 1, "min_ll": 0.0,
            "mq": mq - 256 if mq > 127 else mq, "source": 0, "max_reads": max_read_n & M64}


def check_call(exe, kind, p, want=None):
    """host_check's answer against the model's, and against `want` where the case names one"""
    model = (rp_model if kind == "rp" else sh1_model)(p)
    if want is not None:
        assert model == want, (kind, p, model, want)
    got = run(exe, "read-call", kind, *p)
    assert len(got) == 1, got
    if isinstance(model, tuple):
        assert got[0] == refusal(*model), (kind, p)
        return None
    f = fields(got[0])
    assert f.pop("err") == "0"
    assert float(f.pop("min_ll")) == model["min_ll"], (kind, p)
    assert {n: int(v) for n, v in f.items()} == {n: v for n, v in model.items() if n != "min_ll"}, \
        (kind, p)
    return model


def rp(k=21, prefix_bits=20, min_q=10, max_reads=-1, source_n=1, source_i=0):
    return [k, prefix_bits, min_q, 47, max_reads, 200, source_n, source_i]


def test_read_call_rp_refusals(exe):
    for k in (0, 33, -1):
        check_call(exe, "rp", rp(k=k), (EINVAL, K_RANGE))
    check_call(exe, "rp", rp(k=32), (EINVAL, K_32))
    for n in (0, 5, -1):
        check_call(exe, "rp", rp(source_n=n), (EINVAL, SOURCE_N))
    for n, i in ((1, 1), (4, 4), (2, 3), (3, -1)):
        check_call(exe, "rp", rp(source_n=n, source_i=i), (EINVAL, SOURCE_I))
    check_call(exe, "rp", rp(k=15, prefix_bits=31), (EINVAL, PREFIX_2K))
    check_call(exe, "rp", rp(k=15, prefix_bits=99), (EINVAL, PREFIX_2K))     # 99 clamps to 36
    check_call(exe, "rp", rp(k=15, prefix_bits=-1), (EINVAL, PREFIX_2K))
    # the reference's order: k before the sources, source_n before source_i, the sources before
    # k = 32 and the prefix bits
    check_call(exe, "rp", rp(k=0, source_n=0), (EINVAL, K_RANGE))
    check_call(exe, "rp", rp(source_n=5, source_i=7), (EINVAL, SOURCE_N))
    check_call(exe, "rp", rp(k=32, source_n=0), (EINVAL, SOURCE_N))
    check_call(exe, "rp", rp(k=5, prefix_bits=11, source_i=1), (EINVAL, SOURCE_I))


def test_read_call_rp_accepted(exe):
    assert check_call(exe, "rp", rp(k=15, prefix_bits=30))["k"] == 15          # 2k itself
    assert check_call(exe, "rp", rp(k=16, prefix_bits=33))["k"] == 16          # 2k + 1 at k = 16
    assert check_call(exe, "rp", rp(k=16, prefix_bits=99))["k"] == 16
    assert check_call(exe, "rp", rp(k=31, prefix_bits=99))["k"] == 31
    assert check_call(exe, "rp", rp(k=1, prefix_bits=2))["k"] == 1
    m = check_call(exe, "rp", rp(source_n=4, source_i=3))
    assert (m["sources"], m["source"]) == (4, 3)
    # the threshold: qualities 0, 1 and 41 against log(1 - 10^(-(q-33)/10)) through %.15g
    assert check_call(exe, "rp", rp(min_q=0))["min_ll"] == -708.0
    for q in (1, 41):
        want = float("%.15g" % math.log(1.0 - 10.0 ** (-q / 10.0)))
        assert check_call(exe, "rp", rp(min_q=q))["min_ll"] == want
    # '!' + min_q as an unsigned char: 222 is char 255, 223 wraps to char 0, 256 to '!'
    assert check_call(exe, "rp", rp(min_q=222))["min_ll"] == qll(255)
    assert check_call(exe, "rp", rp(min_q=223))["min_ll"] == -708.0
    assert check_call(exe, "rp", rp(min_q=256 + 41))["min_ll"] == qll(74)
    assert check_call(exe, "rp", rp(min_q=-1))["min_ll"] == -708.0
    assert check_call(exe, "rp", rp(max_reads=-1))["max_reads"] == 2 ** 64 - 1
    assert check_call(exe, "rp", rp(max_reads=0))["max_reads"] == 0
    assert check_call(exe, "rp", rp(max_reads=2 ** 31 - 1))["max_reads"] == 2 ** 31 - 1
    assert check_call(exe, "rp", rp(max_reads=-2 ** 31))["max_reads"] == 2 ** 64 - 2 ** 31


def sh1(k=21, prefix_bits=20, max_memory=100, min_quality=30, max_read_n=-1):
    return [k, 1, prefix_bits, max_memory, min_quality, max_read_n]


def test_read_call_sh1_refusals(exe):
    for k in (0, 33, -1):
        check_call(exe, "sh1", sh1(k=k), (EINVAL, K_RANGE))
    check_call(exe, "sh1", sh1(k=32, prefix_bits=32), (EINVAL, K_32))
    check_call(exe, "sh1", sh1(k=10, prefix_bits=21), (EINVAL, SUFFIX_BITS))   # 2k - 21 wraps
    # prefix_bits -1 is 2^32 - 1: 2k + 1 suffix bits after the wrap, refused as more than 60
    check_call(exe, "sh1", sh1(k=10, prefix_bits=-1), (EINVAL, MAX_MEMORY))
    check_call(exe, "sh1", sh1(k=31, prefix_bits=29), (EINVAL, SUFFIX_BITS))   # 33 suffix bits
    check_call(exe, "sh1", sh1(k=31, prefix_bits=61, max_memory=-1), (EINVAL, MAX_MEMORY))
    # 8 B << prefix_bits against max_memory GiB: one step too small
    check_call(exe, "sh1", sh1(k=31, prefix_bits=30, max_memory=7), (EINVAL, MAX_MEMORY))
    check_call(exe, "sh1", sh1(k=20, prefix_bits=27, max_memory=0), (EINVAL, MAX_MEMORY))
    check_call(exe, "sh1", sh1(k=31, prefix_bits=33, max_memory=63), (EINVAL, MAX_MEMORY))
    # the suffix bits are looked at before the memory
    check_call(exe, "sh1", sh1(k=31, prefix_bits=29, max_memory=0), (EINVAL, SUFFIX_BITS))


def test_read_call_sh1_accepted(exe):
    assert check_call(exe, "sh1", sh1(k=31, prefix_bits=30, max_memory=8))["k"] == 31
    assert check_call(exe, "sh1", sh1(k=20, prefix_bits=27, max_memory=1))["k"] == 20
    assert check_call(exe, "sh1", sh1(k=31, prefix_bits=33, max_memory=64))["k"] == 31
    assert check_call(exe, "sh1", sh1(k=10, prefix_bits=20))["k"] == 10        # no suffix bits
    assert check_call(exe, "sh1", sh1(k=16, prefix_bits=0, max_memory=1))["k"] == 16   # 32 of them
    # a negative max_memory is a huge unsigned one: (2^64 - m) GiB mod 2^64
    assert check_call(exe, "sh1", sh1(k=31, prefix_bits=60, max_memory=-1))["k"] == 31
    assert check_call(exe, "sh1", sh1(k=31, prefix_bits=60, max_memory=-2 ** 31))["k"] == 31
    for p in I.FILE_CASES.values():
        assert isinstance(check_call(exe, "sh1", p[0][1]), dict)
    # (char)min_quality + '!' as a signed char: 94 is the last threshold above 0
    for q, mq in ((0, 33), (30, 63), (94, 127), (95, -128), (222, -1), (223, 0), (-33, 0),
                  (-34, -1), (2 ** 31 - 1, 32), (-2 ** 31, 33)):
        assert check_call(exe, "sh1", sh1(min_quality=q))["mq"] == mq, q
    assert check_call(exe, "sh1", sh1(max_read_n=-1))["max_reads"] == 2 ** 64 - 1
    assert check_call(exe, "sh1", sh1(max_read_n=5))["max_reads"] == 5


# ---------------------------------------------------------------------------- read-batches
def greedy(lens, span_max):
    """ranges [i0, i1) taken greedily, each spanning < span_max bases"""
    out, i0 = [], 0
    while i0 < len(lens):
        i1, span = i0 + 1, lens[i0]
        while i1 < len(lens) and span + lens[i1] < span_max:
            span += lens[i1]
            i1 += 1
        out.append((i0, i1))
        i0 = i1
    return out


def batches(exe, tmp_path, lens, span_max):
    path = str(tmp_path / "lens.txt")
    with open(path, "w") as f:
        f.write("\n".join(map(str, lens)) + "\n")
    return run(exe, "read-batches", span_max, path)


def check_batches(exe, tmp_path, lens, span_max):
    got = [tuple(map(int, l.split())) for l in batches(exe, tmp_path, lens, span_max)]
    assert got == greedy(lens, span_max), (lens[:20], span_max)
    # the ranges tile [0, n) and each spans fewer than span_max bases
    assert [a for a, _ in got] == [0] * bool(lens) + [b for _, b in got[:-1]]
    assert (got[-1][1] if got else 0) == len(lens)
    assert all(a < b and sum(lens[a:b]) < span_max for a, b in got)
    return got


def test_read_batches(exe, tmp_path):
    assert check_batches(exe, tmp_path, [], 100) == []
    assert check_batches(exe, tmp_path, [57], 100) == [(0, 1)]
    assert check_batches(exe, tmp_path, [99] * 5, 100) == [(i, i + 1) for i in range(5)]
    assert check_batches(exe, tmp_path, [0, 0, 0], 1) == [(0, 3)]
    # a batch boundary where off[i1] - off[i0] is exactly span_max - 1, and one base more
    assert check_batches(exe, tmp_path, [40, 59, 1, 98, 1, 1], 100) == [(0, 2), (2, 4), (4, 6)]
    assert check_batches(exe, tmp_path, [40, 60, 1], 100) == [(0, 1), (1, 3)]
    # ~200 ragged reads, the longest of 700 bases, at both spans of test_host_split_by_span
    rng = np.random.default_rng(7)
    lens = [int(x) for x in rng.integers(22, 700, 199)] + [700]
    rng.shuffle(lens)
    for span in (701, 4000, 2 ** 32 - 1):
        got = check_batches(exe, tmp_path, lens, span)
        assert len(got) > (2 if span == 4000 else 50 if span == 701 else 0)
    assert len(check_batches(exe, tmp_path, lens, 2 ** 32 - 1)) == 1


def test_read_batches_refuses_a_long_read_before_any_range(exe, tmp_path):
    want = [refusal(EOVERFLOW, "a read of 2^32 or more bases")]
    assert batches(exe, tmp_path, [100], 100) == want
    assert batches(exe, tmp_path, [10, 20, 30, 100], 100) == want      # the last read of four
    assert batches(exe, tmp_path, [10, 5000, 30], 701) == want


# ---------------------------------------------------------------------------- the reader
@pytest.fixture(scope="module")
def mixed_file(tmp_path_factory):
    """Records with and without qualities, shorter and longer than k = 9, one of them empty."""
    c9, fa = I.lane_cases(9), I.fa_cases(9)
    recs = c9["short"][0] + fa["two_records"] + c9["weak_last"][0] + [(b"ACGTA", None), (b"", None)]
    recs += c9["reads_64"][0][:5] + [(b"ACGTACGTAC", None)]
    path = str(tmp_path_factory.mktemp("reads") / "mixed.fx")
    with open(path, "wb") as f:
        f.write(I.fastx_bytes(recs))
    assert [r for r in O.fastx_records(I.fastx_bytes(recs))] == recs
    return path, recs


def packed(recs):
    """ReadsHost of the records: offsets, has_qual, bases, qualities (0 where there are none)"""
    off = np.concatenate(([0], np.cumsum([len(s) for s, _ in recs]))).astype(np.int64)
    return {"n": str(len(recs)), "off": ",".join(map(str, off)),
            "hasq": "".join("0" if q is None else "1" for _, q in recs),
            "seq": f"{fnv(b''.join(s for s, _ in recs)):016x}",
            "qual": f"{fnv(b''.join(bytes(len(s)) if q is None else q for s, q in recs)):016x}"}


def test_reads_longer_than(exe, mixed_file):
    path, recs = mixed_file
    read = [r for r in recs if len(r[0]) > 0]                   # read_fastx at k = 0
    lens = sorted({len(s) for s, _ in read})
    assert lens[0] == 5 and lens[-1] > 4000
    for k in (0, 4, 5, 8, 9, 10, 32, lens[-2], lens[-1] - 1, lens[-1], 10 ** 6):
        f = fields(run(exe, "reads-longer", k, path)[0])
        kept = [r for r in read if len(r[0]) > k]
        # all long: the object itself comes back, no copy
        assert f.pop("same") == ("1" if len(kept) == len(read) else "0"), k
        assert f == packed(kept), k
    assert packed([])["off"] == "0"                              # all short: empty, off == {0}


def expect_fastx(recs, k, max_reads, batch):
    """read_fastx restated: the flushes (reads, bases) and the T line's fields"""
    flushes, kept, n, bases = [], [], 0, 0
    taken = recs[:max_reads]
    for s, q in taken:
        if len(s) <= k:
            continue
        kept.append((s, q))
        n, bases = n + 1, bases + len(s)
        if bases >= batch:
            flushes.append(f"B {n} {bases}")
            n = bases = 0
    p = packed(kept)
    return flushes, {"read_n": str(len(taken)), "records": str(len(taken)),
                     "lens": ",".join(str(len(s)) for s, _ in kept), "hasq": p["hasq"],
                     "seq": p["seq"], "qual": p["qual"]}


def test_read_fastx_flush(exe, mixed_file):
    path, recs = mixed_file
    k = 9
    assert sum(len(s) <= k for s, _ in recs) >= 4
    whole = run(exe, "read-fastx", path, k, M64, 1 << 40)
    assert len(whole) == 1                                       # never flushed
    for batch in (1, 3 * 32, 5000, 1 << 40):                    # 96 bases: about three records
        for max_reads in (0, 1, 3, 4, 7, len(recs) - 1, len(recs), len(recs) + 1, M64):
            got = run(exe, "read-fastx", path, k, max_reads, batch)
            flushes, total = expect_fastx(recs, k, max_reads, batch)
            assert got[:-1] == flushes, (batch, max_reads)
            assert got[-1].startswith("T ") and fields(got[-1][2:]) == total, (batch, max_reads)
            # max_reads stops after exactly that many records, the short ones counted
            assert int(total["records"]) == min(max_reads, len(recs))
        # the flushed batches concatenate to the unflushed read
        assert got[-1] == whole[0], batch
        assert (len(got) > 3) == (batch < 5000)
    assert run(exe, "read-fastx", str(path) + ".absent", k, M64, 96) == \
        ["T read_n=0 records=0 lens= hasq= seq=%016x qual=%016x" % (fnv(b""), fnv(b""))]


# ---------------------------------------------------------------------------- spectrum-status
def test_spectrum_status(exe):
    def st(S, comb, inner):
        return run(exe, "spectrum-status", S, ",".join(map(str, comb)), ",".join(map(str, inner)))

    assert st(2, [1, 2, 3], [0, 1, 0]) == ["1"]
    assert st(1, [1], [0]) == ["1"]
    assert st(4, [15, 0], [1, 1]) == ["1"]
    assert st(2, [1], [2]) == ["-3"]
    assert st(2, [1], [-1]) == ["-3"]
    assert st(2, [4], [0]) == ["-4"]                             # comb == 1 << S
    assert st(4, [16], [0]) == ["-4"]
    assert st(2, [-1], [0]) == ["-4"]
    # the first offender wins, inner before comb in one entry
    assert st(2, [1, 4, 1], [0, 0, 2]) == ["-4"]
    assert st(2, [1, 1, 4], [0, 2, 0]) == ["-3"]
    assert st(2, [4], [2]) == ["-3"]
