"""The host side of the query entries (kmer_hasher_amd/csrc/kmhg_querycall.h) on the CPU: a query
call's checks in their order and with their texts, the launch sequence's rules, the KMHG_DEVICES
grammar, the multi-device split and the chars a window range reads, through tools/asan/host_check
(ASan + UBSan), a stand-alone program built from the header the engine compiles.  Every expected
value is computed here with Python integers; the char slices are also held against
dist.slice_bounds, the same rule written for a rank without the library."""
import os
import subprocess

import pytest

from kmer_hasher_amd.dist import slice_bounds

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
EXE = os.path.join(ROOT, "tools", "asan", "host_check")
EINVAL, EOVERFLOW = 1, 4            # include/kmhgpu.h
INT32_MAX = 2 ** 31 - 1

ARGS = "the sequence should be longer than k and k should not be longer than 31"
TOO_LONG = "sequence longer than 2^31-1 (int positions)"
RANGE = "window range out of bounds"


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
    r = subprocess.run([exe, "query", *map(str, args)], capture_output=True, text=True, env=env,
                       timeout=300)
    assert r.returncode == 0, (args, r.returncode, r.stdout[-500:], r.stderr[-3000:])
    assert "Sanitizer" not in r.stderr and "runtime error" not in r.stderr, r.stderr[-3000:]
    return [l for l in r.stdout.split("\n") if l]


def fields(line):
    return {n: int(v) for n, v in (w.split("=", 1) for w in line.split(" "))}


def refusal(code, msg):
    return [f"err={code} msg={msg}"]


# ---------------------------------------------------------------------------- query call
def call_model(L, k, w=None):
    """query_call / query_call_range restated: the refusal (code, text) or (w0, w1)"""
    if L <= k or k > 31 or k < 1:
        return EINVAL, ARGS
    if L >= INT32_MAX:
        return EOVERFLOW, TOO_LONG
    Nw = L - k + 1
    if w is None:
        return 0, Nw
    if w[0] < 0 or w[1] > Nw or w[0] > w[1]:
        return EINVAL, RANGE
    return w


def check_call(exe, L, k, w=None, want=None):
    model = call_model(L, k, w)
    if want is not None:
        assert model == want, (L, k, w, model, want)
    got = run(exe, "call", L, k, *(w or ()))
    if isinstance(model[1], str):
        assert got == refusal(*model), (L, k, w)
    else:
        assert len(got) == 1 and fields(got[0]) == {
            "err": 0, "L": L, "k": k, "w0": model[0], "w1": model[1], "part": 0, "runs": 0,
            "rc": 0}, (L, k, w, got)


def test_query_call(exe):
    check_call(exe, 1000, 8, want=(0, 993))
    check_call(exe, 32, 31, want=(0, 2))                        # the shortest at the largest k
    check_call(exe, 2, 1, want=(0, 2))
    for k in (0, 32, -1):
        check_call(exe, 1000, k, want=(EINVAL, ARGS))
    for k in (1, 8, 31):
        check_call(exe, k, k, want=(EINVAL, ARGS))              # L = k
        check_call(exe, k + 1, k, want=(0, 2))
    check_call(exe, 0, 8, want=(EINVAL, ARGS))
    check_call(exe, INT32_MAX, 31, want=(EOVERFLOW, TOO_LONG))
    check_call(exe, 2 ** 31, 31, want=(EOVERFLOW, TOO_LONG))
    check_call(exe, 2 ** 40, 8, want=(EOVERFLOW, TOO_LONG))
    check_call(exe, INT32_MAX - 1, 31, want=(0, INT32_MAX - 31))
    # a size_t length with the top bit set is a negative int64 in the first test: its sentence
    assert run(exe, "call", 2 ** 63, 8) == refusal(EINVAL, ARGS)


def test_query_call_range(exe):
    L, k = 1000, 8
    Nw = L - k + 1
    check_call(exe, L, k, (0, Nw), want=(0, Nw))
    check_call(exe, L, k, (17, 400), want=(17, 400))
    check_call(exe, L, k, (Nw - 1, Nw), want=(Nw - 1, Nw))
    for w in (0, 400, Nw):                                      # the empty range, at both ends too
        check_call(exe, L, k, (w, w), want=(w, w))
    check_call(exe, L, k, (-1, 10), want=(EINVAL, RANGE))
    check_call(exe, L, k, (0, Nw + 1), want=(EINVAL, RANGE))
    check_call(exe, L, k, (11, 10), want=(EINVAL, RANGE))
    check_call(exe, L, k, (Nw + 1, Nw + 1), want=(EINVAL, RANGE))
    check_call(exe, INT32_MAX - 1, 31, (0, INT32_MAX - 31), want=(0, INT32_MAX - 31))
    check_call(exe, INT32_MAX - 1, 31, (0, INT32_MAX - 30), want=(EINVAL, RANGE))


def test_query_call_refusal_order(exe):
    # k out of range and a length past 2^31-1: the sentence comes before the overflow
    check_call(exe, INT32_MAX, 32, want=(EINVAL, ARGS))
    check_call(exe, 2 ** 33, 0, want=(EINVAL, ARGS))
    # the arguments before the range: a bad k, a short or an overlong sequence with a bad range
    check_call(exe, 1000, 32, (-1, 5), want=(EINVAL, ARGS))
    check_call(exe, 8, 8, (5, 2), want=(EINVAL, ARGS))
    check_call(exe, INT32_MAX, 31, (-1, 5), want=(EOVERFLOW, TOO_LONG))
    check_call(exe, INT32_MAX, 31, (0, 2 ** 40), want=(EOVERFLOW, TOO_LONG))


# ---------------------------------------------------------------------------- query rules
def test_query_rules(exe):
    for Nw in (1, 7, 8, 2 ** 31 - 2):
        assert run(exe, "rules", f"guess={Nw}") == [f"guess={Nw + Nw // 8 + 64}"]
    assert run(exe, "rules", "guess=1", "guess=7", "guess=8") == ["guess=65", "guess=71",
                                                                 "guess=73"]
    # runs: 12 B each against 8 B per row, kept only where strictly smaller and there are rows
    for H, NR in ((0, 0), (3, 2), (3, 1), (300, 200), (300, 199), (301, 200), (1, 0),
                  (2 ** 31 - 1, (2 ** 32 - 2) // 3), (2 ** 31 - 1, (2 ** 32 - 2) // 3 + 1)):
        want = 1 if H and 3 * NR < 2 * H else 0
        assert run(exe, "rules", f"runs_pay={H},{NR}") == [f"runs_pay={want}"], (H, NR)
    assert run(exe, "rules", "runs_pay=300,200", "runs_pay=300,199", "runs_pay=0,0") == [
        "runs_pay=0", "runs_pay=1", "runs_pay=0"]
    for cap in (1, 73, 2 ** 31):
        assert run(exe, "rules", f"redo={cap},{cap}", f"redo={cap + 1},{cap}",
                   f"redo=0,{cap}") == ["redo=0", "redo=1", "redo=0"]
    # kq, index k, sources, index windows, U, code words, knob: eligible, then each one false
    ok = [31, 31, 0, 1000, 900, 1, 1]
    assert run(exe, "rules", "diag=" + ",".join(map(str, ok))) == ["diag=1"]
    for at, v in ((0, 15), (1, 15), (2, 1), (3, 0), (3, -5), (4, 0), (5, 0), (6, 0)):
        bad = list(ok)
        bad[at] = v
        assert run(exe, "rules", "diag=" + ",".join(map(str, bad))) == ["diag=0"], (at, v)
    assert run(exe, "rules", "diag=8,8,0,1,1,1,1") == ["diag=1"]


# ---------------------------------------------------------------------------- query devices
def devices_text(n, text):
    return f'KMHG_DEVICES must list device ordinals (0..{n - 1}), got "{text}"'


def test_query_devices(exe):
    assert run(exe, "devices", "0", 1) == ["err=0 devices=0"]
    assert run(exe, "devices", "0,1", 2) == ["err=0 devices=0,1"]
    assert run(exe, "devices", "1,1,0", 2) == ["err=0 devices=1,1,0"]     # repeats and order kept
    assert run(exe, "devices", "7,0,3", 8) == ["err=0 devices=7,0,3"]
    assert run(exe, "devices", "", 8) == ["err=0 devices="]               # nothing listed
    for n, text in ((2, "0,,1"), (2, "0,1,"), (2, ","), (2, ",0"), (2, "a"), (2, "0,a"),
                    (2, "1x"), (2, "-1"), (2, "2"), (8, "8"), (8, "0,1,8"), (1, "1"),
                    (2, "0;1")):
        assert run(exe, "devices", text, n) == refusal(EINVAL, devices_text(n, text)), (n, text)


# ---------------------------------------------------------------------------- query shards
def test_query_shards(exe):
    for k in (8, 31):
        for G in (1, 2, 3, 7):
            for Nw in sorted({0, 1, G - 1, G, 1000003}):
                L = Nw + k - 1
                got = [fields(l) for l in run(exe, "shards", L, k, G)]
                assert len(got) == G
                # the engine's split: contiguous, covering [0, Nw), no part larger than another
                # by more than one window
                assert [(s["w0"], s["w1"]) for s in got] == \
                    [(Nw * i // G, Nw * (i + 1) // G) for i in range(G)]
                assert got[0]["w0"] == 0 and got[-1]["w1"] == Nw
                assert all(a["w1"] == b["w0"] for a, b in zip(got, got[1:]))
                sizes = [s["w1"] - s["w0"] for s in got]
                assert min(sizes) >= 0 and max(sizes) - min(sizes) <= 1
                for s in got:
                    w0, w1, c0, c1 = s["w0"], s["w1"], s["c0"], s["c1"]
                    # the two copies of the rule, tied
                    assert (c0, c1) == slice_bounds(L, k, w0, w1), (L, k, G, s)
                    assert c0 == 0 or c0 % 16 == 0
                    assert 0 <= c0 <= c1 <= L
                    if w1 == w0:                 # no window: nothing is read, nothing is sent
                        assert (c0, c1) == (0, 0)
                    else:                        # what the window rule reads
                        assert c0 <= max(0, w0 - 1) and min(L, w1 + k - 1) <= c1, (L, k, G, s)


def test_query_shard_chars_at_the_ends(exe):
    """One part is the whole sequence; a later part starts on a 16-char boundary at least 64 chars
    before its first window and ends at most k + 64 past its last window's start."""
    k, Nw = 31, 1000003
    L = Nw + k - 1
    assert [fields(l) for l in run(exe, "shards", L, k, 1)] == [
        {"w0": 0, "w1": Nw, "c0": 0, "c1": L}]
    for s in [fields(l) for l in run(exe, "shards", L, k, 7)][1:-1]:
        assert s["c0"] == (s["w0"] & ~15) - 64 and s["c1"] == s["w1"] + k + 64


def test_query_part_offsets(exe):
    for H in ([5], [0, 0, 0], [3, 0, 7, 1], [2 ** 31 - 1] * 8):
        off = [sum(H[:i]) for i in range(len(H))]
        assert run(exe, "offsets", ",".join(map(str, H))) == [
            f"total={sum(H)} off={','.join(map(str, off))}"]
