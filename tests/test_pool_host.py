"""The device block pool (kmer_hasher_amd/csrc/kmhg_pool.h) on the CPU, over a fake device whose
blocks are malloc'ed bytes and whose events complete when the script says so, through
tools/asan/host_check (ASan + UBSan, leaks reported) and host_check_tsan (ThreadSanitizer).  Each
scenario is a script of operations and, written out here from the pool's rules, the line of state
expected after every one: the block returned, the backend's call counts, cached(), the idle
events, the current device and every block by state.  Over every trace: each block the backend
handed out is in exactly one of live / free / pending / freed, cached is the sum of the free
blocks' classes, every block is freed on its own device, and at the end nothing is left."""
import os
import subprocess

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
ASAN = os.path.join(ROOT, "tools", "asan", "host_check")
TSAN = os.path.join(ROOT, "tools", "asan", "host_check_tsan")
MiB = 1 << 20


@pytest.fixture(scope="module")
def exes():
    # flock: pytest-xdist workers each run this fixture; one make at a time
    r = subprocess.run(["flock", os.path.join(ROOT, "tools", "asan", ".build.lock"),
                        "make", "-s", "-C", os.path.join(ROOT, "tools", "asan")],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    return {"asan": ASAN, "tsan": TSAN}


def run(exe, *args):
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0:exitcode=99",
               UBSAN_OPTIONS="print_stacktrace=1", TSAN_OPTIONS="exitcode=98")
    r = subprocess.run([exe, *map(str, args)], capture_output=True, text=True, env=env,
                       timeout=300)
    assert r.returncode == 0, (args, r.returncode, r.stdout[-500:], r.stderr[-3000:])
    assert "Sanitizer" not in r.stderr and "runtime error" not in r.stderr, r.stderr[-3000:]
    return [l for l in r.stdout.split("\n") if l]


def st(ret, calls, cached=0, idle=0, dev=0, live="", free="", pending="", freed=""):
    """One expected line.  calls: the backend's allocs, frees, event creates, records, event waits
    and stream waits so far.  Blocks are id:device:class, pending ones id:device:class:event:owns."""
    a, f, c, r, ew, sw = calls
    return (f"ret={ret} allocs={a} frees={f} creates={c} records={r} ewaits={ew} swaits={sw} "
            f"cached={cached} idle={idle} dev={dev} live={live} free={free} pending={pending} "
            f"freed={freed}")


def check_invariants(lines):
    for l in lines:
        f = dict(w.split("=", 1) for w in l.split(" "))
        sets = {n: [b.split(":") for b in f[n].split(",") if b] for n in ("live", "free", "pending")}
        freed = [int(x) for x in f["freed"].split(",") if x]
        assert all(x > 0 for x in freed), l                     # each freed on its own device
        ids = [int(b[0]) for v in sets.values() for b in v] + freed
        assert sorted(ids) == list(range(1, len(ids) + 1)), l   # exactly one state per block
        assert int(f["cached"]) == sum(int(b[2]) for b in sets["free"]), l
        assert int(f["frees"]) == len(freed), l
    assert f["live"] == f["free"] == f["pending"] == "" and f["cached"] == "0", lines[-1]


def play(exes, tmp_path, steps, knobs=None):
    """steps: (operation, expected line).  Runs the script and compares line by line."""
    path = str(tmp_path / "pool.script")
    with open(path, "w") as f:
        if knobs:
            f.write("knobs %d %d\n" % knobs)
        f.writelines(op + "\n" for op, _ in steps)
    got = run(exes["asan"], "pool", path)
    for i, ((op, want), g) in enumerate(zip(steps, got)):
        assert g == want, (i, op)
    assert len(got) == len(steps)
    check_invariants(got)
    return got


# ---------------------------------------------------------------------------- size classes
CLASS = {0: 256, 1: 256, 256: 256, 257: 512, MiB: MiB, MiB + 1: 2 * MiB, 3 * MiB: 4 * MiB}


@pytest.mark.parametrize("nbytes", sorted(CLASS))
def test_class_and_reuse_without_a_backend_alloc(exes, tmp_path, nbytes):
    c = CLASS[nbytes]
    play(exes, tmp_path, [
        (f"alloc a {nbytes}", st(1, (1, 0, 0, 0, 0, 0), live=f"1:0:{c}")),
        ("release a", st("-", (1, 0, 0, 0, 0, 0), cached=c, free=f"1:0:{c}")),
        ("cached", st(c, (1, 0, 0, 0, 0, 0), cached=c, free=f"1:0:{c}")),
        (f"alloc b {nbytes}", st(1, (1, 0, 0, 0, 0, 0), live=f"1:0:{c}")),       # reused
        (f"alloc c {nbytes}", st(2, (2, 0, 0, 0, 0, 0), live=f"1:0:{c},2:0:{c}")),
        ("release null", st("-", (2, 0, 0, 0, 0, 0), live=f"1:0:{c},2:0:{c}")),
        ("release unknown", st("-", (2, 0, 0, 0, 0, 0), live=f"1:0:{c},2:0:{c}")),
        ("release b", st("-", (2, 0, 0, 0, 0, 0), cached=c, live=f"2:0:{c}", free=f"1:0:{c}")),
        ("release b", st("-", (2, 0, 0, 0, 0, 0), cached=c, live=f"2:0:{c}", free=f"1:0:{c}")),
        ("release c", st("-", (2, 0, 0, 0, 0, 0), cached=2 * c, free=f"1:0:{c},2:0:{c}")),
        ("trim", st("-", (2, 2, 0, 0, 0, 0), freed="1,2")),
        ("cached", st(0, (2, 2, 0, 0, 0, 0), freed="1,2")),
    ])


# ---------------------------------------------------------------------------- best-fit
BIG = 384 * MiB
# request -> (its class, served by the free 384 MiB-class block?)
BEST_FIT = {254 * MiB: False, 256 * MiB: True, 300 * MiB: True, 384 * MiB: True, 386 * MiB: False}


@pytest.mark.parametrize("nbytes", sorted(BEST_FIT))
def test_best_fit_against_a_free_384_mib_block(exes, tmp_path, nbytes):
    head = [(f"alloc big {BIG}", st(1, (1, 0, 0, 0, 0, 0), live=f"1:0:{BIG}")),
            ("release big", st("-", (1, 0, 0, 0, 0, 0), cached=BIG, free=f"1:0:{BIG}"))]
    if BEST_FIT[nbytes]:      # the block keeps its class and returns to it
        play(exes, tmp_path, head + [
            (f"alloc a {nbytes}", st(1, (1, 0, 0, 0, 0, 0), live=f"1:0:{BIG}")),
            ("release a", st("-", (1, 0, 0, 0, 0, 0), cached=BIG, free=f"1:0:{BIG}")),
            ("trim", st("-", (1, 1, 0, 0, 0, 0), freed="1")),
        ])
    else:                     # below 256 MiB never; above 384 MiB it is too small
        assert nbytes % (2 * MiB) == 0
        play(exes, tmp_path, head + [
            (f"alloc a {nbytes}", st(2, (2, 0, 0, 0, 0, 0), cached=BIG, live=f"2:0:{nbytes}",
                                     free=f"1:0:{BIG}")),
            ("release a", st("-", (2, 0, 0, 0, 0, 0), cached=BIG + nbytes,
                             free=f"1:0:{BIG},2:0:{nbytes}")),
            ("trim", st("-", (2, 2, 0, 0, 0, 0), freed=("2,1" if nbytes < BIG else "1,2"))),
        ])


def test_best_fit_off_and_on_a_request_of_256_mib(exes, tmp_path):
    n = 256 * MiB
    play(exes, tmp_path, [
        (f"alloc big {BIG}", st(1, (1, 0, 0, 0, 0, 0), live=f"1:0:{BIG}")),
        ("release big", st("-", (1, 0, 0, 0, 0, 0), cached=BIG, free=f"1:0:{BIG}")),
        (f"alloc a {n}", st(2, (2, 0, 0, 0, 0, 0), cached=BIG, live=f"2:0:{n}", free=f"1:0:{BIG}")),
        ("release a", st("-", (2, 0, 0, 0, 0, 0), cached=BIG + n, free=f"1:0:{BIG},2:0:{n}")),
        ("trim", st("-", (2, 2, 0, 0, 0, 0), freed="2,1")),
    ], knobs=(1, 0))


def test_best_fit_takes_the_smallest_class_of_its_device_that_has_a_block(exes, tmp_path):
    a, b, c, n = 384 * MiB, 320 * MiB, 310 * MiB, 300 * MiB
    free3 = f"1:0:{a},2:0:{b},3:1:{c}"
    play(exes, tmp_path, [
        (f"alloc a {a}", st(1, (1, 0, 0, 0, 0, 0), live=f"1:0:{a}")),
        (f"alloc b {b}", st(2, (2, 0, 0, 0, 0, 0), live=f"1:0:{a},2:0:{b}")),
        ("dev 1", st("-", (2, 0, 0, 0, 0, 0), dev=1, live=f"1:0:{a},2:0:{b}")),
        (f"alloc c {c}", st(3, (3, 0, 0, 0, 0, 0), dev=1, live=free3)),
        ("release a", st("-", (3, 0, 0, 0, 0, 0), dev=1, cached=a, live=f"2:0:{b},3:1:{c}",
                         free=f"1:0:{a}")),
        ("release b", st("-", (3, 0, 0, 0, 0, 0), dev=1, cached=a + b, live=f"3:1:{c}",
                         free=f"1:0:{a},2:0:{b}")),
        ("release c", st("-", (3, 0, 0, 0, 0, 0), dev=1, cached=a + b + c, free=free3)),
        ("dev 0", st("-", (3, 0, 0, 0, 0, 0), cached=a + b + c, free=free3)),
        # 300 MiB on device 0: 320 MiB, not device 1's 310 and not the larger 384
        (f"alloc x {n}", st(2, (3, 0, 0, 0, 0, 0), cached=a + c, live=f"2:0:{b}",
                            free=f"1:0:{a},3:1:{c}")),
        # again: the 320 MiB class is empty now, 384 MiB is within 1.5 x 300
        (f"alloc y {n}", st(1, (3, 0, 0, 0, 0, 0), cached=c, live=f"1:0:{a},2:0:{b}",
                            free=f"3:1:{c}")),
        # a third finds nothing on device 0
        (f"alloc z {n}", st(4, (4, 0, 0, 0, 0, 0), cached=c, live=f"1:0:{a},2:0:{b},4:0:{n}",
                            free=f"3:1:{c}")),
        ("release x", st("-", (4, 0, 0, 0, 0, 0), cached=c + b, live=f"1:0:{a},4:0:{n}",
                         free=f"2:0:{b},3:1:{c}")),
        ("release y", st("-", (4, 0, 0, 0, 0, 0), cached=c + b + a, live=f"4:0:{n}", free=free3)),
        ("release z", st("-", (4, 0, 0, 0, 0, 0), cached=c + b + a + n, free=free3 + f",4:0:{n}")),
        ("trim", st("-", (4, 4, 0, 0, 0, 0), freed="4,2,1,3")),
    ])


# ---------------------------------------------------------------------------- ordered releases
def test_ordered_release_is_invisible_until_complete(exes, tmp_path):
    play(exes, tmp_path, [
        ("alloc a 1000", st(1, (1, 0, 0, 0, 0, 0), live="1:0:1024")),
        ("release a 5", st("-", (1, 0, 1, 1, 0, 0), pending="1:0:1024:1:1")),
        ("cached", st(0, (1, 0, 1, 1, 0, 0), pending="1:0:1024:1:1")),
        # another class and another device do not wait for it
        ("alloc b 300", st(2, (2, 0, 1, 1, 0, 0), live="2:0:512", pending="1:0:1024:1:1")),
        ("dev 1", st("-", (2, 0, 1, 1, 0, 0), dev=1, live="2:0:512", pending="1:0:1024:1:1")),
        ("alloc c 1000", st(3, (3, 0, 1, 1, 0, 0), dev=1, live="2:0:512,3:1:1024",
                            pending="1:0:1024:1:1")),
        ("dev 0", st("-", (3, 0, 1, 1, 0, 0), live="2:0:512,3:1:1024", pending="1:0:1024:1:1")),
        ("complete 1", st("-", (3, 0, 1, 1, 0, 0), live="2:0:512,3:1:1024",
                          pending="1:0:1024:1:1")),
        # the next request polls: the block is cached, its event idle
        ("alloc d 2000", st(4, (4, 0, 1, 1, 0, 0), cached=1024, idle=1,
                            live="2:0:512,3:1:1024,4:0:2048", free="1:0:1024")),
        ("alloc e 1000", st(1, (4, 0, 1, 1, 0, 0), idle=1,
                            live="1:0:1024,2:0:512,3:1:1024,4:0:2048")),
        ("release b", st("-", (4, 0, 1, 1, 0, 0), cached=512, idle=1,
                         live="1:0:1024,3:1:1024,4:0:2048", free="2:0:512")),
        ("release c", st("-", (4, 0, 1, 1, 0, 0), cached=1536, idle=1, live="1:0:1024,4:0:2048",
                         free="2:0:512,3:1:1024")),
        ("release d", st("-", (4, 0, 1, 1, 0, 0), cached=3584, idle=1, live="1:0:1024",
                         free="2:0:512,3:1:1024,4:0:2048")),
        ("release e", st("-", (4, 0, 1, 1, 0, 0), cached=4608, idle=1,
                         free="1:0:1024,2:0:512,3:1:1024,4:0:2048")),
        ("trim", st("-", (4, 4, 1, 1, 0, 0), idle=1, freed="2,1,4,3")),
    ])


def test_depth_1_waits_and_returns_the_same_block(exes, tmp_path):
    play(exes, tmp_path, [
        ("alloc a 4096", st(1, (1, 0, 0, 0, 0, 0), live="1:0:4096")),
        ("release a 9", st("-", (1, 0, 1, 1, 0, 0), pending="1:0:4096:1:1")),
        ("alloc b 4096", st(1, (1, 0, 1, 1, 1, 0), idle=1, live="1:0:4096")),
        # the event is recycled: no second create
        ("release b 9", st("-", (1, 0, 1, 2, 1, 0), pending="1:0:4096:1:1")),
        # a class with a block but none pending allocates
        ("alloc c 8192", st(2, (2, 0, 1, 2, 1, 0), live="2:0:8192", pending="1:0:4096:1:1")),
        ("alloc d 8192", st(3, (3, 0, 1, 2, 1, 0), live="2:0:8192,3:0:8192",
                            pending="1:0:4096:1:1")),
        ("release c", st("-", (3, 0, 1, 2, 1, 0), cached=8192, live="3:0:8192", free="2:0:8192",
                         pending="1:0:4096:1:1")),
        ("release d", st("-", (3, 0, 1, 2, 1, 0), cached=16384, free="2:0:8192,3:0:8192",
                         pending="1:0:4096:1:1")),
        ("trim", st("-", (3, 3, 1, 2, 2, 0), idle=1, freed="1,2,3")),
    ])


def test_depth_2_allocates_a_second_block_then_waits(exes, tmp_path):
    play(exes, tmp_path, [
        ("alloc a 4096", st(1, (1, 0, 0, 0, 0, 0), live="1:0:4096")),
        ("release a 9", st("-", (1, 0, 1, 1, 0, 0), pending="1:0:4096:1:1")),
        ("alloc b 4096", st(2, (2, 0, 1, 1, 0, 0), live="2:0:4096", pending="1:0:4096:1:1")),
        ("release b 9", st("-", (2, 0, 2, 2, 0, 0), pending="1:0:4096:1:1,2:0:4096:2:1")),
        ("alloc c 4096", st(1, (2, 0, 2, 2, 1, 0), idle=1, live="1:0:4096",
                            pending="2:0:4096:2:1")),
        ("release c", st("-", (2, 0, 2, 2, 1, 0), cached=4096, idle=1, free="1:0:4096",
                         pending="2:0:4096:2:1")),
        ("trim", st("-", (2, 2, 2, 2, 2, 0), idle=2, freed="1,2")),
    ], knobs=(2, 1))


def test_a_group_of_3_makes_one_record_and_returns_one_event(exes, tmp_path):
    live = "1:0:256,2:0:512,3:0:1024"
    play(exes, tmp_path, [
        ("alloc a 256", st(1, (1, 0, 0, 0, 0, 0), live="1:0:256")),
        ("alloc b 512", st(2, (2, 0, 0, 0, 0, 0), live="1:0:256,2:0:512")),
        ("alloc c 1024", st(3, (3, 0, 0, 0, 0, 0), live=live)),
        ("group_begin 4", st("-", (3, 0, 0, 0, 0, 0), live=live)),
        ("release a 4", st("-", (3, 0, 0, 0, 0, 0), live=live)),
        ("release b 4", st("-", (3, 0, 0, 0, 0, 0), live=live)),
        ("release c 4", st("-", (3, 0, 0, 0, 0, 0), live=live)),
        ("group_end", st("-", (3, 0, 1, 1, 0, 0),
                         pending="1:0:256:1:0,2:0:512:1:0,3:0:1024:1:1")),
        ("complete 1", st("-", (3, 0, 1, 1, 0, 0),
                          pending="1:0:256:1:0,2:0:512:1:0,3:0:1024:1:1")),
        ("alloc d 2048", st(4, (4, 0, 1, 1, 0, 0), cached=1792, idle=1, live="4:0:2048",
                            free=live)),
        ("release d", st("-", (4, 0, 1, 1, 0, 0), cached=3840, idle=1, free=live + ",4:0:2048")),
        # an empty group records nothing
        ("group_begin 4", st("-", (4, 0, 1, 1, 0, 0), cached=3840, idle=1,
                             free=live + ",4:0:2048")),
        ("group_end", st("-", (4, 0, 1, 1, 0, 0), cached=3840, idle=1, free=live + ",4:0:2048")),
        ("trim", st("-", (4, 4, 1, 1, 0, 0), idle=1, freed="1,2,3,4")),
    ])


def test_a_group_defers_only_ordered_releases_on_its_own_stream(exes, tmp_path):
    play(exes, tmp_path, [
        ("alloc a 256", st(1, (1, 0, 0, 0, 0, 0), live="1:0:256")),
        ("alloc b 256", st(2, (2, 0, 0, 0, 0, 0), live="1:0:256,2:0:256")),
        ("alloc c 512", st(3, (3, 0, 0, 0, 0, 0), live="1:0:256,2:0:256,3:0:512")),
        ("group_begin 4", st("-", (3, 0, 0, 0, 0, 0), live="1:0:256,2:0:256,3:0:512")),
        ("release a 4", st("-", (3, 0, 0, 0, 0, 0), live="1:0:256,2:0:256,3:0:512")),
        # another stream's: its own event, now
        ("release b 5", st("-", (3, 0, 1, 1, 0, 0), live="1:0:256,3:0:512",
                           pending="2:0:256:1:1")),
        # unordered: back at once
        ("release c", st("-", (3, 0, 1, 1, 0, 0), cached=512, live="1:0:256", free="3:0:512",
                         pending="2:0:256:1:1")),
        ("group_end", st("-", (3, 0, 2, 2, 0, 0), cached=512, free="3:0:512",
                         pending="1:0:256:2:1,2:0:256:1:1")),
        ("complete 1", st("-", (3, 0, 2, 2, 0, 0), cached=512, free="3:0:512",
                          pending="1:0:256:2:1,2:0:256:1:1")),
        ("complete 2", st("-", (3, 0, 2, 2, 0, 0), cached=512, free="3:0:512",
                          pending="1:0:256:2:1,2:0:256:1:1")),
        # (b was queued before a: the trim takes the pending blocks in that order)
        ("trim", st("-", (3, 3, 2, 2, 2, 0), idle=2, freed="2,1,3")),
    ])


def test_a_synced_group_records_nothing(exes, tmp_path):
    play(exes, tmp_path, [
        ("alloc a 256", st(1, (1, 0, 0, 0, 0, 0), live="1:0:256")),
        ("alloc b 512", st(2, (2, 0, 0, 0, 0, 0), live="1:0:256,2:0:512")),
        ("group_begin 4", st("-", (2, 0, 0, 0, 0, 0), live="1:0:256,2:0:512")),
        ("release a 4", st("-", (2, 0, 0, 0, 0, 0), live="1:0:256,2:0:512")),
        ("release b 4", st("-", (2, 0, 0, 0, 0, 0), live="1:0:256,2:0:512")),
        ("synced", st("-", (2, 0, 0, 0, 0, 0), live="1:0:256,2:0:512")),
        ("group_end", st("-", (2, 0, 0, 0, 0, 0), cached=768, free="1:0:256,2:0:512")),
        ("trim", st("-", (2, 2, 0, 0, 0, 0), freed="1,2")),
    ])


# ---------------------------------------------------------------------------- failures
def test_event_create_failure_waits_for_the_stream(exes, tmp_path):
    play(exes, tmp_path, [
        ("alloc a 256", st(1, (1, 0, 0, 0, 0, 0), live="1:0:256")),
        ("alloc b 512", st(2, (2, 0, 0, 0, 0, 0), live="1:0:256,2:0:512")),
        ("alloc c 1024", st(3, (3, 0, 0, 0, 0, 0), live="1:0:256,2:0:512,3:0:1024")),
        ("fail event 2", st("-", (3, 0, 0, 0, 0, 0), live="1:0:256,2:0:512,3:0:1024")),
        ("release a 4", st("-", (3, 0, 1, 0, 0, 1), cached=256, live="2:0:512,3:0:1024",
                           free="1:0:256")),
        ("group_begin 4", st("-", (3, 0, 1, 0, 0, 1), cached=256, live="2:0:512,3:0:1024",
                             free="1:0:256")),
        ("release b 4", st("-", (3, 0, 1, 0, 0, 1), cached=256, live="2:0:512,3:0:1024",
                           free="1:0:256")),
        ("release c 4", st("-", (3, 0, 1, 0, 0, 1), cached=256, live="2:0:512,3:0:1024",
                           free="1:0:256")),
        ("group_end", st("-", (3, 0, 2, 0, 0, 2), cached=1792,
                         free="1:0:256,2:0:512,3:0:1024")),
        ("trim", st("-", (3, 3, 2, 0, 0, 2), freed="1,2,3")),
    ])


def test_record_failure_waits_for_the_stream_and_keeps_the_event(exes, tmp_path):
    play(exes, tmp_path, [
        ("alloc a 256", st(1, (1, 0, 0, 0, 0, 0), live="1:0:256")),
        ("fail record 1", st("-", (1, 0, 0, 0, 0, 0), live="1:0:256")),
        ("release a 4", st("-", (1, 0, 1, 1, 0, 1), cached=256, idle=1, free="1:0:256")),
        ("alloc b 256", st(1, (1, 0, 1, 1, 0, 1), idle=1, live="1:0:256")),
        ("release b 4", st("-", (1, 0, 1, 2, 0, 1), pending="1:0:256:1:1")),
        ("trim", st("-", (1, 1, 1, 2, 1, 1), idle=1, freed="1")),
    ])


def test_out_of_memory_then_trim_then_success(exes, tmp_path):
    play(exes, tmp_path, [
        ("alloc a 256", st(1, (1, 0, 0, 0, 0, 0), live="1:0:256")),
        ("alloc b 512", st(2, (2, 0, 0, 0, 0, 0), live="1:0:256,2:0:512")),
        ("alloc keep 512", st(3, (3, 0, 0, 0, 0, 0), live="1:0:256,2:0:512,3:0:512")),
        ("release b", st("-", (3, 0, 0, 0, 0, 0), cached=512, live="1:0:256,3:0:512",
                         free="2:0:512")),
        ("release a 4", st("-", (3, 0, 1, 1, 0, 0), cached=512, live="3:0:512", free="2:0:512",
                           pending="1:0:256:1:1")),
        ("fail alloc-oom 1", st("-", (3, 0, 1, 1, 0, 0), cached=512, live="3:0:512",
                                free="2:0:512", pending="1:0:256:1:1")),
        # two backend calls around a trim that waited for a and freed a and b; keep is live
        ("alloc c 1024", st(4, (5, 2, 1, 1, 1, 0), idle=1, live="3:0:512,4:0:1024", freed="1,2")),
        # the 256 B class has no block any more: the next one is allocated
        ("alloc d 256", st(5, (6, 2, 1, 1, 1, 0), idle=1, live="3:0:512,4:0:1024,5:0:256",
                           freed="1,2")),
        ("release c", st("-", (6, 2, 1, 1, 1, 0), cached=1024, idle=1, live="3:0:512,5:0:256",
                         free="4:0:1024", freed="1,2")),
        ("release d", st("-", (6, 2, 1, 1, 1, 0), cached=1280, idle=1, live="3:0:512",
                         free="4:0:1024,5:0:256", freed="1,2")),
        ("release keep", st("-", (6, 2, 1, 1, 1, 0), cached=1792, idle=1,
                            free="3:0:512,4:0:1024,5:0:256", freed="1,2")),
        ("trim", st("-", (6, 5, 1, 1, 1, 0), idle=1, freed="1,2,5,3,4")),
    ])


def test_out_of_memory_twice_is_an_error_with_the_live_set_unchanged(exes, tmp_path):
    play(exes, tmp_path, [
        ("alloc a 256", st(1, (1, 0, 0, 0, 0, 0), live="1:0:256")),
        ("alloc b 512", st(2, (2, 0, 0, 0, 0, 0), live="1:0:256,2:0:512")),
        ("release b", st("-", (2, 0, 0, 0, 0, 0), cached=512, live="1:0:256", free="2:0:512")),
        ("fail alloc-oom 2", st("-", (2, 0, 0, 0, 0, 0), cached=512, live="1:0:256",
                                free="2:0:512")),
        ("alloc c 1024", st("oom", (4, 1, 0, 0, 0, 0), live="1:0:256", freed="2")),
        # any other error: no trim, no second call
        ("alloc b 512", st(3, (5, 1, 0, 0, 0, 0), live="1:0:256,3:0:512", freed="2")),
        ("release b", st("-", (5, 1, 0, 0, 0, 0), cached=512, live="1:0:256", free="3:0:512",
                         freed="2")),
        ("fail alloc-error 1", st("-", (5, 1, 0, 0, 0, 0), cached=512, live="1:0:256",
                                  free="3:0:512", freed="2")),
        ("alloc c 1024", st("error:fake_device_error", (6, 1, 0, 0, 0, 0), cached=512,
                            live="1:0:256", free="3:0:512", freed="2")),
        ("alloc c 1024", st(4, (7, 1, 0, 0, 0, 0), cached=512, live="1:0:256,4:0:1024",
                            free="3:0:512", freed="2")),
        ("release a", st("-", (7, 1, 0, 0, 0, 0), cached=768, live="4:0:1024",
                         free="1:0:256,3:0:512", freed="2")),
        ("release c", st("-", (7, 1, 0, 0, 0, 0), cached=1792, free="1:0:256,3:0:512,4:0:1024",
                         freed="2")),
        ("trim", st("-", (7, 4, 0, 0, 0, 0), freed="2,1,3,4")),
    ])


def test_trim_across_two_devices_restores_the_device_and_the_counts(exes, tmp_path):
    # depth 2, so that the per-class count shows: two blocks of (device 0, 256 B) before the trim
    play(exes, tmp_path, [
        ("alloc a 256", st(1, (1, 0, 0, 0, 0, 0), live="1:0:256")),
        ("alloc a2 256", st(2, (2, 0, 0, 0, 0, 0), live="1:0:256,2:0:256")),
        ("dev 1", st("-", (2, 0, 0, 0, 0, 0), dev=1, live="1:0:256,2:0:256")),
        ("alloc b 256", st(3, (3, 0, 0, 0, 0, 0), dev=1, live="1:0:256,2:0:256,3:1:256")),
        ("alloc keep 4096", st(4, (4, 0, 0, 0, 0, 0), dev=1,
                               live="1:0:256,2:0:256,3:1:256,4:1:4096")),
        ("release a 4", st("-", (4, 0, 1, 1, 0, 0), dev=1, live="2:0:256,3:1:256,4:1:4096",
                           pending="1:0:256:1:1")),
        ("release a2", st("-", (4, 0, 1, 1, 0, 0), dev=1, cached=256, live="3:1:256,4:1:4096",
                          free="2:0:256", pending="1:0:256:1:1")),
        ("release b", st("-", (4, 0, 1, 1, 0, 0), dev=1, cached=512, live="4:1:4096",
                         free="2:0:256,3:1:256", pending="1:0:256:1:1")),
        ("trim", st("-", (4, 3, 1, 1, 1, 0), dev=1, idle=1, live="4:1:4096", freed="2,1,3")),
        ("cached", st(0, (4, 3, 1, 1, 1, 0), dev=1, idle=1, live="4:1:4096", freed="2,1,3")),
        ("dev 0", st("-", (4, 3, 1, 1, 1, 0), idle=1, live="4:1:4096", freed="2,1,3")),
        # (device 0, 256 B) counts 0 again: one block, pending, is below the depth of 2, so
        # the next request allocates; with two it waits
        ("alloc c 256", st(5, (5, 3, 1, 1, 1, 0), idle=1, live="4:1:4096,5:0:256",
                           freed="2,1,3")),
        ("release c 4", st("-", (5, 3, 1, 2, 1, 0), live="4:1:4096", pending="5:0:256:1:1",
                           freed="2,1,3")),
        ("alloc d 256", st(6, (6, 3, 1, 2, 1, 0), live="4:1:4096,6:0:256",
                           pending="5:0:256:1:1", freed="2,1,3")),
        ("alloc e 256", st(5, (6, 3, 1, 2, 2, 0), idle=1, live="4:1:4096,5:0:256,6:0:256",
                           freed="2,1,3")),
        ("release d", st("-", (6, 3, 1, 2, 2, 0), cached=256, idle=1, live="4:1:4096,5:0:256",
                         free="6:0:256", freed="2,1,3")),
        ("release e", st("-", (6, 3, 1, 2, 2, 0), cached=512, idle=1, live="4:1:4096",
                         free="5:0:256,6:0:256", freed="2,1,3")),
        ("release keep", st("-", (6, 3, 1, 2, 2, 0), cached=4608, idle=1,
                            free="4:1:4096,5:0:256,6:0:256", freed="2,1,3")),
        ("trim", st("-", (6, 6, 1, 2, 2, 0), idle=1, freed="2,1,3,6,5,4")),
    ], knobs=(2, 1))


# ---------------------------------------------------------------------------- threads
def test_four_threads_under_tsan(exes):
    got = run(exes["tsan"], "pool", "threads", 4, 2000)
    assert got and got[0].startswith("ok "), got


def test_four_threads_under_asan(exes):
    got = run(exes["asan"], "pool", "threads", 4, 2000)
    assert got and got[0].startswith("ok "), got
