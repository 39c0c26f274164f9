"""Same-stream block reuse and the run-ahead bound (kmer_hasher_amd/csrc/kmhg_pool.h) on the CPU,
over the fake device of tools/asan/host_check (ASan + UBSan) and host_check_tsan, like
tests/test_pool_host.py: each scenario is a script of operations and, written out here from the
pool's rules, the line of state expected after every one.

The rules: a pending block remembers the stream it was released behind.  alloc_on (a request
that names the stream of its first use) takes a free block of its class, else the oldest pending
block of its class released behind that very stream -- with no event wait and no event query --
else it behaves like alloc: poll (each distinct event queried once), depth rule, host wait.  A
taken block that owned its batch's event passes it to the first block still pending behind it;
the last one returns it to the idle events.  An adopted event is nobody's to return.  RecordPool
hands out records and waits for the oldest pending one's event once `ahead` are pending."""
import itertools
import os
import subprocess

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
ASAN = os.path.join(ROOT, "tools", "asan", "host_check")
TSAN = os.path.join(ROOT, "tools", "asan", "host_check_tsan")


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


def fields(line):
    return dict(w.split("=", 1) for w in line.split(" "))


def play(exes, tmp_path, steps, knobs=None):
    """steps: (operation, expected line).  Runs the script and compares line by line; at the end
    every block is freed and every block was in exactly one state throughout."""
    path = str(tmp_path / "pool.script")
    with open(path, "w") as f:
        if knobs:
            f.write("knobs %d %d\n" % knobs)
        f.writelines(op + "\n" for op, _ in steps)
    got = run(exes["asan"], "pool", path)
    for i, ((op, want), g) in enumerate(zip(steps, got)):
        assert g == want, (i, op)
    assert len(got) == len(steps)
    for l in got:
        f = fields(l)
        sets = {n: [b.split(":") for b in f[n].split(",") if b] for n in ("live", "free", "pending")}
        freed = [int(x) for x in f["freed"].split(",") if x]
        ids = [int(b[0]) for v in sets.values() for b in v] + freed
        assert sorted(ids) == list(range(1, len(ids) + 1)), l   # exactly one state per block
        assert int(f["cached"]) == sum(int(b[2]) for b in sets["free"]), l
    assert f["live"] == f["free"] == f["pending"] == "" and f["cached"] == "0", got[-1]
    return got


# ---------------------------------------------------------------------------- same stream
def test_same_stream_takes_the_pending_block_without_wait_or_query(exes, tmp_path):
    play(exes, tmp_path, [
        ("alloc a 4096", st(1, (1, 0, 0, 0, 0, 0), live="1:0:4096")),
        ("release a 9", st("-", (1, 0, 1, 1, 0, 0), pending="1:0:4096:1:1")),
        # the same block, at once; its event is idle again
        ("alloc_on b 4096 9", st(1, (1, 0, 1, 1, 0, 0), idle=1, live="1:0:4096")),
        ("dones", st(0, (1, 0, 1, 1, 0, 0), idle=1, live="1:0:4096")),
        # ... and recycled: no second create
        ("release b 9", st("-", (1, 0, 1, 2, 0, 0), pending="1:0:4096:1:1")),
        ("alloc_on c 4096 9", st(1, (1, 0, 1, 2, 0, 0), idle=1, live="1:0:4096")),
        ("dones", st(0, (1, 0, 1, 2, 0, 0), idle=1, live="1:0:4096")),
        ("release c", st("-", (1, 0, 1, 2, 0, 0), cached=4096, idle=1, free="1:0:4096")),
        ("trim", st("-", (1, 1, 1, 2, 0, 0), idle=1, freed="1")),
    ])


def test_the_null_stream_is_a_stream_like_any_other(exes, tmp_path):
    play(exes, tmp_path, [
        ("alloc a 4096", st(1, (1, 0, 0, 0, 0, 0), live="1:0:4096")),
        ("release a 0", st("-", (1, 0, 1, 1, 0, 0), pending="1:0:4096:1:1")),
        ("alloc_on b 4096 0", st(1, (1, 0, 1, 1, 0, 0), idle=1, live="1:0:4096")),
        ("release b 0", st("-", (1, 0, 1, 2, 0, 0), pending="1:0:4096:1:1")),
        # no stream named: the host wait, although the block sits behind stream 0
        ("alloc c 4096", st(1, (1, 0, 1, 2, 1, 0), idle=1, live="1:0:4096")),
        ("release c", st("-", (1, 0, 1, 2, 1, 0), cached=4096, idle=1, free="1:0:4096")),
        ("trim", st("-", (1, 1, 1, 2, 1, 0), idle=1, freed="1")),
    ])


def test_another_stream_and_no_stream_wait_as_before(exes, tmp_path):
    play(exes, tmp_path, [
        ("alloc a 4096", st(1, (1, 0, 0, 0, 0, 0), live="1:0:4096")),
        ("release a 9", st("-", (1, 0, 1, 1, 0, 0), pending="1:0:4096:1:1")),
        # first used on stream 7: one query (the poll), one event wait
        ("alloc_on b 4096 7", st(1, (1, 0, 1, 1, 1, 0), idle=1, live="1:0:4096")),
        ("dones", st(1, (1, 0, 1, 1, 1, 0), idle=1, live="1:0:4096")),
        ("release b 9", st("-", (1, 0, 1, 2, 1, 0), pending="1:0:4096:1:1")),
        # no stream
        ("alloc c 4096", st(1, (1, 0, 1, 2, 2, 0), idle=1, live="1:0:4096")),
        ("dones", st(2, (1, 0, 1, 2, 2, 0), idle=1, live="1:0:4096")),
        ("release c", st("-", (1, 0, 1, 2, 2, 0), cached=4096, idle=1, free="1:0:4096")),
        ("trim", st("-", (1, 1, 1, 2, 2, 0), idle=1, freed="1")),
    ])


def test_of_two_pending_blocks_the_requests_own_stream_serves(exes, tmp_path):
    play(exes, tmp_path, [
        ("alloc a 4096", st(1, (1, 0, 0, 0, 0, 0), live="1:0:4096")),
        ("alloc b 4096", st(2, (2, 0, 0, 0, 0, 0), live="1:0:4096,2:0:4096")),
        ("release a 7", st("-", (2, 0, 1, 1, 0, 0), live="2:0:4096", pending="1:0:4096:1:1")),
        ("release b 9", st("-", (2, 0, 2, 2, 0, 0), pending="1:0:4096:1:1,2:0:4096:2:1")),
        # b's, although a is the older one
        ("alloc_on c 4096 9", st(2, (2, 0, 2, 2, 0, 0), idle=1, live="2:0:4096",
                                 pending="1:0:4096:1:1")),
        # a second request on 9 finds only stream 7's: it waits for it, and does not grow the pool
        ("alloc_on d 4096 9", st(1, (2, 0, 2, 2, 1, 0), idle=2, live="1:0:4096,2:0:4096")),
        # another class, another device: nothing of theirs is pending, they allocate
        ("alloc_on e 8192 9", st(3, (3, 0, 2, 2, 1, 0), idle=2,
                                 live="1:0:4096,2:0:4096,3:0:8192")),
        # (the idle event taken is the one returned last: event 1)
        ("release c 9", st("-", (3, 0, 2, 3, 1, 0), idle=1, live="1:0:4096,3:0:8192",
                           pending="2:0:4096:1:1")),
        ("dev 1", st("-", (3, 0, 2, 3, 1, 0), dev=1, idle=1, live="1:0:4096,3:0:8192",
                     pending="2:0:4096:1:1")),
        ("alloc_on f 4096 9", st(4, (4, 0, 2, 3, 1, 0), dev=1, idle=1,
                                 live="1:0:4096,3:0:8192,4:1:4096", pending="2:0:4096:1:1")),
        ("release f", st("-", (4, 0, 2, 3, 1, 0), dev=1, cached=4096, idle=1,
                         live="1:0:4096,3:0:8192", free="4:1:4096", pending="2:0:4096:1:1")),
        ("dev 0", st("-", (4, 0, 2, 3, 1, 0), cached=4096, idle=1, live="1:0:4096,3:0:8192",
                     free="4:1:4096", pending="2:0:4096:1:1")),
        ("release d", st("-", (4, 0, 2, 3, 1, 0), cached=8192, idle=1, live="3:0:8192",
                         free="1:0:4096,4:1:4096", pending="2:0:4096:1:1")),
        ("release e", st("-", (4, 0, 2, 3, 1, 0), cached=16384, idle=1,
                         free="1:0:4096,3:0:8192,4:1:4096", pending="2:0:4096:1:1")),
        ("trim", st("-", (4, 4, 2, 3, 2, 0), idle=2, freed="1,2,3,4")),
    ])


def test_a_free_block_is_taken_before_a_pending_one_and_without_a_poll(exes, tmp_path):
    play(exes, tmp_path, [
        ("alloc a 4096", st(1, (1, 0, 0, 0, 0, 0), live="1:0:4096")),
        ("alloc b 4096", st(2, (2, 0, 0, 0, 0, 0), live="1:0:4096,2:0:4096")),
        ("release a 9", st("-", (2, 0, 1, 1, 0, 0), live="2:0:4096", pending="1:0:4096:1:1")),
        ("release b", st("-", (2, 0, 1, 1, 0, 0), cached=4096, free="2:0:4096",
                         pending="1:0:4096:1:1")),
        ("complete 1", st("-", (2, 0, 1, 1, 0, 0), cached=4096, free="2:0:4096",
                          pending="1:0:4096:1:1")),
        # the free one; the completed event is not even looked at
        ("alloc_on c 4096 9", st(2, (2, 0, 1, 1, 0, 0), live="2:0:4096", pending="1:0:4096:1:1")),
        ("dones", st(0, (2, 0, 1, 1, 0, 0), live="2:0:4096", pending="1:0:4096:1:1")),
        ("release c", st("-", (2, 0, 1, 1, 0, 0), cached=4096, free="2:0:4096",
                         pending="1:0:4096:1:1")),
        ("trim", st("-", (2, 2, 1, 1, 1, 0), idle=1, freed="2,1")),
    ])


# ---------------------------------------------------------------------------- shared events
NAMES = {"a": (1, 256), "b": (2, 512), "c": (3, 1024)}


@pytest.mark.parametrize("order", list(itertools.permutations("abc")))
def test_a_group_of_3_taken_in_every_order_returns_its_event_once(exes, tmp_path, order):
    live3 = "1:0:256,2:0:512,3:0:1024"
    steps = [
        ("alloc a 256", st(1, (1, 0, 0, 0, 0, 0), live="1:0:256")),
        ("alloc b 512", st(2, (2, 0, 0, 0, 0, 0), live="1:0:256,2:0:512")),
        ("alloc c 1024", st(3, (3, 0, 0, 0, 0, 0), live=live3)),
        ("group_begin 4", st("-", (3, 0, 0, 0, 0, 0), live=live3)),
        ("release a 4", st("-", (3, 0, 0, 0, 0, 0), live=live3)),
        ("release b 4", st("-", (3, 0, 0, 0, 0, 0), live=live3)),
        ("release c 4", st("-", (3, 0, 0, 0, 0, 0), live=live3)),
        # the last one queued owns the one event
        ("group_end", st("-", (3, 0, 1, 1, 0, 0),
                         pending="1:0:256:1:0,2:0:512:1:0,3:0:1024:1:1")),
    ]
    pend, owner, live = ["a", "b", "c"], "c", []
    for n in order:
        pend.remove(n)
        live.append(n)
        if n == owner:                 # passed on to the first block still behind it
            owner = pend[0] if pend else None
        want_p = ",".join("%d:0:%d:1:%d" % (*NAMES[x], x == owner) for x in pend)
        want_l = ",".join("%d:0:%d" % NAMES[x] for x in sorted(live))
        steps.append((f"alloc_on x{n} {NAMES[n][1]} 4",
                      st(NAMES[n][0], (3, 0, 1, 1, 0, 0), idle=0 if pend else 1, live=want_l,
                         pending=want_p)))
    steps += [
        ("dones", st(0, (3, 0, 1, 1, 0, 0), idle=1, live=live3)),
        ("release xa", st("-", (3, 0, 1, 1, 0, 0), cached=256, idle=1, live="2:0:512,3:0:1024",
                          free="1:0:256")),
        ("release xb", st("-", (3, 0, 1, 1, 0, 0), cached=768, idle=1, live="3:0:1024",
                          free="1:0:256,2:0:512")),
        # the returned event serves the next release: still one create
        ("release xc 4", st("-", (3, 0, 1, 2, 0, 0), cached=768, free="1:0:256,2:0:512",
                            pending="3:0:1024:1:1")),
        ("trim", st("-", (3, 3, 1, 2, 1, 0), idle=1, freed="1,2,3")),
    ]
    play(exes, tmp_path, steps)


def test_two_classes_two_groups_and_a_wait_in_between(exes, tmp_path):
    """Two blocks of one class and one of another behind one event; a second group on another
    stream; the owner taken by the waiting path while its siblings are still pending."""
    l4 = "1:0:256,2:0:256,3:0:512,4:0:512"
    play(exes, tmp_path, [
        ("alloc a 256", st(1, (1, 0, 0, 0, 0, 0), live="1:0:256")),
        ("alloc b 256", st(2, (2, 0, 0, 0, 0, 0), live="1:0:256,2:0:256")),
        ("alloc c 512", st(3, (3, 0, 0, 0, 0, 0), live="1:0:256,2:0:256,3:0:512")),
        ("alloc d 512", st(4, (4, 0, 0, 0, 0, 0), live=l4)),
        ("group_begin 4", st("-", (4, 0, 0, 0, 0, 0), live=l4)),
        ("release a 4", st("-", (4, 0, 0, 0, 0, 0), live=l4)),
        ("release b 4", st("-", (4, 0, 0, 0, 0, 0), live=l4)),
        ("release c 4", st("-", (4, 0, 0, 0, 0, 0), live=l4)),
        ("group_end", st("-", (4, 0, 1, 1, 0, 0), live="4:0:512",
                         pending="1:0:256:1:0,2:0:256:1:0,3:0:512:1:1")),
        ("release d 5", st("-", (4, 0, 2, 2, 0, 0),
                           pending="1:0:256:1:0,2:0:256:1:0,3:0:512:1:1,4:0:512:2:1")),
        # 512 B on stream 5: d, whose event returns (it was alone behind it)
        ("alloc_on p 512 5", st(4, (4, 0, 2, 2, 0, 0), idle=1, live="4:0:512",
                                pending="1:0:256:1:0,2:0:256:1:0,3:0:512:1:1")),
        # 512 B with no stream: waits for c, the owner; its event has completed, so it returns
        # although a and b are still listed behind it (a later poll finds them done, or waiting
        # for later work: both safe)
        ("alloc q 512", st(3, (4, 0, 2, 2, 1, 0), idle=2, live="3:0:512,4:0:512",
                           pending="1:0:256:1:0,2:0:256:1:0")),
        # 256 B on stream 4, twice: the older first; nobody owns event 1 any more
        ("alloc_on r 256 4", st(1, (4, 0, 2, 2, 1, 0), idle=2, live="1:0:256,3:0:512,4:0:512",
                                pending="2:0:256:1:0")),
        ("alloc_on s 256 4", st(2, (4, 0, 2, 2, 1, 0), idle=2, live=l4)),
        ("release p", st("-", (4, 0, 2, 2, 1, 0), cached=512, idle=2,
                         live="1:0:256,2:0:256,3:0:512", free="4:0:512")),
        ("release q", st("-", (4, 0, 2, 2, 1, 0), cached=1024, idle=2, live="1:0:256,2:0:256",
                         free="3:0:512,4:0:512")),
        ("release r", st("-", (4, 0, 2, 2, 1, 0), cached=1280, idle=2, live="2:0:256",
                         free="1:0:256,3:0:512,4:0:512")),
        ("release s", st("-", (4, 0, 2, 2, 1, 0), cached=1536, idle=2,
                         free="1:0:256,2:0:256,3:0:512,4:0:512")),
        ("trim", st("-", (4, 4, 2, 2, 1, 0), idle=2, freed="1,2,4,3")),
    ])


def test_an_adopted_event_is_never_the_pools(exes, tmp_path):
    live = "1:0:256,2:0:512"
    play(exes, tmp_path, [
        ("alloc a 256", st(1, (1, 0, 0, 0, 0, 0), live="1:0:256")),
        ("alloc b 512", st(2, (2, 0, 0, 0, 0, 0), live=live)),
        ("group_begin 4", st("-", (2, 0, 0, 0, 0, 0), live=live)),
        ("release a 4", st("-", (2, 0, 0, 0, 0, 0), live=live)),
        ("release b 4", st("-", (2, 0, 0, 0, 0, 0), live=live)),
        ("own_event 4", st(1, (2, 0, 1, 1, 0, 0), live=live)),
        ("adopt 1", st("-", (2, 0, 1, 1, 0, 0), live=live)),
        ("group_end", st("-", (2, 0, 1, 1, 0, 0), pending="1:0:256:1:0,2:0:512:1:0")),
        ("alloc_on x 512 4", st(2, (2, 0, 1, 1, 0, 0), live="2:0:512", pending="1:0:256:1:0")),
        ("alloc_on y 256 4", st(1, (2, 0, 1, 1, 0, 0), live=live)),
        ("dones", st(0, (2, 0, 1, 1, 0, 0), live=live)),
        # the pool has no event of its own: the next ordered release makes one
        ("release x 4", st("-", (2, 0, 2, 2, 0, 0), live="1:0:256", pending="2:0:512:2:1")),
        ("release y", st("-", (2, 0, 2, 2, 0, 0), cached=256, free="1:0:256",
                         pending="2:0:512:2:1")),
        ("trim", st("-", (2, 2, 2, 2, 1, 0), idle=1, freed="1,2")),
    ])


def test_a_release_that_cannot_record_waits_for_the_stream(exes, tmp_path):
    play(exes, tmp_path, [
        ("alloc a 256", st(1, (1, 0, 0, 0, 0, 0), live="1:0:256")),
        ("fail record 1", st("-", (1, 0, 0, 0, 0, 0), live="1:0:256")),
        # the stream is waited for and the block is free at once, its event kept
        ("release a 4", st("-", (1, 0, 1, 1, 0, 1), cached=256, idle=1, free="1:0:256")),
        ("alloc_on b 256 4", st(1, (1, 0, 1, 1, 0, 1), idle=1, live="1:0:256")),
        ("fail event 1", st("-", (1, 0, 1, 1, 0, 1), idle=1, live="1:0:256")),
        # (the idle event serves: no create to fail)
        ("release b 4", st("-", (1, 0, 1, 2, 0, 1), live="", pending="1:0:256:1:1")),
        ("alloc_on c 256 4", st(1, (1, 0, 1, 2, 0, 1), idle=1, live="1:0:256")),
        ("alloc d 512", st(2, (2, 0, 1, 2, 0, 1), idle=1, live="1:0:256,2:0:512")),
        # no event can be made for this one: the stream wait again
        ("release d 4", st("-", (2, 0, 1, 3, 0, 1), live="1:0:256", pending="2:0:512:1:1")),
        ("release c 4", st("-", (2, 0, 2, 3, 0, 2), cached=256, free="1:0:256",
                           pending="2:0:512:1:1")),
        ("alloc_on e 256 4", st(1, (2, 0, 2, 3, 0, 2), live="1:0:256", pending="2:0:512:1:1")),
        ("release e", st("-", (2, 0, 2, 3, 0, 2), cached=256, free="1:0:256",
                         pending="2:0:512:1:1")),
        ("dones", st(0, (2, 0, 2, 3, 0, 2), cached=256, free="1:0:256", pending="2:0:512:1:1")),
        ("trim", st("-", (2, 2, 2, 3, 1, 2), idle=1, freed="1,2")),
    ])


def test_a_poll_queries_each_event_once(exes, tmp_path):
    live = "1:0:256,2:0:512,3:0:1024"
    pend = "1:0:256:1:0,2:0:512:1:0,3:0:1024:1:1"
    play(exes, tmp_path, [
        ("alloc a 256", st(1, (1, 0, 0, 0, 0, 0), live="1:0:256")),
        ("alloc b 512", st(2, (2, 0, 0, 0, 0, 0), live="1:0:256,2:0:512")),
        ("alloc c 1024", st(3, (3, 0, 0, 0, 0, 0), live=live)),
        ("group_begin 4", st("-", (3, 0, 0, 0, 0, 0), live=live)),
        ("release a 4", st("-", (3, 0, 0, 0, 0, 0), live=live)),
        ("release b 4", st("-", (3, 0, 0, 0, 0, 0), live=live)),
        ("release c 4", st("-", (3, 0, 0, 0, 0, 0), live=live)),
        ("group_end", st("-", (3, 0, 1, 1, 0, 0), pending=pend)),
        # three blocks behind one event: one query
        ("alloc d 2048", st(4, (4, 0, 1, 1, 0, 0), live="4:0:2048", pending=pend)),
        ("dones", st(1, (4, 0, 1, 1, 0, 0), live="4:0:2048", pending=pend)),
        ("complete 1", st("-", (4, 0, 1, 1, 0, 0), live="4:0:2048", pending=pend)),
        ("alloc e 4096", st(5, (5, 0, 1, 1, 0, 0), cached=1792, idle=1, live="4:0:2048,5:0:4096",
                            free=live)),
        ("dones", st(2, (5, 0, 1, 1, 0, 0), cached=1792, idle=1, live="4:0:2048,5:0:4096",
                     free=live)),
        ("release d", st("-", (5, 0, 1, 1, 0, 0), cached=3840, idle=1, live="5:0:4096",
                         free=live + ",4:0:2048")),
        ("release e", st("-", (5, 0, 1, 1, 0, 0), cached=7936, idle=1,
                         free=live + ",4:0:2048,5:0:4096")),
        ("trim", st("-", (5, 5, 1, 1, 0, 0), idle=1, freed="1,2,3,4,5")),
    ])


def test_a_block_retaken_1000_times_on_one_stream_stays_the_only_one(exes, tmp_path):
    steps = [("alloc a 4096", None)]
    for _ in range(1000):
        steps += [("release a 9", None), ("alloc_on a 4096 9", None)]
    steps += [("dones", None), ("release a", None), ("trim", None)]
    path = str(tmp_path / "pool.script")
    with open(path, "w") as f:
        f.writelines(op + "\n" for op, _ in steps)
    got = run(exes["asan"], "pool", path)
    assert len(got) == len(steps)
    for i in range(1000):
        assert got[1 + 2 * i] == st("-", (1, 0, 1, 1 + i, 0, 0), pending="1:0:4096:1:1"), i
        assert got[2 + 2 * i] == st(1, (1, 0, 1, 1 + i, 0, 0), idle=1, live="1:0:4096"), i
    assert got[-3] == st(0, (1, 0, 1, 1000, 0, 0), idle=1, live="1:0:4096")
    assert got[-1] == st("-", (1, 1, 1, 1000, 0, 0), idle=1, freed="1")


# ---------------------------------------------------------------------------- run-ahead
def rec(ev, free, pending):
    return f"{ev}:{free}:{pending}"


def test_the_third_unfinished_take_waits_for_the_oldest(exes, tmp_path):
    # records come four at a time (events 1..4), the last made handed out first
    play(exes, tmp_path, [
        ("rec_take r1", st(rec(4, 3, 0), (0, 0, 4, 0, 0, 0))),
        ("rec_give r1 5", st("-", (0, 0, 4, 1, 0, 0))),
        ("rec_take r2", st(rec(3, 2, 1), (0, 0, 4, 1, 0, 0))),
        ("rec_give r2 5", st("-", (0, 0, 4, 2, 0, 0))),
        # two in flight: event 4, the older, is waited for, and its record is the one handed out
        ("rec_take r3", st(rec(4, 2, 1), (0, 0, 4, 2, 1, 0))),
        ("dones", st(3, (0, 0, 4, 2, 1, 0))),
        ("rec_give r3 5", st("-", (0, 0, 4, 3, 1, 0))),
        # a completed one is found by the poll: no wait
        ("complete 3", st("-", (0, 0, 4, 3, 1, 0))),
        ("rec_take r4", st(rec(3, 2, 1), (0, 0, 4, 3, 1, 0))),
        # given back after a wait of the caller's: free at once, whatever is in flight
        ("rec_give r4", st("-", (0, 0, 4, 3, 1, 0))),
        ("rec_take r5", st(rec(3, 2, 1), (0, 0, 4, 3, 1, 0))),
        ("rec_give r5 5", st("-", (0, 0, 4, 4, 1, 0))),
        ("rec_take r6", st(rec(4, 2, 1), (0, 0, 4, 4, 2, 0))),
    ])


def test_ahead_1_waits_at_the_second_take_and_ahead_3_at_the_fourth(exes, tmp_path):
    play(exes, tmp_path, [
        ("ahead 1", st("-", (0, 0, 0, 0, 0, 0))),
        ("rec_take r1", st(rec(4, 3, 0), (0, 0, 4, 0, 0, 0))),
        ("rec_give r1 5", st("-", (0, 0, 4, 1, 0, 0))),
        ("rec_take r2", st(rec(4, 3, 0), (0, 0, 4, 1, 1, 0))),
    ])
    play(exes, tmp_path, [
        ("ahead 3", st("-", (0, 0, 0, 0, 0, 0))),
        ("rec_take r1", st(rec(4, 3, 0), (0, 0, 4, 0, 0, 0))),
        ("rec_give r1 5", st("-", (0, 0, 4, 1, 0, 0))),
        ("rec_take r2", st(rec(3, 2, 1), (0, 0, 4, 1, 0, 0))),
        ("rec_give r2 5", st("-", (0, 0, 4, 2, 0, 0))),
        ("rec_take r3", st(rec(2, 1, 2), (0, 0, 4, 2, 0, 0))),
        ("rec_give r3 5", st("-", (0, 0, 4, 3, 0, 0))),
        ("rec_take r4", st(rec(4, 1, 2), (0, 0, 4, 3, 1, 0))),
    ])


# ---------------------------------------------------------------------------- threads
def test_four_threads_each_on_its_own_stream_under_tsan(exes):
    got = run(exes["tsan"], "pool", "stream-threads", 4, 2000)
    assert got and got[0].startswith("ok "), got


def test_four_threads_each_on_its_own_stream_under_asan(exes):
    got = run(exes["asan"], "pool", "stream-threads", 4, 2000)
    assert got and got[0].startswith("ok "), got
