"""Release groups that adopt their owner's event (kmer_hasher_amd/csrc/kmhg_pool.h,
ReleaseGroupT::adopt) on the CPU: the pool over the fake device of tools/asan/host_check (ASan +
UBSan, a stand-alone program), as in test_pool_host.py.  `own_event <stream>` makes and records an
event that belongs to the script (the backend counts its create and its record like any other);
`adopt <event>` hands it to the open group.  The expected line after every operation is written
out from the pool's rules: blocks behind an adopted event are pending with owns = 0, the pool
records nothing for them, and the event never enters the pool's idle list."""
import os
import subprocess

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
ASAN = os.path.join(ROOT, "tools", "asan", "host_check")


@pytest.fixture(scope="module")
def exe():
    # flock: pytest-xdist workers each run this fixture; one make at a time
    r = subprocess.run(["flock", os.path.join(ROOT, "tools", "asan", ".build.lock"),
                        "make", "-s", "-C", os.path.join(ROOT, "tools", "asan"), "host_check"],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    return ASAN


def st(ret, calls, cached=0, idle=0, live="", free="", pending="", freed=""):
    """One expected line.  calls: the backend's allocs, frees, event creates, records, event waits
    and stream waits so far.  Blocks are id:device:class, pending ones id:device:class:event:owns."""
    a, f, c, r, ew, sw = calls
    return (f"ret={ret} allocs={a} frees={f} creates={c} records={r} ewaits={ew} swaits={sw} "
            f"cached={cached} idle={idle} dev=0 live={live} free={free} pending={pending} "
            f"freed={freed}")


def play(exe, tmp_path, steps):
    """steps: (operation, expected line).  Runs the script and compares line by line."""
    path = str(tmp_path / "pool.script")
    with open(path, "w") as f:
        f.writelines(op + "\n" for op, _ in steps)
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0:exitcode=99",
               UBSAN_OPTIONS="print_stacktrace=1")
    r = subprocess.run([exe, "pool", path], capture_output=True, text=True, env=env, timeout=300)
    assert r.returncode == 0, (r.returncode, r.stdout[-500:], r.stderr[-3000:])
    assert "Sanitizer" not in r.stderr and "runtime error" not in r.stderr, r.stderr[-3000:]
    got = [l for l in r.stdout.split("\n") if l]
    for i, ((op, want), g) in enumerate(zip(steps, got)):
        assert g == want, (i, op)
    assert len(got) == len(steps)
    last = dict(w.split("=", 1) for w in got[-1].split(" "))
    assert last["live"] == last["free"] == last["pending"] == "" and last["cached"] == "0"


def test_an_adopting_group_records_nothing_and_its_blocks_wait_for_the_event(exe, tmp_path):
    live = "1:0:256,2:0:512"
    pend = "1:0:256:1:0,2:0:512:1:0"
    play(exe, tmp_path, [
        ("alloc a 256", st(1, (1, 0, 0, 0, 0, 0), live="1:0:256")),
        ("alloc b 512", st(2, (2, 0, 0, 0, 0, 0), live=live)),
        ("group_begin 4", st("-", (2, 0, 0, 0, 0, 0), live=live)),
        ("release a 4", st("-", (2, 0, 0, 0, 0, 0), live=live)),
        ("release b 4", st("-", (2, 0, 0, 0, 0, 0), live=live)),
        # the script's own event: its create and its record are the only ones from here on
        ("own_event 4", st(1, (2, 0, 1, 1, 0, 0), live=live)),
        ("adopt 1", st("-", (2, 0, 1, 1, 0, 0), live=live)),
        ("group_end", st("-", (2, 0, 1, 1, 0, 0), pending=pend)),
        ("cached", st(0, (2, 0, 1, 1, 0, 0), pending=pend)),
        # not complete: a request of another class polls and leaves them pending
        ("alloc c 1024", st(3, (3, 0, 1, 1, 0, 0), live="3:0:1024", pending=pend)),
        ("complete 1", st("-", (3, 0, 1, 1, 0, 0), live="3:0:1024", pending=pend)),
        # the next request polls: both blocks are cached, and no event has become idle
        ("alloc d 2048", st(4, (4, 0, 1, 1, 0, 0), cached=768, live="3:0:1024,4:0:2048",
                            free=live)),
        ("alloc e 256", st(1, (4, 0, 1, 1, 0, 0), cached=512, live="1:0:256,3:0:1024,4:0:2048",
                           free="2:0:512")),
        # a later ordered release makes an event of the pool's own: the adopted one was not kept
        ("release e 4", st("-", (4, 0, 2, 2, 0, 0), cached=512, live="3:0:1024,4:0:2048",
                           free="2:0:512", pending="1:0:256:2:1")),
        ("release c", st("-", (4, 0, 2, 2, 0, 0), cached=1536, live="4:0:2048",
                         free="2:0:512,3:0:1024", pending="1:0:256:2:1")),
        ("release d", st("-", (4, 0, 2, 2, 0, 0), cached=3584,
                         free="2:0:512,3:0:1024,4:0:2048", pending="1:0:256:2:1")),
        ("trim", st("-", (4, 4, 2, 2, 1, 0), idle=1, freed="1,2,3,4")),
    ])


def test_an_adopted_event_that_completes_before_the_group_closes(exe, tmp_path):
    play(exe, tmp_path, [
        ("alloc a 256", st(1, (1, 0, 0, 0, 0, 0), live="1:0:256")),
        ("group_begin 4", st("-", (1, 0, 0, 0, 0, 0), live="1:0:256")),
        ("release a 4", st("-", (1, 0, 0, 0, 0, 0), live="1:0:256")),
        ("own_event 4", st(1, (1, 0, 1, 1, 0, 0), live="1:0:256")),
        ("adopt 1", st("-", (1, 0, 1, 1, 0, 0), live="1:0:256")),
        ("complete 1", st("-", (1, 0, 1, 1, 0, 0), live="1:0:256")),
        # still through pending: the group's end does not ask the event
        ("group_end", st("-", (1, 0, 1, 1, 0, 0), pending="1:0:256:1:0")),
        # the first request polls it back and takes it: no wait, no backend allocation
        ("alloc b 256", st(1, (1, 0, 1, 1, 0, 0), live="1:0:256")),
        ("release b", st("-", (1, 0, 1, 1, 0, 0), cached=256, free="1:0:256")),
        ("trim", st("-", (1, 1, 1, 1, 0, 0), freed="1")),
    ])


def test_a_nested_group_adopts_and_the_outer_one_records_its_own(exe, tmp_path):
    live = "1:0:256,2:0:512"
    play(exe, tmp_path, [
        ("alloc a 256", st(1, (1, 0, 0, 0, 0, 0), live="1:0:256")),
        ("alloc b 512", st(2, (2, 0, 0, 0, 0, 0), live=live)),
        ("group_begin 4", st("-", (2, 0, 0, 0, 0, 0), live=live)),
        ("release a 4", st("-", (2, 0, 0, 0, 0, 0), live=live)),        # the outer group's
        ("group_begin 4", st("-", (2, 0, 0, 0, 0, 0), live=live)),
        ("release b 4", st("-", (2, 0, 0, 0, 0, 0), live=live)),        # the inner group's
        ("own_event 4", st(1, (2, 0, 1, 1, 0, 0), live=live)),
        ("adopt 1", st("-", (2, 0, 1, 1, 0, 0), live=live)),
        ("group_end", st("-", (2, 0, 1, 1, 0, 0), live="1:0:256", pending="2:0:512:1:0")),
        # the outer group adopted nothing: the pool's event 2, owned by its last block
        ("group_end", st("-", (2, 0, 2, 2, 0, 0), pending="1:0:256:2:1,2:0:512:1:0")),
        ("complete 2", st("-", (2, 0, 2, 2, 0, 0), pending="1:0:256:2:1,2:0:512:1:0")),
        ("alloc c 1024", st(3, (3, 0, 2, 2, 0, 0), cached=256, idle=1, live="3:0:1024",
                            free="1:0:256", pending="2:0:512:1:0")),
        ("complete 1", st("-", (3, 0, 2, 2, 0, 0), cached=256, idle=1, live="3:0:1024",
                          free="1:0:256", pending="2:0:512:1:0")),
        ("release c", st("-", (3, 0, 2, 2, 0, 0), cached=1280, idle=1, free="1:0:256,3:0:1024",
                         pending="2:0:512:1:0")),
        ("cached", st(1280, (3, 0, 2, 2, 0, 0), cached=1280, idle=1, free="1:0:256,3:0:1024",
                      pending="2:0:512:1:0")),
        ("alloc d 2048", st(4, (4, 0, 2, 2, 0, 0), cached=1792, idle=1, live="4:0:2048",
                            free="1:0:256,2:0:512,3:0:1024")),
        ("release d", st("-", (4, 0, 2, 2, 0, 0), cached=3840, idle=1,
                         free="1:0:256,2:0:512,3:0:1024,4:0:2048")),
        ("trim", st("-", (4, 4, 2, 2, 0, 0), idle=1, freed="1,2,3,4")),
    ])


def test_trim_waits_for_adopted_entries_and_keeps_no_event(exe, tmp_path):
    live = "1:0:256,2:0:512"
    pend = "1:0:256:1:0,2:0:512:1:0"
    play(exe, tmp_path, [
        ("alloc a 256", st(1, (1, 0, 0, 0, 0, 0), live="1:0:256")),
        ("alloc b 512", st(2, (2, 0, 0, 0, 0, 0), live=live)),
        ("group_begin 4", st("-", (2, 0, 0, 0, 0, 0), live=live)),
        ("release a 4", st("-", (2, 0, 0, 0, 0, 0), live=live)),
        ("release b 4", st("-", (2, 0, 0, 0, 0, 0), live=live)),
        ("own_event 4", st(1, (2, 0, 1, 1, 0, 0), live=live)),
        ("adopt 1", st("-", (2, 0, 1, 1, 0, 0), live=live)),
        ("group_end", st("-", (2, 0, 1, 1, 0, 0), pending=pend)),
        # one wait per pending entry, both blocks freed, the idle list still empty
        ("trim", st("-", (2, 2, 1, 1, 2, 0), freed="1,2")),
        ("cached", st(0, (2, 2, 1, 1, 2, 0), freed="1,2")),
    ])


def test_the_depth_1_wait_takes_an_adopted_entry(exe, tmp_path):
    play(exe, tmp_path, [
        ("alloc a 4096", st(1, (1, 0, 0, 0, 0, 0), live="1:0:4096")),
        ("group_begin 9", st("-", (1, 0, 0, 0, 0, 0), live="1:0:4096")),
        ("release a 9", st("-", (1, 0, 0, 0, 0, 0), live="1:0:4096")),
        ("own_event 9", st(1, (1, 0, 1, 1, 0, 0), live="1:0:4096")),
        ("adopt 1", st("-", (1, 0, 1, 1, 0, 0), live="1:0:4096")),
        ("group_end", st("-", (1, 0, 1, 1, 0, 0), pending="1:0:4096:1:0")),
        # the class has its one block: the request waits for the adopted event and gets it back;
        # the event does not become one of the pool's
        ("alloc b 4096", st(1, (1, 0, 1, 1, 1, 0), live="1:0:4096")),
        # so the pool makes its own for the next ordered release
        ("release b 9", st("-", (1, 0, 2, 2, 1, 0), pending="1:0:4096:2:1")),
        ("trim", st("-", (1, 1, 2, 2, 2, 0), idle=1, freed="1")),
    ])
