"""The readout's host-side work (kmer_hasher_amd/csrc/kmhg_hostwork.h) on the CPU, at shapes of a few
rows: the worker pool, the stripes, the run and pair-row expansions and the small pure helpers,
through tools/asan/host_check (ASan + UBSan) and host_check_tsan (ThreadSanitizer).  Both are
stand-alone programs built from the header the engine compiles.  Every expected value is computed
here with numpy or Python integers."""
import os
import subprocess

import numpy as np
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
    return r.stdout.split("\n")


BOTH = pytest.mark.parametrize("san", ["asan", "tsan"])


# ---------------------------------------------------------------------------- stripes
def stripes_closed_form(total, T, align):
    """T stripes of ceil(total / T) rounded up to align; the empty ones are not run."""
    stripe = -(-(-(-total // T)) // align) * align
    out = []
    for t in range(T):
        a, b = min(total, t * stripe), min(total, (t + 1) * stripe)
        if a < b:
            out.append(f"{a} {b}")
    return out


def test_stripes(exes):
    for align in (1, 512, 4096):
        for T in (1, 2, 3, 16):
            totals = {0, 1, align - 1, align, align + 1, T * align - 1, T * align + 1, 10_007}
            for total in sorted(totals):
                got = [l for l in run(exes["asan"], "stripes", total, T, align) if l]
                assert got == stripes_closed_form(total, T, align), (total, T, align)


# ---------------------------------------------------------------------------- runs
RUN_H = (1, 2, 511, 512, 513, 1537)


def run_lengths(H, shape, rng):
    if shape == "one":
        return [H]
    if shape == "ones":
        return [1] * H
    if shape == "boundary":      # runs that start on the 512-row stripe boundaries (H > 512)
        return [512] * ((H - 1) // 512) + [H - 512 * ((H - 1) // 512)]
    cuts = np.sort(rng.choice(np.arange(1, H), size=min(H - 1, int(rng.integers(1, 40))),
                              replace=False)) if H > 1 else np.empty(0, np.int64)
    return np.diff(np.concatenate(([0], cuts, [H]))).tolist()


def runs_case(H, shape, tmp_path):
    rng = np.random.default_rng(H * 7 + len(shape))
    ln = np.asarray(run_lengths(H, shape, rng), np.int64)
    assert ln.sum() == H and (ln > 0).all()
    st = np.cumsum(ln) - ln
    i0 = rng.integers(0, 1 << 30, ln.size)
    j0 = rng.integers(0, 1 << 30, ln.size)
    d = np.arange(H) - np.repeat(st, ln)
    want = np.stack([np.repeat(i0, ln) + d, np.repeat(j0, ln) + d], 1).astype(np.int32)
    path = str(tmp_path / f"runs_{H}_{shape}.bin")
    np.stack([st, i0, j0], 1).astype("<i4").tofile(path)
    return path, want


def rows_from(path, width):
    return np.fromfile(path, "<i4").reshape(-1, width)


@BOTH
@pytest.mark.parametrize("shape", ["one", "ones", "random", "boundary"])
def test_runs(exes, san, shape, tmp_path):
    out = str(tmp_path / "rows.bin")
    for H in RUN_H:
        path, want = runs_case(H, shape, tmp_path)
        for T in (1, 2, 3, 16):
            run(exes[san], "runs", path, H, T, out)
            assert np.array_equal(rows_from(out, 2), want), (H, shape, T)


@pytest.mark.parametrize("shape", ["one", "ones", "random", "boundary"])
def test_runs_every_cut(exes, shape, tmp_path):
    out = str(tmp_path / "rows.bin")
    for H in RUN_H:
        path, want = runs_case(H, shape, tmp_path)
        assert run(exes["asan"], "runs-split", path, H, out)[0] == f"ok {H + 1}"
        assert np.array_equal(rows_from(out, 2), want), (H, shape)


# ---------------------------------------------------------------------------- pairs
def pairs_case(ns, tmp_path, tag):
    """Repeated keys with ns[m] positions each among single-occurrence rows; the lists lie in the
    positions array in a shuffled order.  Returns the input paths and the expected rows."""
    rng = np.random.default_rng(len(ns))
    M = len(ns)
    U = 2 * M + 3
    pk = np.sort(rng.choice(U, M, replace=False)).astype(np.uint32)     # readout rows of the keys
    ri = np.zeros((U, 2), np.uint32)
    ri[:, 0] = 1
    ps = rng.integers(1, 1 << 30, int(np.sum(ns)) + 5).astype(np.int32)
    end = 2                                      # (a few entries no list uses, front and back)
    for m in rng.permutation(M):
        end += ns[m]
        ri[pk[m]] = (ns[m], end)
    counts = np.asarray(ns, np.uint64)
    po = np.concatenate(([0], np.cumsum(counts * (counts - 1) // 2)[:-1])).astype(np.uint64)
    want = []
    for m in range(M):
        n, e = int(ri[pk[m], 0]), int(ri[pk[m], 1])
        lst = ps[e - n:e]
        j, q = np.triu_indices(n, 1)
        want.append(np.stack([np.full(j.size, pk[m] + 1, np.int32), lst[j], lst[q]], 1))
    paths = []
    for name, a in (("pk", pk.astype("<u4")), ("po", po.astype("<u8")), ("ri", ri.astype("<u4")),
                    ("ps", ps.astype("<i4"))):
        paths.append(str(tmp_path / f"{tag}_{name}.bin"))
        a.tofile(paths[-1])
    return paths, np.concatenate(want)


@pytest.fixture(scope="module")
def pairs_full(tmp_path_factory):
    # every small list length around one key of 2,000 positions: 1,999,000 of ~2 M rows
    return pairs_case([2, 3, 64, 7, 4, 2000, 2, 64, 3, 7, 4], tmp_path_factory.mktemp("pairs"),
                      "full")


@BOTH
@pytest.mark.parametrize("T", [1, 3, 16])
def test_pairs(exes, san, T, pairs_full, tmp_path):
    paths, want = pairs_full
    out = str(tmp_path / "rows.bin")
    run(exes[san], "pairs", *paths, T, out)
    assert np.array_equal(rows_from(out, 3), want)


def test_pairs_every_cut(exes, tmp_path):
    paths, want = pairs_case([2, 3, 4, 7, 64, 2, 3, 7], tmp_path, "small")
    P = want.shape[0]
    assert 2000 < P <= 3000
    out = str(tmp_path / "rows.bin")
    assert run(exes["asan"], "pairs-split", *paths, out)[0] == f"ok {P + 1}"
    assert np.array_equal(rows_from(out, 3), want)


# ---------------------------------------------------------------------------- pair_start
def S(n, j):
    return j * (2 * n - j - 1) // 2


def pair_start_int(n, t):
    """The largest j in [0, n - 2] with S(j) <= t, by bisection on Python integers."""
    lo, hi = 0, n - 2
    while lo < hi:
        mid = (lo + hi + 1) // 2
        if S(n, mid) <= t:
            lo = mid
        else:
            hi = mid - 1
    return lo


def test_pair_start(exes, tmp_path):
    rng = np.random.default_rng(31)
    cases = []
    for n in (2, 3, 1000, 65_537, (1 << 24) + 1, (1 << 31) - 1):
        js = {0, 1, n // 2, n - 3, n - 2} | {int(x) for x in rng.integers(0, n - 1, 1000)}
        for j in sorted(js):
            if not 0 <= j <= n - 2:
                continue
            for t in (S(n, j) - 1, S(n, j), S(n, j) + 1):
                if 0 <= t < n * (n - 1) // 2:      # a key with n positions has n (n - 1) / 2 pairs
                    cases.append((n, t))
    path = str(tmp_path / "cases.txt")
    with open(path, "w") as f:
        f.writelines(f"{n} {t}\n" for n, t in cases)
    got = [int(l) for l in run(exes["asan"], "pair-start", path) if l]
    assert len(got) == len(cases)
    bad = [(n, t, g, pair_start_int(n, t)) for (n, t), g in zip(cases, got)
           if g != pair_start_int(n, t)]
    assert not bad, bad[:10]


# ---------------------------------------------------------------------------- pool
@BOTH
@pytest.mark.parametrize("fresh", [0, 1])
def test_pool_concurrent_callers(exes, san, fresh):
    assert run(exes[san], "pool", 4, 200, 40, fresh)[0] == "ok"


@BOTH
def test_pool_jobs_of_zero_and_one_task(exes, san):
    assert run(exes[san], "pool", 1, 2, 1, 0)[0] == "ok"      # its two jobs: 0 tasks, 1 task


# ---------------------------------------------------------------------------- the pure helpers
def test_misc(exes):
    MB2 = 2 << 20
    args, want = [], []
    for addr in (0, 1, 4096, MB2 - 1, MB2, MB2 + 1, 0x7F12_3456_7000):
        for nbytes in (0, 1, MB2, 2 * MB2 - 1, 2 * MB2, 2 * MB2 + 1, 3 * MB2, 80_000_000):
            a, b = -(-addr // MB2) * MB2, (addr + nbytes) // MB2 * MB2
            args.append(f"span={addr},{nbytes}")
            want.append(f"{a} {b - a}" if nbytes >= 2 * MB2 and b > a else "0 0")
    for b in (0, 1, 255, 256, 257, 1000, (1 << 20) - 1, 1 << 20, (1 << 20) + 1, MB2, MB2 + 1,
              5_000_000_000):
        args.append(f"class={b}")
        want.append(str(max(256, 1 << (b - 1).bit_length()) if b <= 1 << 20
                        else -(-b // MB2) * MB2))
    for nw in (0, 1, 7, 1000, 9_999_970, 499_999_970):
        args.append(f"cap={nw}")
        want.append(str((int(nw / 0.7) + 16 + 7) // 8 * 8))
    for s in (b"\0", b"A", b"AB\0", b"AB\0CD\0", b"ACGTACGT"):
        args.append(f"len={s.hex()}")
        want.append(str(s.index(0) if 0 in s else len(s)))
    got = [l for l in run(exes["asan"], "misc", *args) if l]
    assert got == want, [(a, g, w) for a, g, w in zip(args, got, want) if g != w]
