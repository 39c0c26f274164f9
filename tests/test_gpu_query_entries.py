"""Every exported query entry on one tiny index, rows compared exactly with the oracle: the two
host-pointer entries, the device entry, the range and range-runs entries with their reverse-strand
twins, and the part entry.  All of them are one path over a QueryCall (kmhg_querycall.h) that names
the range and the modes, so a flag that reached the wrong mode shows here as wrong rows: rc rows
where forward ones belong, runs where rows were asked, a part's tile offsets on a whole index.

The index: 3,000 seeded bases with a 400-base poly-A stretch and a run of N, k = 8.  The queries:
the sequence itself (393 poly-A windows x 393 positions: far more rows than the guessed capacity,
so the rows are emitted a second time into an exact buffer; every one of them its own run), 300
unrelated bases (a few chance rows, fewer than the guess, runs do not pay) and a 600-base copy of
an index stretch (one long diagonal: runs pay).  Integer work: every comparison is exact."""
import ctypes as C

import numpy as np
import pytest

from oracle import oracle as O
from revcomp_ref import rc_host

pytestmark = pytest.mark.gpu

K = 8
_D = {}


def _data():
    """The sequences and the oracle's rows, computed once: want[name][rc] is (H, 2)."""
    if not _D:
        rng = np.random.default_rng(20)
        acgt = np.frombuffer(b"ACGT", np.uint8)
        s = acgt[rng.integers(0, 4, 3000)]
        s[800:1200] = ord("A")
        s[2000:2010] = ord("N")
        queries = {"self": s, "unrelated": acgt[np.random.default_rng(28).integers(0, 4, 300)],
                   "copy": s[1300:1900].copy()}
        oi = O.OracleIndex(s, K)
        want = {n: {rc: oi.query(rc_host(q) if rc else q, K).reshape(-1, 2) for rc in (0, 1)}
                for n, q in queries.items()}
        _D.update(s=s, queries=queries, want=want)
    return _D


def _n_runs(rows):
    """The runs of a range's rows as the runs entries count them: a window with several rows
    starts one run per row; a window with one row (i, j) goes on with the run of the window before
    it when that one's only row is (i - 1, j - 1)."""
    if not len(rows):
        return 0
    i, j = rows[:, 0].astype(np.int64), rows[:, 1].astype(np.int64)
    _, inv, cnt = np.unique(i, return_inverse=True, return_counts=True)
    single = cnt[inv] == 1
    go_on = single[1:] & single[:-1] & (i[1:] == i[:-1] + 1) & (j[1:] == j[:-1] + 1)
    return len(rows) - int(go_on.sum())


def _host_rows(idx, q, rc):
    from kmer_hasher_amd import _lib
    L = _lib.lib()
    h, n = C.c_void_p(), C.c_int64()
    fn = L.kmhg_query_run_rc if rc else L.kmhg_query_run
    b = q.tobytes()
    _lib.check(fn(idx.handle, b, len(b), K, C.byref(h), C.byref(n)))
    out = np.full((n.value, 2), -1, np.int32)
    _lib.check(L.kmhg_query_fill(h, out.ctypes.data_as(C.c_void_p)))
    L.kmhg_query_free(h)
    return out


def _rows(q):
    r = q.rows().cpu().numpy()
    q.free()
    return r


def _runs_rows(torch, got, want):
    """A runs entry's answer as rows, after checking that it chose runs exactly when they pay."""
    from kmer_hasher_amd.device import runs_expand
    kind, t, h = got
    H, NR = len(want), _n_runs(want)
    assert h == H
    assert (kind == "runs") == (H > 0 and 3 * NR < 2 * H), (kind, H, NR)
    if kind == "rows":
        return t.cpu().numpy()
    assert t.shape[0] == NR
    out = torch.full((h, 2), -1, dtype=torch.int32, device="cuda")
    runs_expand(t, h, out)
    return out.cpu().numpy()


@pytest.fixture(scope="module")
def index(gpu):
    from kmer_hasher_amd.device import DeviceIndex
    idx = DeviceIndex.build(gpu.from_numpy(_data()["s"].copy()).cuda(), K)
    yield idx
    idx.free()


def test_the_queries_take_the_paths_they_are_meant_to():
    d = _data()
    shape = {n: (len(q) - K + 1, len(d["want"][n][0]), _n_runs(d["want"][n][0]))
             for n, q in d["queries"].items()}
    guess = {n: nw + nw // 8 + 64 for n, (nw, _, _) in shape.items()}
    nw, H, NR = shape["self"]
    assert H > 393 * 393 > guess["self"] and not 3 * NR < 2 * H      # the exact redo; rows
    nw, H, NR = shape["unrelated"]
    assert 0 < H <= guess["unrelated"] and not 3 * NR < 2 * H
    nw, H, NR = shape["copy"]
    assert H >= nw and 3 * NR < 2 * H                                # runs
    for n in shape:
        assert len(d["want"][n][1]) > 0 and not np.array_equal(d["want"][n][0], d["want"][n][1])


@pytest.mark.parametrize("rc", [0, 1], ids=["fwd", "rc"])
@pytest.mark.parametrize("name", ["self", "unrelated", "copy"])
def test_every_entry_equals_the_oracle(gpu, index, name, rc):
    torch = gpu
    d = _data()
    q, want = d["queries"][name], d["want"][name][rc]
    t = torch.from_numpy(q.copy()).cuda()
    nw = len(q) - K + 1
    assert np.array_equal(_host_rows(index, q, rc), want), "host entry"
    whole = index.query_rc(t, K) if rc else index.query(t, K)
    assert np.array_equal(_rows(whole), want), "device entry"
    rng_q = index.query_range_rc if rc else index.query_range
    rng_r = index.query_range_runs_rc if rc else index.query_range_runs
    assert np.array_equal(_rows(rng_q(t, K, 0, nw)), want), "full range"
    assert np.array_equal(_runs_rows(torch, rng_r(t, K, 0, nw), want), want), "full range, runs"
    cuts = [0, nw // 3 + 1, 2 * nw // 3 + 5, nw]
    i_end = want[:, 0].astype(np.int64)
    parts, parts_r = [], []
    for w0, w1 in zip(cuts[:-1], cuts[1:]):
        # the rows of windows [w0, w1): i is the window's 1-based end, w + k
        sub = want[(i_end > w0 + K - 1) & (i_end <= w1 + K - 1)]
        parts.append(_rows(rng_q(t, K, w0, w1)))
        assert np.array_equal(parts[-1], sub), (w0, w1)
        parts_r.append(_runs_rows(torch, rng_r(t, K, w0, w1), sub))
    assert np.array_equal(np.concatenate(parts), want), "three ranges"
    assert np.array_equal(np.concatenate(parts_r), want), "three ranges, runs"


@pytest.mark.parametrize("name", ["self", "unrelated", "copy"])
def test_part_entry_on_a_one_of_one_part(gpu, name):
    torch = gpu
    from kmer_hasher_amd.device import DeviceIndex
    d = _data()
    part = DeviceIndex.build_part(torch.from_numpy(d["s"].copy()).cuda(), K, 0, 1)
    q = d["queries"][name]
    dq = part.query_part(torch.from_numpy(q.copy()).cuda(), K)
    want = d["want"][name][0]
    # the tile offsets only a part query keeps: one tile of 2,048 windows or two, ending at H
    off = dq.tile_offsets().cpu().numpy()
    assert len(off) == (len(q) - K + 1 + 2047) // 2048 + 1 and off[0] == 0 and off[-1] == len(want)
    assert np.array_equal(_rows(dq), want)
    part.free()


def test_table_probe_path(gpu, test_lib, monkeypatch):
    """KMHG_QUERY_DIAG=0 (test build): no diagonal path, every window probes the table."""
    torch = gpu
    from kmer_hasher_amd.device import DeviceIndex
    monkeypatch.setenv("KMHG_QUERY_DIAG", "0")
    d = _data()
    t = torch.from_numpy(d["s"].copy()).cuda()
    idx = DeviceIndex.build(t, K)
    assert np.array_equal(_rows(idx.query(t, K)), d["want"]["self"][0])
    idx.free()
