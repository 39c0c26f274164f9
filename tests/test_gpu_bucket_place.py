"""Pass A of the group bucket kernel by placement (kmhg_build_v2.hip k_v2_bucket_wg): a one-batch
position bucket of a bucket-id stream counts the keys of every home slot, scans the counts into
the linear-probing layout and stores each key at its place; a bucket with a repeated key (or a
second wrap) clears the table and takes the CAS pass.  Every input is built with
KMHG_BUCKET_PLACE=1 and =0 over bucket-id (KMHG_BUILD_BID=1) and key streams (=0; the key-stream
kernels are compiled without the placement and always take the CAS pass) and must equal the
oracle on the build totals, the kmer.pos readout and the seq.kmer.pos self-query.  The test
build's counters (kmhg_bucket_place_counters: placed, fallen back for a repeat, fallen back for a
second wrap) show which path ran."""
import ctypes as C

import numpy as np
import pytest

from kmh_canon import oracle_index
from test_gpu_parity import _api, _check_against_oracle

pytestmark = pytest.mark.gpu

CAPW = 1536        # slots per group bucket (kmhg_kernels.h V2_CAPW)
MODES = [(place, bid) for place in ("1", "0") for bid in ("1", "0")]


def _counters(reset=True):
    from kmer_hasher_amd import _lib
    out = (C.c_uint64 * 3)()
    _lib.check(_lib.lib().kmhg_bucket_place_counters(out, 1 if reset else 0))
    return tuple(int(x) for x in out)


def _iid(L, seed):
    from kmer_hasher_amd import synth
    return synth.iid(L, seed).tobytes().decode()


def _rand(L, seed):
    rng = np.random.default_rng(seed)
    return "".join(rng.choice(list("ACGT"), L))


def _all_modes(monkeypatch, s, k, pairs=True, qks=None):
    """The oracle check in all four modes; returns {(place, bid): (placed, repeat, wrap, buckets,
    fallback to the global-atomic build)} of one more build per mode."""
    make = _api()[0]
    seen = {}
    for place, bid in MODES:
        monkeypatch.setenv("KMHG_BUCKET_PLACE", place)
        monkeypatch.setenv("KMHG_BUILD_BID", bid)
        _check_against_oracle(s, k, qks=qks, pairs=pairs)
        _counters()
        ptr = make(s, k)
        inf = ptr.info()
        seen[(place, bid)] = _counters() + (int(inf.table_slots) // CAPW, int(inf.fallback))
        ptr.free()
        if place == "0" or bid == "0":
            assert seen[(place, bid)][:3] == (0, 0, 0), (place, bid, seen)
    return seen


@pytest.mark.parametrize("k", [31, 32])
def test_smallest_buckets(gpu, test_lib, monkeypatch, k):
    """2 windows, a part-filled bucket, and a window count on either side of the bucket size.
    (L = k, one window, is no index: like the reference, the build refuses a sequence that is
    not longer than k, whichever pass A is chosen -- checked as that refusal.)"""
    from kmer_hasher_amd.api import KmerHashError
    for place, bid in MODES:
        monkeypatch.setenv("KMHG_BUCKET_PLACE", place)
        monkeypatch.setenv("KMHG_BUILD_BID", bid)
        with pytest.raises(KmerHashError, match="at least k"):
            _api()[0](_iid(k, 100 + k), k)
    for L in (k + 1, 200, 1054, 1055):
        seen = _all_modes(monkeypatch, _iid(L, 100 + L), k)
        placed, rpt, wrap, nb, fb = seen[("1", "1")]
        assert fb == 0 and placed + rpt + wrap == nb and placed > 0, (L, seen)


@pytest.mark.parametrize("L,seed", [(60_000, 3), (1_200_000, 17)])
def test_many_buckets_iid(gpu, test_lib, monkeypatch, L, seed):
    """Many i.i.d. buckets: runs that reach the table's end wrap into its first slots.  (With
    code-word keys a one-batch bucket holds at most CAPW windows, so the second-wrap fallback
    cannot fire here; its counter is checked to stay 0.)"""
    seen = _all_modes(monkeypatch, _iid(L, seed), 31, pairs=False)
    placed, rpt, wrap, nb, fb = seen[("1", "1")]
    assert fb == 0 and placed > 0 and placed + rpt + wrap == nb, seen
    assert wrap == 0, seen
    assert all(v[4] == 0 for v in seen.values()), seen


def test_repeats_small(gpu, test_lib, monkeypatch):
    """Every bucket repeats (k = 3, 12 on 5,000 bases); a mix of placed and fallen-back buckets in
    one build (k = 12 on 60,000 bases)."""
    s5 = _rand(5000, 21)
    for k in (3, 12):
        seen = _all_modes(monkeypatch, s5, k)
        assert seen[("1", "1")][4] == 0, seen
    seen = _all_modes(monkeypatch, _rand(60_000, 22), 12)
    placed, rpt, wrap, nb, fb = seen[("1", "1")]
    assert fb == 0 and placed > 0 and rpt > 0, seen


@pytest.mark.parametrize("k", [5, 31])
def test_repeats_tandem(gpu, test_lib, monkeypatch, k):
    """Tandem arrays: multi-batch buckets (never placed) beside one-batch ones."""
    s = "A" * 20000 + "ACGT" * 100 + "AC" * 9000 + "N" * 7 + "ACG" * 7000 + "T"
    _all_modes(monkeypatch, s, k, pairs=False, qks=[k])   # (pair rows: test_bucket_kernels_vs_oracle)


def test_repeats_families(gpu, test_lib, monkeypatch):
    """Repeat families with N runs: most buckets count, scan and then fall back."""
    from kmer_hasher_amd import synth
    rr = synth.add_n_runs(synth.repeat_rich(400_000, 13, n_gap_every=100_000), 0.001, 5)
    seen = _all_modes(monkeypatch, rr.tobytes().decode("latin-1"), 21, pairs=True, qks=[21])
    assert seen[("1", "1")][1] > 0 and seen[("1", "1")][4] == 0, seen


def test_sentinel_key(gpu, test_lib, monkeypatch):
    """k = 32: the all-G window is the empty sentinel (the side slot), the all-T window key 0."""
    for s in ("G" * 40, "T" * 40, "ACGT" * 20 + "G" * 32 + "ACGTT" * 9):
        _all_modes(monkeypatch, s, 32, qks=[31])


def test_ballot_variant(gpu, test_lib, monkeypatch):
    """The ballot-rank kernels (KMHG_TEST_BALLOT=1) have the placement in front of them too."""
    from kmer_hasher_amd import synth
    monkeypatch.setenv("KMHG_TEST_BALLOT", "1")
    seen = _all_modes(monkeypatch, _iid(60_000, 3), 31, pairs=False)
    placed, rpt, wrap, nb, fb = seen[("1", "1")]
    assert fb == 0 and placed > 0 and placed + rpt + wrap == nb, seen
    rr = synth.add_n_runs(synth.repeat_rich(400_000, 13, n_gap_every=100_000), 0.001, 5)
    _all_modes(monkeypatch, rr.tobytes().decode("latin-1"), 21, pairs=True, qks=[21])


@pytest.mark.parametrize("ballot", ["0", "1"])
@pytest.mark.parametrize("base,k,n", [("A", 31, n) for n in (1535, 1536, 1537, 3073, 2047, 2048, 2049)]
                         + [("G", 32, 1537), ("G", 32, 2049)])
def test_batch_boundary(gpu, test_lib, monkeypatch, base, k, n, ballot):
    """One bucket of exactly n windows of one key, n on either side of a batch: 1536 windows per
    batch of a bucket-id stream, 2048 of a key stream (one batch against two, two against three).
    All-G at k = 32 is the sentinel key, so the many-batch count lands in the side slot."""
    monkeypatch.setenv("KMHG_TEST_BALLOT", ballot)
    seen = _all_modes(monkeypatch, base * (n + k - 1), k, pairs=False)
    assert all(v[4] == 0 for v in seen.values()), seen


@pytest.mark.parametrize("tags", ["0", "1"])
def test_query_paths_over_placed_layout(gpu, test_lib, monkeypatch, tags):
    """The table probe and the tag probe (diagonal path off) find keys placed in home order,
    wrapped runs included: a self-query and an unrelated query of the iid 60 K index."""
    make, _, sqk = _api()
    monkeypatch.setenv("KMHG_QUERY_DIAG", "0")
    monkeypatch.setenv("KMHG_QUERY_TAGS", tags)
    monkeypatch.setenv("KMHG_BUILD_BID", "1")
    s, u = _iid(60_000, 3), _iid(40_000, 4)
    oi = oracle_index(s, 31)
    for place in ("1", "0"):
        monkeypatch.setenv("KMHG_BUCKET_PLACE", place)
        _counters()
        ptr = make(s, 31)
        for q in (s, u, u[:100] + s[5000:9000] + u[100:300]):
            assert np.array_equal(sqk(ptr, q, 31).reshape(-1), oi.query(q, 31)), (place, tags)
        assert (_counters()[0] > 0) == (place == "1")
        ptr.free()
