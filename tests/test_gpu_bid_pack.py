"""The packed middle stream of two-pass bucket-id builds (kmhg_kernels.h StreamFmt::DigitPos: the
k_v2_scatter passes Bids -> DigitPos and DigitPos -> Pos, k_v2_histp<DigitPos> and the bucket-start
level over a DigitPos input): one u32 per window between the two radix passes, the digit-pos word
(pass-1 digit << 24) | pos, instead of the BidPos pair of arrays (bucket id, pos).  It is taken by
a bucket-id build of two passes at a radix <= 256 and fewer than 2^24 windows without digit
streams; every other bucket-id build keeps the two arrays.

Every case is built with KMHG_BUILD_BID=1 under KMHG_BID_PACK=1 and =0.  Each build must equal the
oracle on the build totals, the kmer.pos readout with pair rows and the seq.kmer.pos self-query,
the two settings must agree byte for byte, and the test build's counters
(kmhg_bid_pack_counters: packed, two arrays) must show the packed stream for =1 exactly where the
plan is eligible and never for =0."""
import ctypes as C

import numpy as np
import pytest

from kmh_canon import oracle_index
from test_gpu_parity import _api, _check_against_oracle

pytestmark = pytest.mark.gpu

CAPW = 1536        # slots per group bucket (kmhg_kernels.h V2_CAPW)
MAXR_IL = 320      # the widest radix of one pass (kmhg_kernels.h V2_MAXR_IL)


def _counters(reset=True):
    from kmer_hasher_amd import _lib
    out = (C.c_uint64 * 2)()
    _lib.check(_lib.lib().kmhg_bid_pack_counters(out, 1 if reset else 0))
    return tuple(int(x) for x in out)


def _plan(nb, maxr=None):
    """(passes, R) of build_device_v2's radix plan for nb buckets."""
    maxr = max(2, min(MAXR_IL, maxr or MAXR_IL))
    for passes in range(1, 5):
        R = 1
        while R ** passes < nb:
            R += 1
        if R <= maxr:
            return passes, R
    raise AssertionError(nb)


def _eligible(nb, nw, maxr=None, ds=False):
    passes, R = _plan(nb, maxr)
    return passes == 2 and R <= 256 and nw < (1 << 24) and not ds


def _iid(L, seed):
    from kmer_hasher_amd import synth
    return synth.iid(L, seed).tobytes().decode()


def _readout(s, k):
    """One more build: (info totals, kmer.pos arrays, self-query rows), buckets, counters.  (The
    pair rows are a function of the position rows; both settings' were compared with the
    oracle's.)"""
    make, kpos, sqk = _api()
    _counters()
    ptr = make(s, k)
    inf = ptr.info()
    assert int(inf.fallback) == 0
    res = kpos(ptr, 11)
    out = {"totals": (inf.n_kmers, inf.n_positions, inf.n_pairs, inf.max_count),
           "count": res["count"].tobytes(), "pos": res["pos"].tobytes(), "kmer": res["kmer"],
           "query": sqk(ptr, s, min(k, 31)).tobytes()}
    nb = int(inf.table_slots) // CAPW
    ptr.free()
    return out, nb, _counters()


def _both(monkeypatch, s, k, maxr=None, pairs=True, ds=False, qks=None):
    """The oracle check and the byte comparison under both knob settings; returns whether the
    plan was eligible for the packed stream."""
    monkeypatch.setenv("KMHG_BUILD_BID", "1")
    if maxr:
        monkeypatch.setenv("KMHG_MAXR", str(maxr))
    got = {}
    for pack in ("1", "0"):
        monkeypatch.setenv("KMHG_BID_PACK", pack)
        _check_against_oracle(s, k, qks=qks, pairs=pairs)
        got[pack], nb, ctr = _readout(s, k)
        want = _eligible(nb, len(s) - k + 1, maxr, ds) and pack == "1"
        assert ctr == ((1, 0) if want else (0, 1)), (pack, nb, ctr)
    assert got["1"] == got["0"]
    return _eligible(nb, len(s) - k + 1, maxr, ds)


@pytest.mark.parametrize("L", [4000, 2048 + 30, 2048 + 31, 4096 + 30])
def test_two_passes_minimum(gpu, test_lib, monkeypatch, L):
    """KMHG_MAXR=2: 4 buckets, radix 2, two tiles (the second part-filled, or exactly full); a
    window count on either side of one tile (2,048 windows are two buckets: one pass, so the two
    arrays; 2,049 are three: two passes)."""
    ok = _both(monkeypatch, _iid(L, 200 + L), 31, maxr=2)
    assert ok == (L != 2048 + 30)


@pytest.mark.parametrize("ballot", ["0", "1"])
def test_many_tiles(gpu, test_lib, monkeypatch, ballot):
    """KMHG_MAXR=8 at 60,000 bases: 59 buckets, radix 8, 30 tiles; once with the ballot ranks."""
    if ballot == "1":
        monkeypatch.setenv("KMHG_TEST_BALLOT", "1")
    assert _both(monkeypatch, _iid(60_000, 3), 31, maxr=8)


def test_default_plan_smallest_two_pass(gpu, test_lib, monkeypatch):
    """More than 320 buckets: the default plan's first two-pass build (332 buckets, radix 19)."""
    assert _both(monkeypatch, _iid(340_000, 7), 31)


@pytest.mark.parametrize("k", [5, 31])
def test_repeats_tandem(gpu, test_lib, monkeypatch, k):
    """Tandem arrays and an N run: invalid windows (ids ~0) and multi-batch buckets."""
    s = "A" * 20000 + "ACGT" * 100 + "AC" * 9000 + "N" * 7 + "ACG" * 7000 + "T"
    assert _both(monkeypatch, s, k, maxr=8, qks=[k])


def test_repeat_families_default_plan(gpu, test_lib, monkeypatch):
    """Repeat families with N runs under the default plan (391 buckets, two passes)."""
    from kmer_hasher_amd import synth
    rr = synth.add_n_runs(synth.repeat_rich(400_000, 13, n_gap_every=100_000), 0.001, 5)
    assert _both(monkeypatch, rr.tobytes().decode("latin-1"), 21, qks=[21])


def test_ineligible_plans_keep_two_arrays(gpu, test_lib, monkeypatch):
    """Three passes (KMHG_MAXR=4 at 60,000 bases) and digit streams (KMHG_DS_BID=1) keep the two
    arrays whatever the knob says, and agree with the oracle."""
    s = _iid(60_000, 3)
    assert _plan(59, 4)[0] == 3
    assert not _both(monkeypatch, s, 31, maxr=4)
    monkeypatch.setenv("KMHG_DS_BID", "1")
    assert not _both(monkeypatch, s, 31, maxr=8, ds=True)


@pytest.mark.parametrize("maxr", [None, 16])
@pytest.mark.parametrize("n_parts", [2, 3])
def test_owner_computes_parts(gpu, test_lib, monkeypatch, n_parts, maxr):
    """The parts of a 340,000-base build with bucket-id streams and KMHG_BID_PACK=1, assembled
    and compared with the single-device index.  Under the default plan the parts' 166 / 111 local
    buckets take one pass (two arrays) beside the whole build's packed two; KMHG_MAXR=16 gives
    every part a two-pass plan over its LOCAL bucket ids (the packed stream) and the whole build
    three passes."""
    torch = gpu
    from kmer_hasher_amd import synth
    from kmer_hasher_amd.device import DeviceIndex
    from test_gpu_parts import _assemble_local, _slot_sets
    monkeypatch.setenv("KMHG_BUILD_BID", "1")
    monkeypatch.setenv("KMHG_BID_PACK", "1")
    if maxr:
        monkeypatch.setenv("KMHG_MAXR", str(maxr))
    k = 31
    seq_np = synth.iid(340_000, 7)
    nw = seq_np.size - k + 1
    seq = torch.from_numpy(seq_np.copy()).cuda()
    _counters()
    whole = DeviceIndex.build(seq, k)
    inf_w = whole.info()
    nb = int(inf_w["table_slots"]) // CAPW
    assert _counters() == ((1, 0) if _eligible(nb, nw, maxr) else (0, 1))
    meta_w, bufs_w = whole.export_image()
    parts = [DeviceIndex.build_part(seq, k, p, n_parts) for p in range(n_parts)]
    n_packed = sum(_eligible(int(p.part_info()["nb"]), nw, maxr) for p in parts)
    assert _counters() == (n_packed, n_parts - n_packed)
    assert n_packed == (n_parts if maxr else 0)
    idx, table, positions, lay = _assemble_local(parts, torch)
    inf_a = idx.info()
    for f in ("n_kmers", "n_positions", "n_pairs", "max_count", "table_slots"):
        assert inf_w[f] == inf_a[f], (n_parts, f)
    assert _slot_sets(table, positions, lay["capb"]) == \
        _slot_sets(bufs_w[0][:table.numel()], bufs_w[1], lay["capb"])
    s = seq_np.tobytes()
    oi = oracle_index(s, k)
    res = idx.positions(14)
    assert np.array_equal(res["count"].cpu().numpy(), oi.counts)
    assert np.array_equal(res["pos"].cpu().numpy().reshape(-1), oi.pos_rows())
    assert np.array_equal(res["pair.pos"].cpu().numpy().reshape(-1), oi.pair_rows())
    q = idx.query(seq, k)
    assert np.array_equal(q.rows().cpu().numpy().reshape(-1), oi.query(s, k))
    q.free()
    for p in parts:
        p.free()
    idx.free()
    whole.free()
