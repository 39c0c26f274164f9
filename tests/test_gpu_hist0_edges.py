"""Edges of the first pass over the sequence (V_hist0, kmhg_build_v2.hip; Win8, kmhg_device.h).

Each thread takes eight consecutive windows of a 2,048-window tile from 64 staged chars: the
code and N-flag words are aligned to its first window once, a wave in which no lane sees an N
and no lane's last window comes near the sequence's end skips validity altogether, every other
wave takes an 8-bit validity mask per thread with the sequence-end rules (a window must end
inside the sequence; a final N-free run of exactly k chars is dropped) applied once per thread.
The shapes are the smallest that reach each branch: sequences of at most three tiles, lengths
around k and around the tile, every k at which the 2k-bit key changes shape (1, below / at /
above half a word, 31, 32 with the all-G key of the side slot), a single N at the start, around
the first 16-char word, at the end rules' positions, on either side of a tile boundary and at
the end of the staged halo, an N run over a tile boundary, all N, no N, and at k = 1 an N that
exactly one lane of one wave sees.  kmer.pos against the oracle (tests/test_gpu_parity.py's
reference), on bucket-id and on key streams (KMHG_BUILD_BID=1 / 0, test library), and over the
parts of an owner-computes build."""
import numpy as np
import pytest

from kmh_canon import oracle_index

pytestmark = pytest.mark.gpu

TILE = 2048          # windows per tile of the radix passes (kmhg_common.h PTILE)
HALO = 32            # chars staged behind a tile (kmhg_common.h HALO)
KS = [1, 15, 16, 17, 21, 31, 32]


def _rand(rng, n):
    return "".join(rng.choice(list("ACGT"), n)) if n else ""


def _with_n(s, positions):
    b = bytearray(s.encode())
    for p in positions:
        assert 0 <= p < len(b), p
        b[p] = ord("N")
    return b.decode()


def _sequences(k):
    """(name, sequence) for one k, seeded."""
    rng = np.random.default_rng(1000 + k)
    out = []
    for L in (k + 7, 2047, 2048, 2049, 2048 + k - 1, 4096 + k, 4097 + k):
        out.append((f"L{L}", _rand(rng, L)))            # no N at all
    L = 4097 + k
    base = _rand(rng, L)
    singles = [0, 15, 16, 17, L - 1, L - k, L - k - 1, TILE - 1, TILE, TILE + HALO - 1,
               TILE + HALO, 2 * TILE - 1, 2 * TILE]
    for p in sorted(set(singles)):
        out.append((f"N@{p}", _with_n(base, [p])))
    out.append(("Nrun", _with_n(base, range(TILE - 8, TILE + 12))))
    out.append(("Nrun-end", _with_n(base, range(L - k - 3, L - k))))     # a final run of exactly k
    out.append(("allN", "N" * (TILE + 40)))
    out.append(("lower-iupac", base[:3000].lower() + "RYKM" + base[3004:]))
    if k == 1:
        # a lane's eight windows read chars [s0, s0 + 8): one lane of tile 0's second wave
        out.append(("one-lane", _with_n(base, [1000])))
    if k == 32:
        # the all-G key is the empty sentinel: it lives in the side slot
        out.append(("G40", "G" * 40))
        out.append(("G-run", base[:2030] + "G" * 40 + base[2070:]))
        out.append(("G-end", base[:L - 33] + "G" * 33))
    return out


def _check(make, kpos, s, k, tag):
    oi = oracle_index(s, k)
    ptr = make(s, k)
    res = kpos(ptr, 11)
    inf = ptr.info()
    ptr.free()
    assert np.array_equal(res["count"], oi.counts), tag
    assert np.array_equal(res["pos"].reshape(-1), oi.pos_rows()), tag
    assert res["kmer"] == oi.kmer_strings(), tag
    assert (inf.n_kmers, inf.n_positions, inf.max_count) == (oi.U, oi.N, oi.max_n), tag


@pytest.mark.parametrize("k", KS)
def test_first_pass_edges_vs_oracle(gpu, test_lib, monkeypatch, k):
    from kmer_hasher_amd import kmer_pos, make_kmer_hash
    # L = k: one window, which the end rule drops -- refused up front, as the reference refuses it
    with pytest.raises(Exception, match="at least k"):
        make_kmer_hash(_rand(np.random.default_rng(k), k), k)
    for name, s in _sequences(k):
        for bid in ("1", "0"):
            monkeypatch.setenv("KMHG_BUILD_BID", bid)
            _check(make_kmer_hash, kmer_pos, s, k, (k, name, bid))


@pytest.mark.parametrize("n_parts", [2, 4])
def test_first_pass_edges_over_parts(gpu, n_parts):
    """Two parts take the histogram instance, four the compacting one (PARTC)."""
    torch = gpu
    from kmer_hasher_amd.device import DeviceIndex, merge_part_positions
    k = 31
    rng = np.random.default_rng(7)
    L = 4097 + k
    s = _with_n(_rand(rng, L), list(range(TILE - 8, TILE + 12)) + [0, 17, L - k - 1])
    seq = torch.from_numpy(np.frombuffer(s.encode(), np.uint8).copy()).cuda()
    parts = [DeviceIndex.build_part(seq, k, p, n_parts) for p in range(n_parts)]
    gmask = torch.stack([p.first_mask() for p in parts]).sum(0, dtype=torch.int32)
    segs = [p.positions_part(gmask, 15) for p in parts]
    got = {f: v.cpu().numpy() for f, v in merge_part_positions(segs, 15, k).items()}
    for p in parts:
        p.free()
    oi = oracle_index(s, k)
    assert np.array_equal(got["count"], oi.counts)
    assert np.array_equal(got["pos"].reshape(-1), oi.pos_rows())
    assert np.array_equal(got["pair.pos"].reshape(-1), oi.pair_rows())
    assert [bytes(r[:k]).decode() for r in got["kmer"]] == oi.kmer_strings()
