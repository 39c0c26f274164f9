"""seq.kmer.chains -- the blocks of seq.kmer.blocks linked across diagonals (kmhg_blocks_chains /
kmhg_chains_run*, kmhg_chains.hip) -- against tests/chains_ref.py, the O(B^2) numpy restatement of
the definition in include/kmhgpu.h.  Integer work: every comparison is exact, order included.  The
passes run over tiles of 2,048 BLOCKS and the candidate scan reads 64 blocks per step."""
import numpy as np
import pytest

from revcomp_ref import rc_host
import chains_ref

pytestmark = pytest.mark.gpu

M = 2**31 - 1
ANY = 2**40
DEFAULTS = (5000, 500)


def _dev(torch, blocks):
    b = np.ascontiguousarray(np.asarray(blocks, np.int32).reshape(-1, 4))
    return torch.from_numpy(b).cuda()


def _chains(torch, t, max_dist, max_drift, min_hits=1):
    from kmer_hasher_amd import device
    chains, member = device.blocks_chains(t, max_dist, max_drift, min_hits)
    assert chains.dtype == torch.int32 and chains.dim() == 2 and chains.shape[1] == 6
    assert member.dtype == torch.int32 and member.shape == (t.shape[0],)
    assert chains.is_cuda and member.is_cuda
    return chains.cpu().numpy(), member.cpu().numpy()


def _check(torch, blocks, params):
    """The device's chains of `blocks` against chains_ref at every (max_dist, max_drift[,
    min_hits]); returns the references."""
    blocks = np.asarray(blocks, np.int64).reshape(-1, 4)
    t = _dev(torch, blocks)
    out = []
    for p in params:
        want = chains_ref.chains(blocks, *p)
        got = _chains(torch, t, *p)
        assert got[0].shape == want[0].shape and np.array_equal(got[0], want[0]), (len(blocks), p)
        assert np.array_equal(got[1], want[1]), (len(blocks), p)
        out.append(want)
    return out


def _alone(blocks):
    """Every block as its own chain."""
    b = np.asarray(blocks, np.int64).reshape(-1, 4)
    return np.column_stack([b[:, 0], b[:, 1], b[:, 0] + b[:, 2] - 1, b[:, 1] + b[:, 2] - 1, b[:, 3],
                            np.ones(len(b), np.int64)])


# ------------------------------------------------------------------ 1. hand-made blocks
def test_empty_and_one_block(gpu):
    (c, m), = _check(gpu, np.zeros((0, 4)), [DEFAULTS])
    assert c.shape == (0, 6) and m.shape == (0,)
    (c, m), (c0, _), (cn, mn) = _check(gpu, [(5, 9, 4, 3)], [DEFAULTS, (0, 0), (ANY, ANY, 4)])
    assert c.tolist() == c0.tolist() == [[5, 9, 8, 12, 3, 1]] and m.tolist() == [1]
    assert cn.shape == (0, 6) and mn.tolist() == [0]


def test_max_dist_edge(gpu):
    D = 37
    for extra, linked in ((0, True), (1, False)):
        for di, dj in ((extra, extra), (extra, 0), (0, extra)):
            b = [(1, 1, 4, 4), (5 + D + di, 5 + D + dj, 2, 2)]      # gi = D + di, gj = D + dj
            (c, m), = _check(gpu, b, [(D, 1)])
            assert m.tolist() == ([1, 1] if linked or (di, dj) == (0, 0) else [1, 2]), (di, dj)


def test_max_drift_edge(gpu):
    R = 11
    for shift, linked in ((R, True), (R + 1, False)):
        for b in ([(1, 1, 4, 4), (6, 6 + shift, 2, 2)], [(1, 1, 4, 4), (6 + shift, 6, 2, 2)]):
            (c, m), = _check(gpu, b, [(100, R)])
            assert m.tolist() == ([1, 1] if linked else [1, 2]), (shift, b)


def test_overlap_in_one_coordinate_is_not_linked(gpu):
    for b in ([(1, 1, 4, 4), (4, 9, 2, 2)], [(1, 1, 4, 4), (9, 4, 2, 2)]):      # i only, j only
        (c, m), = _check(gpu, b, [(ANY, ANY)])
        assert np.array_equal(c, _alone(b)) and m.tolist() == [1, 2]


def test_contests_and_ties(gpu):
    # two successors choose block 0: the nearer wins, the other starts its own chain
    (c, m), = _check(gpu, [(1, 1, 4, 4), (6, 6, 2, 2), (7, 9, 1, 1)], [(9, 9)])
    assert c.tolist() == [[1, 1, 7, 7, 6, 2], [7, 9, 7, 9, 1, 1]] and m.tolist() == [1, 1, 2]
    # two equal-cost predecessors: the lower index wins
    (c, m), = _check(gpu, [(1, 3, 1, 1), (3, 1, 1, 1), (5, 5, 1, 1)], [(9, 9)])
    assert c.tolist() == [[1, 3, 5, 5, 2, 2], [3, 1, 3, 1, 1, 1]] and m.tolist() == [1, 2, 1]
    # two equal-cost successors: the lower index wins
    (c, m), = _check(gpu, [(1, 1, 2, 2), (4, 6, 1, 1), (6, 4, 1, 1)], [(9, 9)])
    assert c.tolist() == [[1, 1, 4, 6, 3, 2], [6, 4, 6, 4, 1, 1]] and m.tolist() == [1, 1, 2]


def test_staircase_of_5000_blocks_is_one_chain(gpu):
    """One path through every tile and wave boundary: 5,000 blocks need 13 doublings of the
    pointers' reach (chain_rounds: seven launches of four hops)."""
    n = 5000
    t = np.arange(n, dtype=np.int64)
    b = np.stack([1 + 5 * t, 1 + 5 * t + (t & 1), np.full(n, 3), np.full(n, 2)], axis=1)
    (c, m), (c0, m0) = _check(gpu, b, [(3, 1), (2, 1)])
    assert c.tolist() == [[1, 1, 5 * (n - 1) + 3, 5 * (n - 1) + 1 + 3, 2 * n, n]]
    assert (m == 1).all()
    # at max_dist = 2 the gaps (2, 3) break every other link: block 0, 2,499 pairs, block 4,999
    assert len(c0) == n // 2 + 1 and (c0[1:-1, 5] == 2).all() and c0[0, 5] == c0[-1, 5] == 1


def test_fan_of_1000_candidates_the_last_examined_wins(gpu):
    """One block preceded by 1,000 one-window blocks on distinct diagonals, all inside its window
    and all candidates: the scan crosses the 64- and 256-candidate steps, and the nearest is the
    one with the largest ei -- the last of the sorted order."""
    t = np.arange(1000, dtype=np.int64)
    fan = np.stack([1 + t, 1 + 2 * t, np.ones(1000), np.ones(1000)], axis=1).astype(np.int64)
    b = np.vstack([fan, [(1001, 2001, 2, 2)]])
    pred, child = chains_ref.links(b, 5000, 2000)
    assert pred[1000] == 999 and child[999] == 1000
    _check(gpu, b, [(5000, 2000), (5000, 0), (ANY, ANY)])
    # a block on the diagonal of the fan's first block alone: at max_drift = 0 the only candidate
    # is the FIRST of the sorted order
    b = np.vstack([fan, [(1001, 1001, 2, 2)]])
    assert chains_ref.links(b, 5000, 0)[0][1000] == 0
    _check(gpu, b, [(5000, 0)])


def test_min_hits_drops_a_middle_chain_and_renumbers(gpu):
    b = [(1, 1, 4, 4), (2, 50, 1, 1), (6, 6, 2, 2), (90, 90, 3, 3)]
    (c, m), (c1, m1) = _check(gpu, b, [(9, 9, 2), (9, 9, 1)])
    assert c.tolist() == [[1, 1, 7, 7, 6, 2], [90, 90, 92, 92, 3, 1]] and m.tolist() == [1, 0, 1, 2]
    assert m1.tolist() == [1, 2, 1, 3]


def test_extreme_coordinates(gpu):
    b = [(1, 1, 2, 2), (M - 1, M - 1, 2, 1)]
    (c, m), (_, m2) = _check(gpu, b, [(M - 4, 0), (M - 5, 0)])
    assert c.tolist() == [[1, 1, M, M, 3, 2]] and m2.tolist() == [1, 2]
    _check(gpu, [(1, 1, 1, 1), (1, M, 1, 1), (M, 1, 1, 1), (M, M, 1, 1)], [(ANY, ANY), (ANY, 0)])
    _check(gpu, [(1, 1, M, M)], [(ANY, ANY)])


def test_refusals_carry_their_words_and_the_library_goes_on(gpu):
    torch = gpu
    from kmer_hasher_amd import _lib, device
    ok = _dev(torch, [(1, 1, 4, 4), (8, 8, 2, 2)])
    for args, word in (((-1, 0, 1), "max_dist must not be negative"),
                       ((0, -1, 1), "max_drift must not be negative"),
                       ((0, 0, 0), "min_hits must be a positive integer")):
        with pytest.raises(_lib.KmhgError) as e:
            device.blocks_chains(ok, *args)
        assert str(e.value) == word and e.value.code == _lib.KMHG_EINVAL
    for bad, word in (([(1, 2, 1, 1), (1, 2, 1, 1)], "blocks are not in ascending (i, j) order"),
                      ([(1, 1, 2, 3)], "blocks must have i, j >= 1, 1 <= hits <= span and ends "
                                       "within 2^31 - 1")):
        with pytest.raises(_lib.KmhgError) as e:
            device.blocks_chains(_dev(torch, bad), 5, 5)
        assert str(e.value) == word and e.value.code == _lib.KMHG_EINVAL
    with pytest.raises(TypeError):
        device.blocks_chains(ok[:, :3], 5, 5)
    assert _chains(torch, ok, 3, 0)[1].tolist() == [1, 1]


# ------------------------------------------------------------------ 2. random blocks
def _random_blocks(seed, n=3000, side=20_000, cells=60):
    """n blocks that overlap nowhere: each inside its own cell of a cells x cells grid."""
    rng = np.random.default_rng(seed)
    w = side // cells
    pick = np.sort(rng.choice(cells * cells, n, replace=False))
    ci, cj = pick // cells, pick % cells
    span = rng.integers(1, w // 2, n)
    i = 1 + ci * w + rng.integers(0, w - span + 1)
    j = 1 + cj * w + rng.integers(0, w - span + 1)
    b = np.stack([i, j, span, rng.integers(1, span + 1)], axis=1)
    return b[np.lexsort((b[:, 1], b[:, 0]))]


RANDOM_PARAMS = [(5000, 500, 1), (ANY, 0, 1), (700, ANY, 150)]


@pytest.mark.parametrize("seed", [1, 2, 3])
def test_random_blocks(gpu, seed):
    b = _random_blocks(seed)
    refs = _check(gpu, b, RANDOM_PARAMS)
    assert any((c[:, 5] > 1).any() for c, _ in refs)         # something was linked
    if seed == 1:                                            # determinism: identical bytes
        t = _dev(gpu, b)
        for p in RANDOM_PARAMS:
            one, two = _chains(gpu, t, *p), _chains(gpu, t, *p)
            assert one[0].tobytes() == two[0].tobytes() and one[1].tobytes() == two[1].tobytes()


# ------------------------------------------------------------------ 3. identities on a real query
@pytest.fixture(scope="module")
def fa(gpu, testfa):
    """test.fa[:6000], k = 15, self (53,933 segments): the index, the query and its segments as
    blocks (max_gap = 0), once."""
    torch = gpu
    from kmer_hasher_amd.device import DeviceIndex
    s = np.frombuffer(testfa[:6000].encode(), np.uint8).copy()
    t = torch.from_numpy(s).cuda()
    idx = DeviceIndex.build(t, 15)
    q = idx.query(t, 15)
    yield dict(idx=idx, q=q, t=t, segs=q.blocks(0))
    q.free()
    idx.free()


def test_testfa_max_dist_zero_gives_the_blocks(gpu, fa):
    for max_gap in (0, 15):
        blocks = fa["q"].blocks(max_gap)
        c, m = _chains(gpu, blocks, 0, ANY)
        assert np.array_equal(c, _alone(blocks.cpu().numpy()))
        assert np.array_equal(m, np.arange(1, len(blocks) + 1))
    assert len(fa["segs"]) == 53_933


@pytest.mark.parametrize("D", [15, 200])
def test_testfa_max_drift_zero_reproduces_the_blocks(gpu, fa, D):
    """max_drift = 0 links only along a diagonal, and the nearest block before b on its diagonal is
    within D windows iff seq.kmer.blocks(max_gap = D) merges them: from the segments (max_gap = 0)
    and from the blocks of a smaller max_gap alike."""
    want = fa["q"].blocks(D).cpu().numpy()
    for blocks in (fa["segs"], fa["q"].blocks(7)):
        c, m = _chains(gpu, blocks, D, 0)
        got = np.column_stack([c[:, 0], c[:, 1], c[:, 2] - c[:, 0] + 1, c[:, 4]])
        assert np.array_equal(got, want)
        assert np.array_equal(c[:, 3] - c[:, 1], c[:, 2] - c[:, 0])        # one diagonal each
        assert c[:, 5].sum() == len(blocks) and m.min() == 1 and m.max() == len(c)


def test_testfa_sums_hold_at_the_defaults(gpu, fa):
    blocks = fa["q"].blocks(15)
    b = blocks.cpu().numpy().astype(np.int64)
    c, m = _chains(gpu, blocks, *DEFAULTS)
    assert c[:, 4].astype(np.int64).sum() == b[:, 3].sum() == 5_275_316
    assert c[:, 5].astype(np.int64).sum() == len(b) and len(c) < len(b)
    assert np.array_equal(np.bincount(m, minlength=len(c) + 1)[1:], c[:, 5])
    assert np.array_equal(np.bincount(m, weights=b[:, 3], minlength=len(c) + 1)[1:], c[:, 4])
    first = np.unique(m, return_index=True)[1]               # a chain starts at its first block
    assert np.array_equal(b[first, :2], c[:, :2])
    ck, mk = _chains(gpu, blocks, *DEFAULTS, 1000)
    keep = c[:, 4] >= 1000
    assert np.array_equal(ck, c[keep])
    assert np.array_equal(mk, np.where(keep, np.cumsum(keep), 0)[m - 1])
    # the first 6,000 blocks against the O(B^2) reference, computed here
    head = b[:6000]
    _check(gpu, head, [DEFAULTS])


def test_testfa_whole_input_against_the_recorded_reference(gpu, fa):
    """All 53,911 blocks (max_gap = 15) at the defaults against chains_ref on the same blocks.  The
    O(B^2) reference takes 20 s at this size, so it was run once, on blocks_ref's blocks of the
    oracle's rows, and its result recorded as digests (tests/golden/chains_testfa.json names the
    calls): the blocks' digest ties the device's input to the reference's."""
    import hashlib
    import json
    import os
    want = json.load(open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden",
                                       "chains_testfa.json")))
    blocks = fa["q"].blocks(15)
    b = np.ascontiguousarray(blocks.cpu().numpy())
    assert len(b) == want["blocks"]
    assert hashlib.sha256(b.tobytes()).hexdigest() == want["blocks_sha256"]
    c, m = _chains(gpu, blocks, *DEFAULTS)
    assert len(c) == want["chains"] and int(c[:, 5].max()) == want["longest_chain_blocks"]
    assert int(c[:, 4].max()) == want["largest_chain_hits"]
    assert hashlib.sha256(np.ascontiguousarray(c).tobytes()).hexdigest() == want["chains_sha256"]
    assert hashlib.sha256(np.ascontiguousarray(m).tobytes()).hexdigest() == want["chain_sha256"]


# ------------------------------------------------------------------ 4. a planted-indel query
def _planted(seed=1, n=20_000):
    """An iid sequence A and B = A with three indels of 1 to 20 bases and 20 substitutions."""
    rng = np.random.default_rng(seed)
    A = rng.integers(0, 4, n)
    B = list(A)
    for p in sorted(rng.choice(np.arange(2000, 18000, 500), 3, replace=False))[::-1]:
        ln = int(rng.integers(1, 21))
        if rng.random() < 0.5:
            del B[p:p + ln]
        else:
            B[p:p] = list(rng.integers(0, 4, ln))
    B = np.array(B)
    sub = rng.choice(len(B), 20, replace=False)
    B[sub] = (B[sub] + rng.integers(1, 4, 20)) % 4
    al = np.frombuffer(b"ACGT", np.uint8)
    return al[A].copy(), al[B].copy()


def test_planted_indels_are_chained(gpu):
    """Seed 1 (two deletions of 5 and 14 bases, an insertion of 3): with max_gap = k the 20
    substitutions are bridged and four blocks remain, one per stretch between indels; checked on
    the CPU with chains_ref before the seed was fixed: the defaults give one chain holding every
    hit, max_dist = 0 four."""
    torch = gpu
    from kmer_hasher_amd.device import DeviceIndex
    k = 21
    A, B = _planted()
    idx = DeviceIndex.build(torch.from_numpy(A).cuda(), k)
    tb = torch.from_numpy(B).cuda()
    chains, blocks, member, n_rows = idx.chains(tb, k)                 # the defaults, max_gap = k
    b = blocks.cpu().numpy()
    want = chains_ref.chains(b, *DEFAULTS)
    assert np.array_equal(chains.cpu().numpy(), want[0])
    assert np.array_equal(member.cpu().numpy(), want[1])
    c = want[0]
    assert n_rows == b[:, 3].sum() and c[:, 4].max() >= 0.9 * b[:, 3].sum()
    apart = idx.chains(tb, k, max_dist=0)
    assert len(apart[0]) > 3 and np.array_equal(apart[0].cpu().numpy(), _alone(b))
    assert torch.equal(apart[1], blocks)
    idx.free()


# ------------------------------------------------------------------ 5. the routes agree
def test_routes_give_the_same_bytes(gpu, testfa):
    torch = gpu
    from kmer_hasher_amd import api, device
    from kmer_hasher_amd.device import DeviceIndex
    k = 15
    s = testfa[:2500]
    a = s[:1200] + rc_host(s[1200:1900]) + s[1900:]          # one inverted stretch
    ta = torch.from_numpy(np.frombuffer(a.encode(), np.uint8).copy()).cuda()
    ts = torch.from_numpy(np.frombuffer(s.encode(), np.uint8).copy()).cuda()
    idx = DeviceIndex.build(ta, k)
    ptr = api.make_kmer_hash(a, k)
    for rc in (False, True):
        q = idx.query_rc(ts, k) if rc else idx.query(ts, k)
        for max_dist, max_drift, max_gap, min_len, min_hits in (
                (5000, 500, k, 1, 1), (300, 30, 0, 2, 40), (ANY, ANY, k, 1, 2**40)):
            blocks = q.blocks(max_gap, min_len)
            chains, member = device.blocks_chains(blocks, max_dist, max_drift, min_hits)
            assert len(blocks) > 100 and (min_hits > M) == (len(chains) == 0)
            what = (rc, max_dist, max_drift, max_gap, min_len, min_hits)
            for got in (q.chains(max_dist, max_drift, max_gap, min_len, min_hits),
                        idx.chains(ts, k, max_dist, max_drift, max_gap, min_len, min_hits, rc)[:3],
                        idx.chains(ts, k, max_dist, max_drift, max_gap, min_len, min_hits, rc,
                                   row_free=True)[:3]):
                assert torch.equal(got[0], chains) and torch.equal(got[1], blocks), what
                assert torch.equal(got[2], member), what
            for row_free in (False, True):
                r = api.seq_kmer_chains(ptr, s, k, max_dist, max_drift, max_gap, min_len, min_hits,
                                        rc=rc, row_free=row_free)
                assert sorted(r) == ["blocks", "chain", "chains"]
                assert r["chains"].dtype == r["blocks"].dtype == r["chain"].dtype == np.int32
                assert np.array_equal(r["chains"], chains.cpu().numpy()), what
                assert np.array_equal(r["blocks"], blocks.cpu().numpy()), what
                assert np.array_equal(r["chain"], member.cpu().numpy()), what
        q.free()
    # the defaults: max_gap = k, minimap2's -g and -r
    r = api.seq_kmer_chains(ptr, s, k)
    chains, blocks, member, _ = idx.chains(ts, k)
    assert np.array_equal(r["chains"], chains.cpu().numpy())
    assert np.array_equal(r["blocks"], api.seq_kmer_blocks(ptr, s, k))
    want = chains_ref.chains(r["blocks"], *DEFAULTS)
    assert np.array_equal(r["chains"], want[0]) and np.array_equal(r["chain"], want[1])
    idx.free()
    ptr.free()


def test_api_refuses_a_counts_index_and_bad_parameters(gpu):
    from kmer_hasher_amd import api
    cp = api.count_kmers("ACGTACGTACGTAAACCC", (4, 0, 1))
    with pytest.raises(api.KmerHashError) as e:
        api.seq_kmer_chains(cp, "ACGTACGT", 4)
    assert str(e.value) == "blocks need a position index"
    ptr = api.make_kmer_hash("ACGTACGTACGTAAACCC", 4)
    for kw, word in ((dict(min_len=0), "min_len must be a positive integer"),
                     (dict(max_gap=-1), "max_gap must not be negative"),
                     (dict(max_dist=-1), "max_dist must not be negative"),
                     (dict(max_drift=-1), "max_drift must not be negative"),
                     (dict(min_hits=0), "min_hits must be a positive integer")):
        for row_free in (False, True):
            with pytest.raises(api.KmerHashError) as e:
                api.seq_kmer_chains(ptr, "ACGTACGT", 4, row_free=row_free, **kw)
            assert str(e.value) == word
    r = api.seq_kmer_chains(ptr, "ACGTACGT", 4)
    assert r["chains"].shape[1] == 6 and r["blocks"].shape[1] == 4
    assert r["chains"][:, 4].sum() == len(api.seq_kmer_pos(ptr, "ACGTACGT", 4))
    assert r["chains"][:, 5].sum() == len(r["blocks"]) == len(r["chain"])
    ptr.free()
    cp.free()


# ------------------------------------------------------------------ 6. one base repeated
def test_homopolymer_blocks_all_overlap_and_nothing_links(gpu):
    """"A" * 3000, k = 15, self: every pair of windows matches, so there is one block per diagonal,
    5,971 of them, each overlapping every other in i or in j: no links, the chains are the
    blocks."""
    torch = gpu
    from kmer_hasher_amd.device import DeviceIndex
    t = torch.from_numpy(np.full(3000, ord("A"), np.uint8)).cuda()
    idx = DeviceIndex.build(t, 15)
    for row_free in (False, True):
        chains, blocks, member, n_rows = idx.chains(t, 15, row_free=row_free)
        b = blocks.cpu().numpy()
        assert len(b) == 5971 and n_rows == 2986 * 2986
        assert np.array_equal(chains.cpu().numpy(), _alone(b))
        assert np.array_equal(member.cpu().numpy(), np.arange(1, 5972))
    idx.free()
