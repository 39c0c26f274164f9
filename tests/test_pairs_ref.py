"""kmer.pairs on the CPU: the two restatements against each other, the facts every named input
(pairs_inputs.py) is built to have, and proof that the inputs can tell a wrong kernel from a right
one.

The reference crashes at kmer.pairs (test.R:330), so nothing of its own pins this product: the GPU
rows are compared with pairs_ref (plain dicts and loops over the strings) and OracleIndex.pairs_with
(numpy over the compiled oracle's CSR).  Here the two must agree exactly on every input.  Then a
model of the kernels' dealing (tiles of TILE keys, row t of a key -> (t / count_b, t mod count_b),
inline or listed positions) is run with one defect at a time; each defect must change the rows of
the case built for it, so no such kernel could pass test_gpu_pairs.py."""
import numpy as np
import pytest

import pairs_inputs as I
import pairs_ref as R
from oracle import oracle as O

TILE = I.TILE


def _oracle(seq, k):
    return O.OracleIndex(seq, k)


@pytest.mark.parametrize("name,d", I.RUNS)
def test_two_restatements_agree(name, d):
    x, y = I.sides(name, d)
    k = I.case(name).k
    assert np.array_equal(I.want(name, d), _oracle(x, k).pairs_with(_oracle(y, k)))


def test_khash_order_agrees():
    c = I.case("khash")
    oa, ob = _oracle(c.a, c.k), _oracle(c.b, c.k)
    order = oa.khash_order()
    got = R.pairs_ref(c.a, c.b, c.k, order)
    assert np.array_equal(got, oa.pairs_with(ob, order))
    assert oa.U > 2 * TILE and len(got) == len(I.want("khash", "ab"))
    assert not np.array_equal(got, I.want("khash", "ab"))       # the order shows in the rows


def _oracle_table(name):
    k, S, x = I.count_specs()[name]
    if S == 0:
        return _oracle(x, k)
    oc = O.OracleCounts(k, S)
    for source, seqs in x:
        oc.add(seqs, source)
    return oc.index()


@pytest.mark.parametrize("na,nb", I.COUNT_RUNS)
def test_counts_restatements_agree(na, nb):
    oa, ob = _oracle_table(na), _oracle_table(nb)
    want = I.count_want(na, nb)
    assert len(want) > 2 * TILE and oa.U > 2 * TILE               # several tiles of keys and rows
    assert np.array_equal(want, oa.pairs_with(ob))


def test_counts_inputs_have_their_shapes():
    sp = I.count_specs()
    assert {sp[n][1] for n in sp} == {0, 1, 3}
    m = np.array(list(I.count_table("c1_multi").values()))
    s = np.array(list(I.count_table("c1_single").values()))
    assert m.shape[1] == 1 and m.max() >= 3 and len(m) > len(s)  # re-counted and new keys
    m3 = np.array(list(I.count_table("c3_multi").values()))
    assert m3.shape[1] == 3 and (m3 == 0).any() and (m3 > 0).all(0).any()   # zeros are "positions" too


# ------------------------------------------------------------------------------- shape facts
def _counts(name, d="ab"):
    x, y = I.sides(name, d)
    return R.key_counts(x, y, I.case(name).k)


def _tile_totals(kc):
    rows = np.array([na * nb for _, na, nb in kc], np.int64)
    return [int(rows[t:t + TILE].sum()) for t in range(0, len(rows), TILE)]


@pytest.mark.parametrize("U", I.UA_EDGES)
def test_ua_edges_distinct_kmers(U):
    kc = _counts(f"ua_{U}")
    assert len(kc) == U and all(na == 1 and nb == 1 for _, na, nb in kc)
    assert len(I.want(f"ua_{U}", "ab")) == 2 * U


def test_empty_middle_tile_totals():
    kc = _counts("empty_middle_tile")
    assert len(kc) == 3 * TILE and all(na == 1 for _, na, _ in kc)
    assert _tile_totals(kc) == [TILE, 0, TILE]
    back = _tile_totals(_counts("empty_middle_tile", "ba"))      # b's own middle keys: unshared too
    assert len(back) == 3 and back[0] > 0 and back[1] == 0 and back[2] > 0


def _runs(flags):
    """Maximal runs [(value, length)] of a boolean list."""
    out = []
    for f in flags:
        if out and out[-1][0] == f:
            out[-1][1] += 1
        else:
            out.append([f, 1])
    return out


def test_holes_every_tile_has_both_kinds_of_run():
    c = I.case("holes")
    kc = _counts("holes")
    assert len(kc) == c.facts["U"] == 2 * TILE + 500              # a last tile partly filled
    assert all(na == 1 and nb <= 1 for _, na, nb in kc)
    shared = [nb == 1 for _, _, nb in kc]
    for t in range(0, len(kc), TILE):
        inner = _runs(shared[t:t + TILE])[1:-1]                   # runs wholly inside the tile
        assert [False, c.k] in inner and [True, c.k + 3] in inner, t


@pytest.mark.parametrize("rank", I.HEAVY_RANKS)
def test_tile_edge_heavy_rank_and_counts(rank):
    name = f"heavy_rank_{rank}"
    f = I.case(name).facts
    kc = _counts(name)
    heavy = [(r, na, nb) for r, (key, na, nb) in enumerate(kc) if key == f["key"]]
    assert heavy == [(rank, 300, 299)] == [(f["rank"], f["count_a"], f["count_b"])]
    assert all(na == 1 and nb <= 1 for key, na, nb in kc if key != f["key"])
    assert all(nb == 1 for key, _, nb in _counts(name, "ba") if key != f["key"])
    assert len(kc) > rank + 300                                    # keys after it, in its tile
    assert len(I.want(name, "ab")) == 2 * (300 * 299 + sum(nb for k_, _, nb in kc if k_ != f["key"]))


def test_inline_list_mix_adjacent_in_one_tile():
    c = I.case("inline_list_mix")
    kc = _counts("inline_list_mix")
    assert [(na, nb) for _, na, nb in kc] == c.facts["counts"] and len(kc) < TILE
    combos = {(min(na, 2), min(nb, 2)) for _, na, nb in kc}
    assert combos == {(x, y) for x in (1, 2) for y in (0, 1, 2)}


def test_geometry_sizes():
    c = I.case("geometry")
    assert (len(c.a), len(c.b)) == (200, 400_000) and c.a in c.b
    assert len(I.want("geometry", "ab")) == len(I.want("geometry", "ba")) == 2 * (200 - c.k + 1)


@pytest.mark.parametrize("which", ["both", "a_only", "b_only"])
def test_side_slot_key_counts(which):
    c = I.case(f"side_{which}")
    da, db = R.kmer_starts(c.a, c.k), R.kmer_starts(c.b, c.k)
    assert c.k == 32
    assert len(da.get(I.SIDE_KEY, ())) == c.facts["side_a"]
    assert len(db.get(I.SIDE_KEY, ())) == c.facts["side_b"]
    if which != "b_only":
        assert 0 < list(da).index(I.SIDE_KEY) < len(da) - 1        # inside a real sequence
    assert len(I.want(f"side_{which}", "ab")) > 2 * c.facts["side_a"] * c.facts["side_b"]


def test_n_and_case_runs_of_k_and_k_minus_1():
    c = I.case("n_and_case")
    f = c.facts
    for seq, lone, (lo, hi) in ((c.a, f["lone_a"], f["none_a"]), (c.b, f["lone_b"], f["none_b"])):
        starts = O.windows(seq, c.k)[1]
        assert starts[(starts >= lo) & (starts < hi)].tolist() == [lone]
    assert any(ch in c.a for ch in b"acgt") and b"n" in c.a and b"N" in c.a
    kc = _counts("n_and_case")
    assert {(min(na, 2), min(nb, 2)) for _, na, nb in kc} >= {(1, 1), (1, 2), (2, 1), (2, 2), (1, 0)}


def test_empty_cases_are_empty():
    for name in ("empty_all_n", "empty_disjoint"):
        c = I.case(name)
        assert len(c.a) > c.k and len(R.kmer_starts(c.b, c.k)) > TILE
        assert len(I.want(name, "ab")) == len(I.want(name, "ba")) == 0
    assert len(R.kmer_starts(I.case("empty_all_n").a, 31)) == 0
    assert len(R.kmer_starts(I.case("empty_disjoint").a, 31)) == 470
    assert len(I.SHORT_A[0]) == I.SHORT_A[1]


# ------------------------------------------------------------------------------- mutants
def _model(name, defect=None, d="ab"):
    """The rows as k_join_probe / k_join_emit deal them, with one defect (None: none)."""
    x, y = I.sides(name, d)
    k = I.case(name).k
    da, db = R.kmer_starts(x, k), R.kmer_starts(y, k)
    flat_b = [p for lb in db.values() for p in lb]               # b's lists end to end
    keys = list(da.items())
    out, last = [], None
    for t0 in range(0, len(keys), TILE):
        n0 = len(out)
        for c, (key, la) in enumerate(keys[t0:t0 + TILE]):
            lb = db.get(key, [])
            na, nb = len(la), len(lb)
            if defect == "drop_last_of_tile" and c == TILE - 1:
                continue
            if defect == "drop_first_of_later_tiles" and c == 0 and t0:
                continue
            if defect == "skip_side_slot" and key == I.SIDE_KEY:
                continue
            for t in range(na * nb):
                if defect == "swap_inner_outer":
                    j, i = divmod(t, na)
                elif defect == "divide_by_count_a":
                    i, j = divmod(t, na)
                    i, j = i % na, j % nb                        # (what memory holds there: not modelled)
                else:
                    i, j = divmod(t, nb)
                pb = lb[j]
                if defect == "inline_b_as_index" and nb == 1:
                    pb = flat_b[pb % len(flat_b)]
                out += [la[i], pb]
        if defect == "continue_into_empty_tile" and len(out) == n0 and last is not None:
            out += last
        last = out[-2:] if out else None
    return np.array(out, np.int32)


@pytest.mark.parametrize("defect,name", [
    ("swap_inner_outer", "heavy_rank_2047"),
    ("swap_inner_outer", "heavy_rank_2048"),
    ("swap_inner_outer", "heavy_rank_0"),
    ("divide_by_count_a", "heavy_rank_2047"),
    ("divide_by_count_a", "heavy_rank_2048"),
    ("divide_by_count_a", "heavy_rank_0"),
    ("drop_last_of_tile", "heavy_rank_2047"),
    ("drop_first_of_later_tiles", "ua_2049"),
    ("drop_first_of_later_tiles", "heavy_rank_2048"),
    ("inline_b_as_index", "inline_list_mix"),
    ("continue_into_empty_tile", "empty_middle_tile"),
    ("skip_side_slot", "side_both"),
])
def test_inputs_tell_a_defective_kernel(defect, name):
    true = I.want(name, "ab")
    assert np.array_equal(_model(name), true)                      # the model itself is right
    assert not np.array_equal(_model(name, defect), true)
