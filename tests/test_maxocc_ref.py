"""tests/maxocc_ref.py -- the restatement every GPU test of kmer.max.occ checks against -- pinned
on the CPU against a count written from the strings alone: how often a row's k-mer occurs in the
index sequence, by a plain dictionary over its windows."""
from collections import Counter

import numpy as np
import pytest

from oracle import oracle as O
import maxocc_ref

M = 2**31 - 1


def _plain_mask(a, k, rows, max_occ):
    """Rows whose k-mer a[j - 1 : j - 1 + k] is held by at most max_occ windows of `a` (windows of
    A, C, G, T only, either case)."""
    up = a.upper()
    n = Counter(up[p:p + k] for p in range(len(up) - k + 1) if set(up[p:p + k]) <= set("ACGT"))
    js = np.unique(rows[:, 1])                       # (the dictionary once per distinct j)
    cj = np.array([n[up[j - 1:j - 1 + k]] for j in js.tolist()])
    return rows[cj[np.searchsorted(js, rows[:, 1])] <= max_occ]


@pytest.fixture(scope="module")
def fa(testfa):
    s = testfa[:6000]
    ox = O.OracleIndex(s, 15)
    return s, 15, s, ox, ox.query(s, 15).reshape(-1, 2)


@pytest.fixture(scope="module")
def counted():
    k, units, a, q, ox = maxocc_ref.counted_case()
    rows = ox.query(q, k).reshape(-1, 2)
    per_window = np.unique(rows[:, 0], return_counts=True)[1]
    assert set(per_window.tolist()) == set(maxocc_ref.COUNTS)
    assert len(q) - k + 1 > maxocc_ref.TILE and rows[-1, 0] == len(q)
    return a, k, q, ox, rows


@pytest.mark.parametrize("case", ["fa", "counted"])
def test_mask_rows_equals_the_plain_count(request, case):
    a, k, q, ox, rows = request.getfixturevalue(case)
    caps = (1, 2, 8, 100) if case == "fa" else (1, 2, 4, 5, 256, 257, 2099, 2100)
    sizes = []
    for n in caps:
        got = maxocc_ref.mask_rows(a, k, rows, n, ox)
        want = _plain_mask(a, k, rows, n)
        assert got.dtype == rows.dtype and np.array_equal(got, want), n
        assert np.array_equal(got, maxocc_ref.mask_rows(a, k, rows, n)), n     # builds its own oracle
        sizes.append(len(got))
    assert 0 < sizes[0] and sizes == sorted(sizes) and len(set(sizes)) > 2 and sizes[-1] <= len(rows)


def test_the_boundary_is_inclusive(counted):
    """A window of exactly max_occ hits keeps them all; one more and it loses all."""
    a, k, q, ox, rows = counted
    for c in maxocc_ref.COUNTS:
        per = np.unique(maxocc_ref.mask_rows(a, k, rows, c, ox)[:, 0], return_counts=True)[1]
        assert per.max() == c and set(per.tolist()) == {x for x in maxocc_ref.COUNTS if x <= c}
        if c > 1:
            per = np.unique(maxocc_ref.mask_rows(a, k, rows, c - 1, ox)[:, 0], return_counts=True)[1]
            assert per.max() < c


@pytest.mark.parametrize("case", ["fa", "counted"])
def test_off_and_beyond_the_largest_count_change_nothing(request, case):
    a, k, q, ox, rows = request.getfixturevalue(case)
    top = int(ox.counts.max())
    assert top > 1
    for n in (0, top, top + 1, M):
        got = maxocc_ref.mask_rows(a, k, rows, n, ox)
        assert got.shape == rows.shape and np.array_equal(got, rows), n
    assert len(maxocc_ref.mask_rows(a, k, rows, top - 1, ox)) < len(rows)


@pytest.mark.parametrize("case", ["fa", "counted"])
def test_cap_one_leaves_the_windows_with_one_hit(request, case):
    a, k, q, ox, rows = request.getfixturevalue(case)
    got = maxocc_ref.mask_rows(a, k, rows, 1, ox)
    i, n = np.unique(rows[:, 0], return_counts=True)
    assert len(got) and np.array_equal(got[:, 0], i[n == 1])        # one row each, in window order
    assert np.array_equal(got, rows[np.isin(rows[:, 0], i[n == 1])])


def test_occurrences_are_the_oracles_counts(fa):
    s, k, _, ox, _ = fa
    occ = maxocc_ref.occurrences(ox)
    assert occ.sum() == int((ox.counts.astype(np.int64) ** 2).sum())
    assert np.count_nonzero(occ) == ox.N and occ[0] == 0
