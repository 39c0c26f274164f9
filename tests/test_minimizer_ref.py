"""tests/minimizer_ref.py -- the restatement every GPU test of minimizer sampling checks against --
pinned on the CPU against the library's host mask (kmhg_minimizer_mask: the function of
kmhg_minimizer.h the kernel shares its rule with).  The reference takes valid(s) from the oracle's
index and codes, hashes and scans spans itself; the host function walks neighbours.  Exact.

w is legal up to 256, so w = Nw - 1, Nw and Nw + 1 are tried on pieces of each string short
enough for them (Nw <= 255); the whole strings take w = 1, 2, 5, 19, 255 and 256."""
import numpy as np
import pytest

from oracle import oracle as O
import minimizer_ref

MSG = "w must be between 1 and 256"


def _iid(n, seed):
    return "".join(np.random.default_rng(seed).choice(list("ACGT"), n))


def _strings(testfa):
    rng = np.random.default_rng(5)
    with_n = list(_iid(2500, 2))
    for p in (0, 100, 116, 700, len(with_n) - 16, len(with_n) - 1):
        with_n[p] = "N"
    with_n[1200:1240] = "N" * 40
    with_n[1300:1303] = "nnn"
    return {
        "iid": _iid(3000, 1),
        "fa": testfa[:6000],
        "with_n": "".join(with_n),
        "homopolymer": "A" * 300,
        "period3": "ACG" * 400,
        "lower": "".join(c.lower() if rng.random() < 0.2 else c for c in _iid(700, 3)),
    }


def _host(s, k, w, rc=False):
    from kmer_hasher_amd import minimizer_mask
    return minimizer_mask(s, k, w, rc)


@pytest.mark.parametrize("name", ["iid", "fa", "with_n", "homopolymer", "period3", "lower"])
def test_reference_equals_the_host_mask(testfa, name):
    s = _strings(testfa)[name]
    n_checked = 0
    for k in (5, 15, 31):
        for w in (1, 2, 5, 19, 255, 256):
            for rc in (False, True):
                want = minimizer_ref.mask(s, k, w, rc)
                got = _host(s, k, w, rc)
                assert got.dtype == np.uint8 and got.shape == want.shape
                assert np.array_equal(got, want), (name, k, w, rc)
                n_checked += 1
        for nwin in (3, 40, 255):
            t = s[:nwin + k - 1]
            for w in (1, 2, nwin - 1, nwin, nwin + 1):
                if not 1 <= w <= 256:
                    continue
                for rc in (False, True):
                    want = minimizer_ref.mask(t, k, w, rc)
                    assert np.array_equal(_host(t, k, w, rc), want), (name, k, nwin, w, rc)
                    if w == nwin + 1:
                        assert not want.any()
                    n_checked += 1
    assert n_checked >= 100


def test_w1_selects_every_indexed_window(testfa):
    for s in _strings(testfa).values():
        ox = O.OracleIndex(s, 15)
        m = _host(s, 15, 1)
        assert np.array_equal(np.flatnonzero(m) + 1, np.sort(ox.positions))


def test_homopolymer_selects_every_window_with_a_full_span_to_its_right():
    """Equal hashes: the leftmost of every span, so window s iff s + w - 1 <= Nw."""
    k, w = 5, 10
    m = minimizer_ref.mask("A" * 300, k, w)
    nw = 300 - k + 1
    assert np.array_equal(m, (np.arange(nw) + w <= nw).astype(np.uint8))
    assert np.array_equal(_host("A" * 300, k, w), m)


def test_period3_keeps_one_phase():
    """Three distinct hashes in rotation: every span of w >= 3 has its minimum at the phase of the
    smallest one, so exactly that phase is selected, while a span fits."""
    k, w = 5, 7
    s = "ACG" * 400
    m = minimizer_ref.mask(s, k, w)
    h = minimizer_ref.hashes(s, k)
    phase = int(np.argmin(h[:3]))
    on = np.flatnonzero(m)
    assert len(on) and set((on % 3).tolist()) == {phase}
    assert np.array_equal(_host(s, k, w), m)


def test_density_on_iid_input():
    """200,000 i.i.d. chars, k = 15, w = 10: the selected fraction within 10 % of 2 / (w + 1)."""
    s = _iid(200_000, 20261021)
    m = minimizer_ref.mask(s, 15, 10)
    frac = m.mean()
    print("selected fraction", frac, "expected", 2 / 11)
    assert abs(frac - 2 / 11) <= 0.1 * 2 / 11
    assert np.array_equal(_host(s, 15, 10), m)


@pytest.mark.parametrize("w", [0, 257, -1, -(2**31)])
def test_refusals(w):
    from kmer_hasher_amd import KmerHashError, make_kmer_hash, minimizer_mask
    with pytest.raises(KmerHashError, match=MSG):
        minimizer_mask("ACGT" * 20, 5, w)
    # the build entry refuses before it touches the GPU
    with pytest.raises(KmerHashError, match=MSG):
        make_kmer_hash("ACGT" * 20, 5, False, w)


def test_filter_rows_keeps_order_and_both_masks(testfa):
    s = testfa[:3000]
    k = 15
    ox = O.OracleIndex(s, k)
    rows = ox.query(s, k).reshape(-1, 2)
    m = minimizer_ref.mask(s, k, 5)
    got = minimizer_ref.filter_rows(rows, k, m, m)
    assert 0 < len(got) < len(rows)
    assert m[got[:, 0].astype(np.int64) - k].all() and m[got[:, 1].astype(np.int64) - 1].all()
    keep = np.array([m[i - k] and m[j - 1] for i, j in rows.tolist()], bool)
    assert np.array_equal(got, rows[keep])
    ones = np.ones_like(m)
    assert np.array_equal(minimizer_ref.filter_rows(rows, k, ones, ones), rows)
