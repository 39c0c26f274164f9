"""count.kmers.fq.sh / kmer.spec.sh on the CPU: the compiled reference reproduces
tests/golden/fq_sh_golden.json, the clean-room automaton (tests/fq_walk.py) equals it on every
golden case, and the C-ABI / Python front end refuse bad arguments with the reference's words
before any device work."""
import ctypes as C
import os

import numpy as np
import pytest

import fq_sh_inputs as I
import fq_walk as W
import ref_fq_sh as R
from kmh_canon import sha
from oracle import oracle as O

GOLD = {c["name"]: c for c in I.load_golden()["cases"]}
needs_ref = pytest.mark.skipif(not R.available(), reason="oracle/_ref/libkmh_ref_sh.so not built")


def _seeded():
    for k in I.LANE_KS:
        for n, (recs, mq) in I.lane_cases(k).items():
            yield f"lane_k{k}_{n}", k, recs, mq
    for k in I.FA_KS:
        for n, recs in I.fa_cases(k).items():
            yield f"fa_k{k}_{n}", k, recs, I.MQ


def _check(name, keys, cnt, spectrum_of):
    g = GOLD[name]
    assert len(keys) == g["U"], name
    assert sha(keys) == g["keys_sha"] and sha(cnt) == g["counts_sha"], name
    if "keys" in g:
        assert [int(x) for x in keys] == g["keys"] and [int(x) for x in cnt] == g["counts"], name
    for mc, sp in g["spectra"].items() if spectrum_of else ():
        got = np.asarray(spectrum_of(int(mc)), np.float64)
        assert sha(got) == sp["sha"], (name, mc)
        if "counts" in sp:
            assert got.tolist() == sp["counts"], (name, mc)
        assert got[0] == 0 and got.sum() == g["U"]


def test_golden_covers_every_case():
    assert set(GOLD) == set(I.FILE_CASES) | {n for n, *_ in _seeded()}
    assert any(c["U"] == 0 for c in GOLD.values()) and any("keys" in c for c in GOLD.values())


@needs_ref
@pytest.mark.parametrize("name", list(I.FILE_CASES))
def test_reference_reproduces_golden_files(name):
    calls = I.FILE_CASES[name]
    ref = R.RefSH1(calls[0][1][0], calls[0][1][2], calls[0][1][3])
    for f, prm in calls:
        ref.add_fastx(os.path.join(I.GOLDEN, f), prm)
    keys, cnt = ref.arrays()
    _check(name, keys, cnt, ref.spectrum)


@needs_ref
def test_reference_reproduces_golden_seeded():
    for name, k, recs, mq in _seeded():
        ref = R.RefSH1(k, I.prefix_bits_for(k)).add_records(recs, mq)
        keys, cnt = ref.arrays()
        # k = 31 needs a 30-bit prefix array, which sh_count_spectrum walks in full (seconds per
        # call): its spectra are reproduced for one case, keys and counts for all
        slow = k == 31 and name != "lane_k31_reads_65"
        _check(name, keys, cnt, None if slow else ref.spectrum)
        ref.close()


def _walk_arrays(counter):
    keys = np.array(sorted(counter), np.uint64)
    return keys, np.array([counter[int(x)] for x in keys], np.int32)


@pytest.mark.parametrize("name", list(I.FILE_CASES))
def test_clean_room_equals_golden_files(name):
    total = W.Counter()
    for f, prm in I.FILE_CASES[name]:
        recs = O.fastx_records(O.read_fastx(os.path.join(I.GOLDEN, f)))
        total.update(W.count_records(recs, prm[0], prm[4], prm[5]))
    keys, cnt = _walk_arrays(total)
    _check(name, keys, cnt, lambda mc: W.spectrum(total, mc))


def test_clean_room_equals_golden_seeded():
    for name, k, recs, mq in _seeded():
        c = W.count_records(recs, k, mq)
        keys, cnt = _walk_arrays(c)
        _check(name, keys, cnt, lambda mc: W.spectrum(c, mc))


def test_walk_rules_by_hand():
    """The end rule and the weak-base rule on strings small enough to check by eye (k = 3)."""
    assert W.window_starts("ggg", 3) == []                    # the init window ends the record
    assert W.window_starts("gggb", 3) == [0]                  # ... followed by a bad base: counted
    assert W.window_starts("gggg", 3) == [0, 1]               # a rolled window may end the record
    assert W.window_starts("wgww", 3) == [0]                  # weak accepted inside the init
    assert W.window_starts("wgwg", 3) == [0, 1]               # the roll tests only the new base
    # a weak base stops the roll and starts the next init: windows 2 and 3 (holding it later) lost
    assert W.window_starts("ggggwggg", 3) == [0, 1, 4, 5]
    assert W.window_starts("gbwggg", 3) == [2, 3]
    assert W.threshold_char(30) == ord("?") and W.threshold_char(0) == ord("!")
    assert W.threshold_char(100) == 133 - 256                 # (char) wraps: every quality is good


# ---------------------------------------------------------------- refusals without a device
def _lib():
    from kmer_hasher_amd import _lib
    return _lib, _lib.lib()


@pytest.mark.parametrize("prm,msg", [
    ([0, 1, 0, 100, 30, -1], "k must be a positive integer less than 1+MAX_K"),
    ([33, 1, 20, 100, 30, -1], "k must be a positive integer less than 1+MAX_K"),
    ([32, 1, 32, 100, 30, -1], "k must be at most 31 for the suffix hash"),
    ([20, 1, 4, 100, 30, -1], "suffix bits (2k - prefix_bits) must be in 0 .. 32"),
    ([10, 1, 24, 100, 30, -1], "suffix bits (2k - prefix_bits) must be in 0 .. 32"),
    ([20, 1, 30, 1, 30, -1], "max_memory is too small for the prefix array of the suffix hash"),
    ([20, 1, 20, 0, 30, -1], "max_memory is too small for the prefix array of the suffix hash"),
])
def test_capi_param_refusals(prm, msg, tmp_path):
    lib_mod, L = _lib()
    h = C.c_void_p()
    arr = (C.c_int32 * 6)(*prm)
    p = str(tmp_path / "x.fq").encode()
    for rc in (L.kmhg_sh1_count_fastq(C.byref(h), p, arr),
               L.kmhg_sh1_count_reads_device(C.byref(h), None, None, None, None, 0, arr, None)):
        assert rc == lib_mod.KMHG_EINVAL and L.kmhg_last_error().decode() == msg
        assert not h.value


def test_capi_null_and_kind_refusals():
    lib_mod, L = _lib()
    out = (C.c_double * 4)()
    assert L.kmhg_sh1_spectrum(None, 3, out) == lib_mod.KMHG_EINVAL
    assert L.kmhg_last_error().decode() == "unable to obtain a suffix_hash from external pointer"
    assert L.kmhg_sh1_count_fastq(None, b"x", None) == lib_mod.KMHG_EINVAL
    assert L.kmhg_sh1_count_reads(None, None, None) == lib_mod.KMHG_EINVAL


def test_python_front_end_refusals(tmp_path):
    from kmer_hasher_amd import api
    E = api.KmerHashError
    with pytest.raises(E, match="^fq_file should be a character vector of length at least one$"):
        api.count_kmers_fq_sh(["a.fq", "b.fq"], [20, 1, 20, 100, 30, -1])
    with pytest.raises(E, match="^k_r must be an integer vector of length 3$"):
        api.count_kmers_fq_sh("a.fq", [20, 1, 20])
    with pytest.warns(UserWarning, match="negative or 0 report n value specified: set to 1e6"):
        with pytest.raises(E, match="^k must be a positive integer less than 1\\+MAX_K$"):
            api.count_kmers_fq_sh("a.fq", [0, 0, 20, 100, 30, -1])    # the warning comes first
    with pytest.raises(E, match="^Unable to extract suffix_hash from external pointer$"):
        api.count_kmers_fq_sh("a.fq", [20, 1, 20, 100, 30, -1], "not a pointer")
    for bad in (None, 3, api.ExtPtr(0, tag=api.SUFFIX_HASH_N_TAG), api.ExtPtr(0)):
        with pytest.raises(E, match="^unable to obtain a suffix_hash from external pointer$"):
            api.kmer_spec_sh(bad, 10)
