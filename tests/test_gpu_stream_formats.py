"""Key-stream radix passes with digit streams on, under every digit width and middle-stream
layout (kmhg_kernels.h StreamFmt): KMHG_BUILD_BID=0 and KMHG_DIGIT_STREAM=1, then

  KMHG_DS_U8=1 / 0     the digit stream the next pass's histogram reads is Digits8 / Digits16;
  KMHG_DS_PACK=1 / 0   the streams before the last are Packed12 / stay KeyPos (KeyPos -> KeyPos
                       with digits out, then KeyPos -> Packed12 into the bucket kernel).

Every setting is built with lane ranks and with ballot ranks and must equal the oracle on the
build totals, the kmer.pos readout with pair rows and the seq.kmer.pos self-query; per input the
four settings' kmer.pos readouts must agree byte for byte.  The knobs select the path
deterministically; no counter reports which digit width or layout ran, so the path is selected
here, not observed."""
import pytest

from test_gpu_parity import _api, _check_against_oracle

pytestmark = pytest.mark.gpu

SETTINGS = [("1", "1"), ("0", "1"), ("1", "0"), ("0", "0")]      # (KMHG_DS_U8, KMHG_DS_PACK)


def _iid(L, seed):
    from kmer_hasher_amd import synth
    return synth.iid(L, seed).tobytes().decode()


def _tandem():
    """test_gpu_bid_pack.test_repeats_tandem's string: invalid windows, multi-batch buckets."""
    return "A" * 20000 + "ACGT" * 100 + "AC" * 9000 + "N" * 7 + "ACG" * 7000 + "T"


# name -> (sequence, k, KMHG_MAXR)
INPUTS = {
    # 59 buckets, radix 4, three passes, 30 tiles: a true middle stream and a last pass
    "iid60k_maxr4": (lambda: _iid(60_000, 3), 31, 4),
    # the same input in two passes (radix 8)
    "iid60k_maxr8": (lambda: _iid(60_000, 3), 31, 8),
    # the minimum two-pass plans: the second tile part-filled, and exactly full
    "two_tiles_part": (lambda: _iid(2048 + 31, 200 + 2048 + 31), 31, 2),
    "two_tiles_full": (lambda: _iid(4096 + 30, 200 + 4096 + 30), 31, 2),
    "tandem_k5": (_tandem, 5, 8),
}


def _setenv(monkeypatch, maxr, u8, pack, ballot="0"):
    monkeypatch.setenv("KMHG_BUILD_BID", "0")
    monkeypatch.setenv("KMHG_DIGIT_STREAM", "1")
    monkeypatch.setenv("KMHG_MAXR", str(maxr))
    monkeypatch.setenv("KMHG_DS_U8", u8)
    monkeypatch.setenv("KMHG_DS_PACK", pack)
    if ballot == "1":
        monkeypatch.setenv("KMHG_TEST_BALLOT", "1")


@pytest.mark.parametrize("ballot", ["0", "1"])
@pytest.mark.parametrize("u8,pack", SETTINGS)
@pytest.mark.parametrize("name", list(INPUTS))
def test_against_oracle(gpu, test_lib, monkeypatch, name, u8, pack, ballot):
    make_s, k, maxr = INPUTS[name]
    _setenv(monkeypatch, maxr, u8, pack, ballot)
    _check_against_oracle(make_s(), k, qks=[k])


@pytest.mark.parametrize("name", list(INPUTS))
def test_settings_agree(gpu, test_lib, monkeypatch, name):
    """The four settings' kmer.pos readouts of one input, byte for byte."""
    make_s, k, maxr = INPUTS[name]
    s = make_s()
    make, kpos, _ = _api()
    got = {}
    for u8, pack in SETTINGS:
        _setenv(monkeypatch, maxr, u8, pack)
        ptr = make(s, k)
        inf = ptr.info()
        assert int(inf.fallback) == 0
        res = kpos(ptr, 11)
        got[u8, pack] = ((inf.n_kmers, inf.n_positions, inf.n_pairs, inf.max_count),
                         res["count"].tobytes(), res["pos"].tobytes(), res["kmer"])
        ptr.free()
    for st in SETTINGS[1:]:
        assert got[st] == got[SETTINGS[0]], st
