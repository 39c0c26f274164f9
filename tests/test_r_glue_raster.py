"""The R glue's sequence_kmer_raster (seq.kmer.raster) over tests/rshim (see tests/test_r_glue.py
for the stand-in R runtime).  Like sequence_kmer_blocks it is exported from the glue but not in
its registration table, so it is called by symbol.  error() outside a registered call aborts the
stand-in runtime after printing the message, so each refusal runs in a child process of its own
and is read from there; the argument checks come before any device work (CPU)."""
import ctypes as C
import os
import re
import subprocess
import sys

import numpy as np
import pytest

from oracle import oracle as O
from revcomp_ref import rc_host
import raster_ref
from test_r_glue import INTSXP, ROOT, FakeR

REALSXP, VECSXP = 14, 19
RFILE = os.path.join(ROOT, "kmer_hasher_amd", "R", "kmer_hash_gpu.R")
HERE = os.path.dirname(os.path.abspath(__file__))


@pytest.fixture(scope="module")
def R():
    r = FakeR()
    f = r.L.sequence_kmer_raster
    f.restype, f.argtypes = C.c_void_p, [C.c_void_p] * 7
    yield r
    r.L.fr_reset()


def test_entry_point_exported_wrapped_and_not_registered(R):
    assert R.L.sequence_kmer_raster
    txt = re.sub(r"\s+", " ", open(RFILE).read())
    assert ('seq.kmer.raster <- function(ex.ptr, seq, k, bins=1024, rc=FALSE, i.range=NULL, '
            'j.range=NULL){ .Call("sequence_kmer_raster", ex.ptr, as.character(seq), '
            'as.integer(k), as.integer(bins), as.integer(rc), '
            'if(is.null(i.range)) NULL else as.integer(i.range), '
            'if(is.null(j.range)) NULL else as.integer(j.range)) }') in txt
    assert "image(" in txt and "log1p(r$counts)" in txt       # how to draw it
    names = set()
    for j in range(R.n_routines):
        n = C.c_int()
        names.add(R.L.fr_routine(j, C.byref(n)).decode())
    assert "sequence_kmer_raster" not in names and "sequence_kmer_positions" in names


_CHILD = """
import ctypes as C, sys
sys.path.insert(0, {here!r}); sys.path.insert(0, {root!r})
from test_r_glue import FakeR
R = FakeR()
f = R.L.sequence_kmer_raster
f.restype, f.argtypes = C.c_void_p, [C.c_void_p] * 7
args = dict(ptr=R.nil(), seq=R.s("ACGTACGT"), k=R.i(3), bins=R.i(4), rc=R.i(0), i_range=R.nil(),
            j_range=R.nil())
args.update({name}={value})
f(args["ptr"], args["seq"], args["k"], args["bins"], args["rc"], args["i_range"], args["j_range"])
print("returned")
"""

BINS = "bins should be one or two positive integers"
IR = "i.range should be c(lo, hi) with 1 <= lo <= hi"
JR = "j.range should be c(lo, hi) with 1 <= lo <= hi"


@pytest.mark.parametrize("name,value,message", [
    ("seq", 'R.s("ACGT", "ACGT")', "seq_r should be a single sequence"),
    ("seq", "R.i(1)", "seq_r should be a single sequence"),
    ("k", "R.d(3.0)", "k should be an integer of length 1"),
    ("bins", "R.i(0)", BINS),
    ("bins", "R.i(4, -1)", BINS),
    ("bins", "R.i(1, 2, 3)", BINS),
    ("bins", "R.d(4.0)", BINS),
    ("rc", "R.nil()", "rc should be an integer of length 1"),
    ("rc", "R.i(-2**31)", "rc should be an integer of length 1"),   # NA_integer_
    ("i_range", "R.i(0, 5)", IR),
    ("i_range", "R.i(5)", IR),
    ("i_range", "R.d(1.0, 5.0)", IR),
    ("j_range", "R.i(7, 6)", JR),
    ("ptr", "R.nil()", "ptr_r should be an external pointer"),      # after the argument checks
    ("ptr", 'R.L.fr_extptr(None, b"other_tag")', "External pointer has incorrect tag"),
])
def test_refusals_carry_their_words(R, name, value, message):
    r = subprocess.run([sys.executable, "-c",
                        _CHILD.format(here=HERE, root=ROOT, name=name, value=value)],
                       capture_output=True, text=True, timeout=120)
    assert r.returncode != 0 and "returned" not in r.stdout, (r.stdout, r.stderr[-2000:])
    assert f"fake_r: error() outside a call: {message}\n" in r.stderr, r.stderr[-2000:]


def _fields(R, ret):
    assert R.L.fr_type(ret) == VECSXP and R.L.fr_len(ret) == 6
    assert R.strings(R.L.fr_names(ret)) == ["counts", "i0", "j0", "bin_i", "bin_j", "n_rows"]
    c = R.L.fr_elt(ret, 0)
    assert R.L.fr_type(c) == REALSXP                 # numeric: a cell may exceed integer.max
    n_i, n_j = R.L.fr_nrow(c), R.L.fr_ncol(c)
    counts = np.ctypeslib.as_array(R.L.fr_reals(c), shape=(n_i * n_j,)).copy()
    ints = []
    for j in range(1, 5):
        e = R.L.fr_elt(ret, j)
        assert R.L.fr_type(e) == INTSXP and R.L.fr_len(e) == 1
        ints.append(int(R.L.fr_ints(e)[0]))
    h = R.L.fr_elt(ret, 5)
    assert R.L.fr_type(h) == REALSXP and R.L.fr_len(h) == 1
    return counts.reshape(n_j, n_i).T, ints, float(R.L.fr_reals(h)[0])


@pytest.mark.gpu
def test_shape_values_strands_and_frames(gpu, R, testfa):
    k = 15
    s = testfa[:3000]
    a = s[:1500] + rc_host(s[1500:2200]) + s[2200:2900]      # one inverted stretch, a shorter index
    ptr = R.call("make_kmer_h_index", R.s(a), R.i(k), R.i(0))
    oi = O.OracleIndex(a, k)
    for rc in (0, 1):
        rows = oi.query(rc_host(s) if rc else s, k).reshape(-1, 2)
        for bins, ir, jr, frame in (
                (R.i(1024), R.nil(), R.nil(), (1, 1, 3, 3, 1000, 967)),
                (R.i(7, 300), R.i(100, 2000), R.i(5, 2899), (100, 5, 272, 10, 7, 290)),
                (R.i(1), R.nil(), R.i(2000, 2000), (1, 2000, 3000, 1, 1, 1))):
            ret = R.L.sequence_kmer_raster(ptr, R.s(s), R.i(k), bins, R.i(rc), ir, jr)
            counts, ints, h = _fields(R, ret)
            assert ints == list(frame[:4]) and h == len(rows) > 0
            want = raster_ref.raster(rows, frame)
            assert counts.shape == want.shape and np.array_equal(counts, want.astype(np.float64))
    assert R.L.fr_finalize(ptr) == 1
