"""The R glue's kmer_max_occ (kmer.max.occ) over tests/rshim (see tests/test_r_glue.py for the
stand-in R runtime).  Like sequence_kmer_raster it is exported from the glue but not in its
registration table, so it is called by symbol.  error() outside a registered call aborts the
stand-in runtime after printing the message, so each refusal runs in a child process of its own
and is read from there; the argument check comes before the pointer is looked at, so every such
child ends before anything touches the GPU (CPU).  The library's own refusals (a value out of
range, a counts index) are checked in-process through the C ABI and the Python API in
tests/test_gpu_maxocc.py; the glue hands them to error() by the line the pointer refusals here
already take."""
import ctypes as C
import os
import re
import subprocess
import sys

import numpy as np
import pytest

import maxocc_ref
from test_r_glue import INTSXP, ROOT, FakeR

RFILE = os.path.join(ROOT, "kmer_hasher_amd", "R", "kmer_hash_gpu.R")
HERE = os.path.dirname(os.path.abspath(__file__))
M = 2**31 - 1


@pytest.fixture(scope="module")
def R():
    r = FakeR()
    f = r.L.kmer_max_occ
    f.restype, f.argtypes = C.c_void_p, [C.c_void_p] * 2
    yield r
    r.L.fr_reset()


def test_entry_point_exported_wrapped_and_not_registered(R):
    assert R.L.kmer_max_occ
    txt = re.sub(r"\s+", " ", open(RFILE).read())
    assert ('kmer.max.occ <- function(ex.ptr, max.occ=0){ '
            'invisible(.Call("kmer_max_occ", ex.ptr, as.integer(max.occ))) }') in txt
    names = set()
    for j in range(R.n_routines):
        n = C.c_int()
        names.add(R.L.fr_routine(j, C.byref(n)).decode())
    assert "kmer_max_occ" not in names and "kmer_row_order" in names


_CHILD = """
import ctypes as C, sys
sys.path.insert(0, {here!r}); sys.path.insert(0, {root!r})
from test_r_glue import FakeR
R = FakeR()
f = R.L.kmer_max_occ
f.restype, f.argtypes = C.c_void_p, [C.c_void_p] * 2
args = dict(ptr=R.nil(), max_occ=R.i(3))
args.update({name}={value})
f(args["ptr"], args["max_occ"])
print("returned")
"""

ARG = "max.occ should be an integer of length 1"


@pytest.mark.parametrize("name,value,message", [
    ("max_occ", "R.d(3.0)", ARG),                     # the wrapper's as.integer() was skipped
    ("max_occ", 'R.s("3")', ARG),
    ("max_occ", "R.nil()", ARG),
    ("max_occ", "R.i(1, 2)", ARG),
    ("max_occ", "R.i(-2**31)", ARG),                  # NA_integer_: as.integer(2^31), as.integer("x")
    ("ptr", "R.nil()", "ptr_r should be an external pointer"),       # after the argument check
    ("ptr", 'R.L.fr_extptr(None, b"suffix_hash_250930")', "External pointer has incorrect tag"),
    ("ptr", 'R.L.fr_extptr(None, b"kmer_hash_250930")', "external pointer has been finalised"),
])
def test_refusals_carry_their_words(R, name, value, message):
    r = subprocess.run([sys.executable, "-c",
                        _CHILD.format(here=HERE, root=ROOT, name=name, value=value)],
                       capture_output=True, text=True, timeout=120)
    assert r.returncode != 0 and "returned" not in r.stdout, (r.stdout, r.stderr[-2000:])
    assert f"fake_r: error() outside a call: {message}\n" in r.stderr, r.stderr[-2000:]


def _one_int(R, ret):
    assert R.L.fr_type(ret) == INTSXP and R.L.fr_len(ret) == 1
    return int(R.L.fr_ints(ret)[0])


@pytest.mark.gpu
def test_sets_returns_the_previous_value_and_filters_the_query(gpu, R):
    k, units, a, q, ox = maxocc_ref.counted_case()
    rows = ox.query(q, k).reshape(-1, 2)
    ptr = R.call("make_kmer_h_index", R.s(a), R.i(k), R.i(0))
    before = R.int_matrix(R.call("sequence_kmer_positions", ptr, R.s(q), R.i(k)))
    assert np.array_equal(before, rows)
    assert _one_int(R, R.L.kmer_max_occ(ptr, R.i(4))) == 0
    got = R.int_matrix(R.call("sequence_kmer_positions", ptr, R.s(q), R.i(k)))
    want = maxocc_ref.mask_rows(a, k, rows, 4, ox)
    assert 0 < len(want) < len(rows)
    assert np.array_equal(got, want)
    assert _one_int(R, R.L.kmer_max_occ(ptr, R.i(M))) == 4           # the largest legal value
    assert _one_int(R, R.L.kmer_max_occ(ptr, R.i(0))) == M
    got = R.int_matrix(R.call("sequence_kmer_positions", ptr, R.s(q), R.i(k)))
    assert np.array_equal(got, rows)
    assert R.L.fr_finalize(ptr) == 1
