"""The compiled reference as the source of expected values for count.kmers.fq.sh / kmer.spec.sh.

oracle/_ref/libkmh_ref_sh.so (built by oracle/Makefile from the reference's own sources) holds
init_kmer_qual_2, init_suffix_hash_p, sh_add_kmer, sh_kmer_count and sh_count_spectrum.  The
.Call wrapper count_kmers_fastq_sh and its helper seq_to_counts_sh live in src/kmer_hash.c, which
needs R headers; their two short loops (the record loop, src/kmer_hash.c:768-773, and the roll
loop, :306-329) are restated here over those compiled functions, as oracle/ref_sh_harness.c does
for the .rp wrappers.  Records come from the oracle's kseq restatement (oracle.fastx_records).
"""
import ctypes as C
import os

import numpy as np

from oracle import oracle as O

HERE = os.path.dirname(os.path.abspath(__file__))
LIB = os.path.join(os.path.dirname(HERE), "oracle", "_ref", "libkmh_ref_sh.so")
M64 = (1 << 64) - 1


def available() -> bool:
    return os.path.exists(LIB)


_lib = None


def lib():
    global _lib
    if _lib is None:
        L = C.CDLL(LIB)
        u64p = C.POINTER(C.c_uint64)
        L.init_kmer_qual_2.restype = C.c_size_t
        L.init_kmer_qual_2.argtypes = [C.c_char_p, C.c_char_p, C.c_char, C.c_size_t, u64p, u64p,
                                       C.c_int]
        L.init_suffix_hash_p.restype = None
        L.init_suffix_hash_p.argtypes = [C.c_void_p, C.c_uint32, C.c_uint32, C.c_size_t]
        L.free_suffix_hash.restype = None
        L.free_suffix_hash.argtypes = [C.c_void_p]
        L.sh_add_kmer.restype = C.c_int
        L.sh_add_kmer.argtypes = [C.c_void_p, C.c_uint64]
        L.sh_kmer_count.restype = C.c_uint32
        L.sh_kmer_count.argtypes = [C.c_void_p, C.c_uint64]
        L.sh_count_spectrum.restype = C.c_size_t
        L.sh_count_spectrum.argtypes = [C.c_void_p, C.POINTER(C.c_double), C.c_uint32]
        _lib = L
    return _lib


def _schar(b: int) -> int:
    return b - 256 if b >= 128 else b


class RefSH1:
    """One suffix_hash of the compiled reference (struct of 72 bytes, zeroed buffer of 256)."""

    def __init__(self, k: int, prefix_bits: int, max_memory_gib: int = 100):
        self.L = lib()
        self.k = k
        self.buf = C.create_string_buffer(256)
        self.L.init_suffix_hash_p(self.buf, prefix_bits, 2 * k - prefix_bits, max_memory_gib << 30)
        self.keys = set()

    def add_record(self, seq: bytes, qual, min_quality: int) -> None:
        """seq_to_counts_sh (src/kmer_hash.c:296-332) over the compiled init_kmer_qual_2 and
        sh_add_kmer."""
        L, k = self.L, self.k
        mq_byte = (min_quality + 33) & 0xFF            # char min_quality = (char)params[4] + '!'
        mq = _schar(mq_byte)
        s = seq.split(b"\0")[0] + b"\0"
        n = len(s) - 1
        mask = (1 << (2 * k)) - 1 if k < 32 else M64
        shift = 64 - 2 * k
        off, rc = C.c_uint64(0), C.c_uint64(0)
        i = 0
        while s[i]:
            i = L.init_kmer_qual_2(s, qual, C.c_char(bytes([mq_byte])), i, C.byref(off),
                                   C.byref(rc), k)
            if not s[i]:
                break
            f, r = off.value, rc.value
            key = min(f & mask, (r >> shift) & mask)
            L.sh_add_kmer(self.buf, key)
            self.keys.add(key)
            while i < n and (s[i] | 0x20) != 0x6E and (qual is None or _schar(qual[i]) > mq):
                c = (s[i] >> 1) & 3
                f = ((f << 2) | c) & M64
                r = (r >> 2) | (((c + 2) % 4) << 62)
                i += 1
                key = min(f & mask, (r >> shift) & mask)
                L.sh_add_kmer(self.buf, key)
                self.keys.add(key)
            off.value, rc.value = f, r

    def add_records(self, records, min_quality: int, max_read_n: int = -1) -> "RefSH1":
        """The record loop of count_kmers_fastq_sh (src/kmer_hash.c:768-773)."""
        limit = max_read_n if max_read_n >= 0 else 1 << 62      # (size_t) of the int
        n_reads = 0
        for s, q in records:
            if n_reads >= limit:
                break
            n_reads += 1
            if len(s) <= self.k:
                continue
            self.add_record(s, q, min_quality)
        return self

    def add_fastx(self, path: str, params) -> "RefSH1":
        """params = (k, report_n, prefix_bits, max_memory, min_quality, max_read_n)"""
        assert params[0] == self.k
        return self.add_records(O.fastx_records(O.read_fastx(path)), params[4], params[5])

    def arrays(self):
        """(keys ascending u64, counts i32) read back with sh_kmer_count"""
        keys = np.array(sorted(self.keys), np.uint64)
        cnt = np.array([self.L.sh_kmer_count(self.buf, int(x)) for x in keys], np.int32)
        return keys, cnt

    def spectrum(self, max_count: int) -> np.ndarray:
        out = (C.c_double * (max_count + 1))()
        self.L.sh_count_spectrum(self.buf, out, max_count + 1)
        return np.array(out[:], np.float64)

    def close(self):
        if self.buf is not None:
            self.L.free_suffix_hash(self.buf)
            self.buf = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass
