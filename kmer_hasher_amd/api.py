"""Host-side mirror of the reference's R API for the index hot path (reference kmer_hash.R:5-28).

    make_kmer_hash(seq, k, do_sort=False)  <- make.kmer.hash  (kmer_hash.R:5-8)
    kmer_pos(ex_ptr, opt_flag)             <- kmer.pos        (kmer_hash.R:10-21)
    seq_kmer_pos(ex_ptr, seq, k)           <- seq.kmer.pos    (kmer_hash.R:23-28)
    kmer_pairs(ptr_a, ptr_b)               <- kmer.pairs      (kmer_hash.R:30-34), fixed
    count_kmers(seq, params, hash_ptr)     <- count.kmers     (kmer_hash.R:43-46)
    count_kmers_fq_sh_rp(fq, params, ptr)  <- count.kmers.fq.sh.rp (kmer_hash.R:75-78)
    seq_kmer_depth_sh(ptr, seq, k)         <- seq.kmer.depth.sh    (kmer_hash.R:80-83)
    kmer_spec_sh_n(ptr, max_count, comb, comb_inner, source_min)
                                           <- kmer.spec.sh.n       (kmer_hash.R:93-96)
    count_kmers_fq_sh(fq, params, ptr)     <- count.kmers.fq.sh    (kmer_hash.R:56-59)
    kmer_spec_sh(ptr, max_count)           <- kmer.spec.sh         (kmer_hash.R:89-91)
    set_row_order(ex_ptr, "khash")         kmer.pos rows in the reference's khash order (opt-in)
    set_max_occ(ex_ptr, n)                 queries drop the windows whose k-mer occurs > n times

Same argument meaning, same validation order and the reference's own error messages (raised as
``KmerHashError``, the analogue of R's error()).  Results follow the R wrappers after their
``t()``: ``pos`` is an (N, 2) int32 matrix with columns (i, pos), ``pair.pos`` (P, 3) with
(i, x, y), the query an (H, 2) matrix with (i, j).  Everything runs through libkmhgpu.so on the
GPU; nothing here computes a result on the CPU.

The external pointer is an ``ExtPtr`` carrying the reference's tag "kmer_hash_250930"
(src/kmer_hash.c:22) and a finaliser that frees the device index (finalise_khash_ptr,
src/kmer_hash.c:56-66).
"""
from __future__ import annotations

import ctypes as C
import warnings
import weakref

import numpy as np

from . import _lib

KMER_HASH_TAG = "kmer_hash_250930"
SUFFIX_HASH_N_TAG = "suffix_hash_n_250930"          # src/kmer_hash.c:25
SUFFIX_HASH_TAG = "suffix_hash_250930"              # src/kmer_hash.c:24
OPT_KMER, OPT_POS, OPT_PAIRS, OPT_COUNT = 1, 2, 4, 8
FIELDS = ("kmer", "pos", "pair.pos", "count")          # src/kmer_hash.c:18
INT_MAX = 2**31 - 1


class KmerHashError(ValueError):
    """R error() raised by the .Call bridge."""


class ExtPtr:
    """Analogue of the EXTPTRSXP returned by make_kmer_h_index."""

    def __init__(self, handle: int, tag: str = KMER_HASH_TAG):
        self._h = C.c_void_p(handle)
        self.tag = tag
        self._fin = weakref.finalize(self, ExtPtr._finalise, handle)

    @staticmethod
    def _finalise(handle):
        if handle:
            _lib.lib().kmhg_free(C.c_void_p(handle))

    @property
    def handle(self) -> C.c_void_p:
        if not self._h:
            raise KmerHashError("external pointer has been freed")
        return self._h

    def info(self) -> _lib.Info:
        inf = _lib.Info()
        _lib.check(_lib.lib().kmhg_index_info(self.handle, C.byref(inf)))
        return inf

    def free(self):
        if self._h:
            self._fin()
            self._h = C.c_void_p(0)


def _as_seq_bytes(seq, what: str) -> bytes:
    # as.character(seq); STRING_ELT(seq_r, 0) -- only the first element is used
    if isinstance(seq, (list, tuple)):
        if len(seq) < 1:
            raise KmerHashError(what)
        seq = seq[0]
    if isinstance(seq, str):
        return seq.encode("latin-1")
    if isinstance(seq, (bytes, bytearray)):
        return bytes(seq)
    if isinstance(seq, np.ndarray) and seq.dtype == np.uint8:
        return seq.tobytes()
    raise KmerHashError(what)


def _as_int(x, what: str) -> int:
    if isinstance(x, (list, tuple, np.ndarray)):
        if len(x) < 1:
            raise KmerHashError(what)
        x = x[0]
    try:
        return int(x)
    except (TypeError, ValueError):
        raise KmerHashError(what) from None


def make_kmer_hash(seq, k, do_sort=False, w=1) -> ExtPtr:
    """make.kmer.hash -> .Call("make_kmer_h_index", ...)  (src/kmer_hash.c:506-540).

    w > 1 (make.kmer.hash.min, not in the reference): an index of the (w,k)-minimizer windows
    alone (kmhg_build_sampled, include/kmhgpu.h); queries on it apply the same rule to the
    query sequence.  w = 1 calls exactly what it always called."""
    b = _as_seq_bytes(seq, "seq_r should be a character vector of length at least one")
    kk = _as_int(k, "k_r must be an integer vector of length at least one")
    ds = _as_int(do_sort, "sort_pos_r must be an integer vector of length at least one")
    ww = _as_int(w, "w must be between 1 and 256")
    out = C.c_void_p()
    if ww == 1:
        rc = _lib.lib().kmhg_build(b, len(b), kk, ds, C.byref(out))
    else:
        rc = _lib.lib().kmhg_build_sampled(b, len(b), kk, ww, ds, C.byref(out))
    if rc == _lib.KMHG_EINVAL:
        raise KmerHashError(_lib.lib().kmhg_last_error().decode())
    _lib.check(rc)
    return ExtPtr(out.value)


def get_sampling(ex_ptr) -> int:
    """The minimizer w an index was built with (kmhg_get_sampling); 1: every window."""
    if not isinstance(ex_ptr, ExtPtr):
        raise KmerHashError("ptr_r should be an external pointer")
    w = C.c_int()
    _lib.check(_lib.lib().kmhg_get_sampling(ex_ptr.handle, C.byref(w)))
    return w.value


def minimizer_mask(seq, k, w, rc=False) -> np.ndarray:
    """The (w,k)-minimizer selection of a sequence on the CPU (kmhg_minimizer_mask): a uint8
    array of L - k + 1 entries, entry s - 1 = 1 iff window start s is selected; rc: of the
    reverse complement, in its own coordinates."""
    b = _as_seq_bytes(seq, "seq_r should be a character vector of length at least one")
    kk = _as_int(k, "k should be an integer of length 1")
    ww = _as_int(w, "w must be between 1 and 256")
    n = b.find(b"\0")
    L = len(b) if n < 0 else n
    out = np.zeros(max(L - kk + 1, 1), dtype=np.uint8)
    r = _lib.lib().kmhg_minimizer_mask(b, len(b), kk, ww, 1 if rc else 0,
                                       out.ctypes.data_as(C.c_void_p))
    if r == _lib.KMHG_EINVAL:
        raise KmerHashError(_lib.lib().kmhg_last_error().decode())
    _lib.check(r)
    return out[:L - kk + 1]


def _extract(ptr) -> ExtPtr:
    # extract_khash_ptr, src/kmer_hash.c:491-503
    if not isinstance(ptr, ExtPtr):
        raise KmerHashError("ptr_r should be an external pointer")
    if ptr.tag != KMER_HASH_TAG:
        raise KmerHashError("External pointer has incorrect tag")
    return ptr


def kmer_pos(ex_ptr, opt_flag) -> dict:
    """kmer.pos -> .Call("kmer_positions", ...)  (src/kmer_hash.c:1054-1147).

    Returns {"kmer", "pos", "pair.pos", "count"}; unset flags give None (R's NULL)."""
    p = _extract(ex_ptr)
    if isinstance(opt_flag, (list, tuple, np.ndarray)) and len(opt_flag) != 1:
        raise KmerHashError("opt_flag_r should be an integer vector of length 1")
    opt = _as_int(opt_flag, "opt_flag_r should be an integer vector of length 1") & 0xFFFFFFFF
    L = _lib.lib()
    nk, npos, npair, ncnt = C.c_int64(), C.c_int64(), C.c_int64(), C.c_int64()
    _lib.check(L.kmhg_positions_size(p.handle, opt, C.byref(nk), C.byref(npos), C.byref(npair),
                                     C.byref(ncnt)))
    # R's allocMatrix takes an int ncol: the reference overflows silently; we refuse cleanly.
    if npair.value > INT_MAX or npos.value > INT_MAX:
        raise KmerHashError("result has more than 2^31-1 columns (R matrix limit)")
    k = p.info().k
    kb = np.empty(nk.value * (k + 1), np.uint8) if opt & OPT_KMER else None
    pos = np.empty(2 * npos.value, np.int32) if opt & OPT_POS else None
    pairs = np.empty(3 * npair.value, np.int32) if opt & OPT_PAIRS else None
    cnt = np.empty(ncnt.value, np.int32) if opt & OPT_COUNT else None

    def ptr(a):
        return a.ctypes.data if a is not None and a.size else None

    _lib.check(L.kmhg_positions_fill(p.handle, opt, ptr(kb), ptr(pos), ptr(pairs), ptr(cnt)))
    out = dict.fromkeys(FIELDS)
    if kb is not None:
        out["kmer"] = [x.decode() for x in kb.reshape(-1, k + 1)[:, :k].view(f"S{k}").ravel()] \
            if nk.value else []
    if pos is not None:
        out["pos"] = pos.reshape(-1, 2)          # t(tmp$pos): columns i, pos
    if pairs is not None:
        out["pair.pos"] = pairs.reshape(-1, 3)   # t(tmp$pair.pos): columns i, x, y
    if cnt is not None:
        out["count"] = cnt
    return out


def kmer_pairs(ptr_a, ptr_b) -> np.ndarray:
    """kmer.pairs -> .Call("kmer_pair_pos", ...)  (src/kmer_hash.c:1174-1203, kmer_hash.R:30-34).

    Returns an (M, 2) int32 matrix with columns (a, b): for every k-mer held by both indices,
    each position in a paired with each position in b (a outer, b inner), k-mers in a's kmer.pos
    row order.  Defined where the reference crashes (empty buckets of a, out-of-bounds kh_exist
    on b); the indices must share k."""
    a, b = _extract(ptr_a), _extract(ptr_b)
    L = _lib.lib()
    q = C.c_void_p()
    h = C.c_int64()
    rc = L.kmhg_pairs_run(a.handle, b.handle, C.byref(q), C.byref(h))
    if rc == _lib.KMHG_EINVAL:
        raise KmerHashError(L.kmhg_last_error().decode())
    _lib.check(rc)
    try:
        if h.value > INT_MAX:
            raise KmerHashError("result has more than 2^31-1 columns (R matrix limit)")
        rows = np.empty(2 * h.value, np.int32)
        if h.value:
            _lib.check(L.kmhg_query_fill(q, rows.ctypes.data))
    finally:
        L.kmhg_query_free(q)
    return rows.reshape(-1, 2)


def set_row_order(ex_ptr, order: str = "first") -> None:
    """Label kmer.pos k-mers by first occurrence ("first", the default) or in the reference's own
    khash bucket order ("khash": byte-identical kmer.pos output, src/kmer_hash.c:1096-1124).
    KMHG_ROW_ORDER=khash in the environment makes "khash" the default for new indices."""
    p = _extract(ex_ptr)
    code = {"first": _lib.KMHG_ORDER_FIRST, "khash": _lib.KMHG_ORDER_KHASH}.get(order)
    if code is None:
        raise KmerHashError("order must be 'first' or 'khash'")
    _lib.check(_lib.lib().kmhg_set_row_order(p.handle, code))


def set_max_occ(ex_ptr, max_occ=0) -> int:
    """kmer.max.occ (not in the reference): the occurrence cap of later queries on a position
    index.  0 is off; with max_occ = n >= 1 a query window whose k-mer occurs at more than n
    positions of the index yields no hit, in seq_kmer_pos / seq_kmer_pos_rc, seq_kmer_segs,
    seq_kmer_blocks, seq_kmer_chains and seq_kmer_raster alike (include/kmhgpu.h,
    kmhg_set_max_occ); kmer_pos, kmer_pairs and the counting entries ignore it.  Returns the
    value read just before the set (two library calls: with another thread setting the same index
    at that moment it need not be the value this call replaced)."""
    p = _extract(ex_ptr)
    n = _as_int(max_occ, "max.occ must be between 0 and 2^31-1")
    if not -2**63 <= n < 2**63:
        raise KmerHashError("max.occ must be between 0 and 2^31-1")
    before = get_max_occ(ex_ptr)
    rc = _lib.lib().kmhg_set_max_occ(p.handle, n)
    if rc == _lib.KMHG_EINVAL:
        raise KmerHashError(_lib.lib().kmhg_last_error().decode())
    _lib.check(rc)
    return before


def get_max_occ(ex_ptr) -> int:
    """The index's occurrence cap (set_max_occ); 0: none."""
    p = _extract(ex_ptr)
    n = C.c_int64()
    _lib.check(_lib.lib().kmhg_get_max_occ(p.handle, C.byref(n)))
    return n.value


def seq_kmer_pos(ex_ptr, seq, k) -> np.ndarray:
    """seq.kmer.pos -> .Call("sequence_kmer_positions", ...)  (src/kmer_hash.c:1151-1172).

    Returns an (H, 2) int32 matrix with columns (i, j): i = 1-based end of the query window,
    j = 1-based start of the indexed occurrence; rows ordered by i then j."""
    return _seq_kmer_pos(ex_ptr, seq, k, "kmhg_query_run")


def seq_kmer_pos_rc(ex_ptr, seq, k) -> np.ndarray:
    """seq.kmer.pos.rc: seq.kmer.pos of the REVERSE COMPLEMENT of seq, made on the device from
    the forward string -- what the reference's usage script writes as
    seq.kmer.pos(hash, reverseComplement(x), k) (test.R:42-43), with rev.comp's 2-bit rule
    (test.R:31-36) except that N stays N (rev.comp would turn it into C).

    Returns the same (H, 2) int32 matrix as seq_kmer_pos would for rc(seq): i = 1-based end of
    the window in rc(seq), j = 1-based start of the indexed occurrence, ordered by i then j.  A
    row's window starts at forward position len(seq) - i + 1 (1-based) of seq.  Runs on the
    index's device (KMHG_DEVICES is not honoured)."""
    return _seq_kmer_pos(ex_ptr, seq, k, "kmhg_query_run_rc")


_STRANDS = {"both": 3, "forward": 1, "fwd": 1, "+": 1, "reverse": 2, "rev": 2, "-": 2,
            0: 3, 1: 1, -1: 2}


def _reads_query(ex_ptr, reads, k, strand, max_reads):
    """Runs reads.kmer.pos; returns (library, rquery handle, rows, reads)."""
    p = _extract(ex_ptr)
    if isinstance(k, (list, tuple, np.ndarray)) and len(k) != 1:
        raise KmerHashError("k should be an integer of length 1")
    kk = _as_int(k, "k should be an integer of length 1")
    if kk < 1 or kk > 31:
        raise KmerHashError("k should be between 1 and 31")
    try:
        strands = _STRANDS[strand]
    except (KeyError, TypeError):
        raise KmerHashError('strand should be "both", "forward" or "reverse"') from None
    L = _lib.lib()
    q = C.c_void_p()
    h = C.c_int64()
    if isinstance(reads, (str, bytes)):          # a FASTA / FASTQ file, gzipped or not
        path = reads.encode() if isinstance(reads, str) else reads
        r = C.c_void_p()
        _lib.check(L.kmhg_fastx_read(path, int(max_reads), 0, C.byref(r)))
        try:
            nr = C.c_int64()
            _lib.check(L.kmhg_reads_info(r, None, C.byref(nr), None))
            rc = L.kmhg_reads_query_run(p.handle, r, kk, strands, C.byref(q), C.byref(h))
        finally:
            L.kmhg_reads_free(r)
        n_reads = nr.value
    else:
        if not isinstance(reads, (list, tuple)):
            raise KmerHashError("reads should be a list of sequences or a file name")
        bs = []
        for x in reads:
            if isinstance(x, str):
                x = x.encode("latin-1")
            elif not isinstance(x, (bytes, bytearray)):
                raise KmerHashError("reads should be a list of sequences or a file name")
            z = x.find(b"\0")                    # a C string ends at its first NUL
            bs.append(bytes(x) if z < 0 else bytes(x[:z]))
        n_reads = len(bs)
        off = np.zeros(n_reads + 1, np.int64)
        np.cumsum([len(b) for b in bs], out=off[1:])
        seq = np.frombuffer(b"".join(bs) + b"\0", np.uint8)
        rc = L.kmhg_reads_query_run_packed(p.handle, seq.ctypes.data, int(off[-1]),
                                           off.ctypes.data, n_reads, kk, strands, C.byref(q),
                                           C.byref(h))
    if rc == _lib.KMHG_EINVAL:
        raise KmerHashError(L.kmhg_last_error().decode())
    _lib.check(rc)
    return L, q, h.value, n_reads


def reads_kmer_pos(ex_ptr, reads, k, strand="both", max_reads=INT_MAX) -> np.ndarray:
    """reads.kmer.pos (not in the reference): every read of a batch against a position index, on
    both strands, in one device call.

    reads: a list of str or bytes, one read each, or the name of a FASTA / FASTQ file (gzipped or
    not).  A file is read with kmhg_fastx_read(path, max_reads, 0): with k = 0 that call keeps
    every non-empty record, so read numbers are the numbers of the file's non-empty records.
    strand: "both", "forward" or "reverse".

    Returns an (H, 4) int32 matrix with columns (read, strand, i, j): read 1-based, strand +1 or
    -1; the rows of read r on strand +1 are exactly seq_kmer_pos(ptr, read_r, k), those on strand
    -1 exactly seq_kmer_pos_rc(ptr, read_r, k) (i in rc(read_r)'s coordinates); ordered by read,
    forward before reverse, then (i, j).  A read of at most k bases has no row."""
    L, q, h, _ = _reads_query(ex_ptr, reads, k, strand, max_reads)
    try:
        if h > INT_MAX:
            raise KmerHashError("result has more than 2^31-1 rows (R matrix limit)")
        rows = np.empty(4 * h, np.int32)
        if h:
            _lib.check(L.kmhg_rquery_fill(q, rows.ctypes.data))
    finally:
        L.kmhg_rquery_free(q)
    return rows.reshape(-1, 4)


def reads_kmer_vote(ex_ptr, reads, k, band=64, strand="both", max_reads=INT_MAX) -> np.ndarray:
    """reads.kmer.vote (not in the reference): where each read of reads_kmer_pos(ptr, reads, k,
    strand) lies.  A row votes for pos = j - i + k, the index position of base 1 of the read
    (strand +1) or of its reverse complement (strand -1), possibly <= 0, in the cell (strand,
    floor(pos / band)); 1 <= band <= 2^30.

    Returns an (n_reads, 6) int32 matrix (read, strand, pos, hits, second, total), one row per
    read in read order: the cell with the most votes (ties: forward, then the smaller bin) as
    strand and pos = bin * band, its votes, the most votes among the read's other cells, and all
    of the read's rows; (r, 0, 0, 0, 0, 0) for a read without rows."""
    bb = _as_int(band, "band should be an integer of length 1")
    if bb < 1 or bb > 2**30:
        raise KmerHashError("band must be between 1 and 2^30")
    L, q, _, n_reads = _reads_query(ex_ptr, reads, k, strand, max_reads)
    try:
        votes = np.empty(6 * n_reads, np.int32)
        if n_reads:
            rc = L.kmhg_rquery_votes(q, bb, votes.ctypes.data)
            if rc == _lib.KMHG_EINVAL:
                raise KmerHashError(L.kmhg_last_error().decode())
            _lib.check(rc)
    finally:
        L.kmhg_rquery_free(q)
    return votes.reshape(-1, 6)


def seq_kmer_segs(ex_ptr, seq, k, min_len=1, rc=False, row_free=False) -> np.ndarray:
    """seq.kmer.segs (not in the reference): the dot plot of seq against the index as maximal
    diagonal segments instead of points.

    Runs seq.kmer.pos (rc=False) or seq.kmer.pos.rc (rc=True) on the device and returns an (S, 3)
    int32 matrix with columns (i, j, len), ordered by (i, j): rows (i + t, j + t), 0 <= t < len,
    are all in the seq.kmer.pos result and neither (i - 1, j - 1) nor (i + len, j + len) is.  len
    counts windows; the exact match covers len + k - 1 bases.  min_len keeps the segments of at
    least that many rows; with min_len = 1 the segments expand back to exactly the rows.  Only a
    position index (make_kmer_hash) is accepted: a counts index's "positions" are count vectors,
    not ascending.

    row_free=True takes the route that never writes the rows (kmhg_segments_run): the same
    matrix, byte for byte, also where the query has more than 2^31 - 1 rows and the default
    route refuses; it runs on the index's device."""
    L = _lib.lib()
    need, ints = "segments need a position index", [(min_len, "min_len must be a positive integer")]
    g = C.c_void_p()
    n = C.c_int64()
    if row_free:
        p, b, kk, (ml,) = _dot_plot_args(ex_ptr, seq, k, need, ints)
        try:
            rcode = L.kmhg_segments_run(p.handle, b, len(b), kk, 1 if rc else 0, ml, C.byref(g),
                                        C.byref(n), None)
            return _records_matrix(L, rcode, L.kmhg_segs_fill, g, n.value, 3)
        finally:
            L.kmhg_segs_free(g)
    q, _, (ml,) = _dot_plot_query(ex_ptr, seq, k, rc, need, ints)
    try:
        rcode = L.kmhg_query_segments(q, ml, C.byref(g), C.byref(n))
        if rcode == _lib.KMHG_EINVAL:
            raise KmerHashError(L.kmhg_last_error().decode())
        _lib.check(rcode)
        segs = np.empty(3 * n.value, np.int32)
        if n.value:
            _lib.check(L.kmhg_segs_fill(g, segs.ctypes.data))
    finally:
        L.kmhg_segs_free(g)
        L.kmhg_query_free(q)
    return segs.reshape(-1, 3)


def _records_matrix(L, rcode, fill, handle, n, cols) -> np.ndarray:
    """The (n, cols) int32 matrix of a segs / blocks handle a row-free entry returned with rcode."""
    if rcode in (_lib.KMHG_EINVAL, _lib.KMHG_EOVERFLOW):
        raise KmerHashError(L.kmhg_last_error().decode())
    _lib.check(rcode)
    out = np.empty(cols * n, np.int32)
    if n:
        _lib.check(fill(handle, out.ctypes.data))
    return out.reshape(-1, cols)


def _dot_plot_args(ex_ptr, seq, k, need, ints):
    """What the dot-plot summaries check before any query runs: a position index (`need`: the
    message for any other index), one sequence, k, then the integers of `ints`, (value, message)
    pairs (a value of None stands for k).  Returns (index, sequence bytes, k, integers)."""
    p = _extract(ex_ptr)
    if p.info().kind != 0:
        raise KmerHashError(need)
    if isinstance(seq, (list, tuple)) and len(seq) != 1:
        raise KmerHashError("seq_r should be a single sequence")
    b = _as_seq_bytes(seq, "seq_r should be a single sequence")
    if isinstance(k, (list, tuple, np.ndarray)) and len(k) != 1:
        raise KmerHashError("k should be an integer of length 1")
    kk = _as_int(k, "k should be an integer of length 1")
    vals = [kk if v is None else _as_int(v, msg) for v, msg in ints]
    return p, b, kk, vals


def _dot_plot_query(ex_ptr, seq, k, rc, need, ints):
    """The query handle of seq.kmer.pos (rc=False) or seq.kmer.pos.rc (rc=True) of one sequence
    against a position index (`need`: the message for any other index), which the caller frees;
    with it k and the integers of `ints`, (value, message) pairs converted after k and before the
    query runs (a value of None stands for k)."""
    p, b, kk, vals = _dot_plot_args(ex_ptr, seq, k, need, ints)
    L = _lib.lib()
    q = C.c_void_p()
    h = C.c_int64()
    rcode = (L.kmhg_query_run_rc if rc else L.kmhg_query_run)(p.handle, b, len(b), kk,
                                                              C.byref(q), C.byref(h))
    if rcode == _lib.KMHG_EINVAL:
        raise KmerHashError(L.kmhg_last_error().decode())
    _lib.check(rcode)
    return q, kk, vals


def seq_kmer_blocks(ex_ptr, seq, k, max_gap=None, min_len=1, min_hits=1, rc=False,
                    row_free=False) -> np.ndarray:
    """seq.kmer.blocks (not in the reference): the dot plot of seq against the index as diagonal
    segments merged across small gaps.

    Takes the segments seq_kmer_segs(ex_ptr, seq, k, min_len, rc) gives and, on every diagonal,
    joins neighbours whose gap -- the windows between the end of one and the start of the next --
    is at most max_gap.  Returns a (B, 4) int32 matrix with columns (i, j, span, hits), ordered
    by (i, j): the block starts at row (i, j), covers span windows of its diagonal from its first
    row to its last, and holds hits rows of the seq.kmer.pos result (span - hits is the sum of
    its gaps).  min_hits keeps the blocks with at least that many rows.  max_gap=None means k: one
    isolated substitution removes k consecutive windows from a diagonal, and a gap of k bridges
    it.  max_gap = 0 gives the segments themselves as (i, j, len, len).  Only a position index
    (make_kmer_hash) is accepted.

    row_free=True takes the route that never writes the rows (kmhg_blocks_run), as in
    seq_kmer_segs: the same matrix, byte for byte, also beyond 2^31 - 1 rows."""
    L = _lib.lib()
    need = "blocks need a position index"
    ints = [(min_len, "min_len must be a positive integer"), (max_gap, "max_gap must not be negative"),
            (min_hits, "min_hits must be a positive integer")]
    g = C.c_void_p()
    n = C.c_int64()
    if row_free:
        p, b, kk, (ml, mg, mh) = _dot_plot_args(ex_ptr, seq, k, need, ints)
        try:
            rcode = L.kmhg_blocks_run(p.handle, b, len(b), kk, 1 if rc else 0, ml, mg, mh,
                                      C.byref(g), C.byref(n), None)
            return _records_matrix(L, rcode, L.kmhg_blocks_fill, g, n.value, 4)
        finally:
            L.kmhg_blocks_free(g)
    q, _, (ml, mg, mh) = _dot_plot_query(ex_ptr, seq, k, rc, need, ints)
    try:
        rcode = L.kmhg_query_blocks(q, ml, mg, mh, C.byref(g), C.byref(n))
        if rcode == _lib.KMHG_EINVAL:
            raise KmerHashError(L.kmhg_last_error().decode())
        _lib.check(rcode)
        blocks = np.empty(4 * n.value, np.int32)
        if n.value:
            _lib.check(L.kmhg_blocks_fill(g, blocks.ctypes.data))
    finally:
        L.kmhg_blocks_free(g)
        L.kmhg_query_free(q)
    return blocks.reshape(-1, 4)


def seq_kmer_chains(ex_ptr, seq, k, max_dist=5000, max_drift=500, max_gap=None, min_len=1,
                    min_hits=1, rc=False, row_free=False) -> dict:
    """seq.kmer.chains (not in the reference): the blocks of seq_kmer_blocks linked across
    diagonals into chains.

    An indel shifts the diagonal and splits one alignment into several blocks.  Block a may precede
    block b when b starts after a ends in both coordinates, the larger of the two gaps (in windows)
    is at most max_dist and their difference -- the diagonal shift -- at most max_drift (minimap2's
    -g and -r).  Every block chooses its nearest such predecessor (the smallest sum of the two
    gaps, then the lower block), every block keeps the nearest of the blocks that chose it, and the
    links both ends agree on form the chains (include/kmhgpu.h has the definition; this is greedy
    nearest-neighbour chaining, not minimap2's dynamic program).

    Returns {"chains": (C, 6) int32 with columns (i, j, i.end, j.end, hits, blocks), ordered by
    (i, j); "blocks": the (B, 4) int32 blocks seq_kmer_blocks(ex_ptr, seq, k, max_gap, min_len, 1,
    rc) gives; "chain": (B,) int32, the 1-based row of `chains` each block belongs to, 0 where
    min_hits dropped its chain}.  min_hits keeps the chains of at least that many rows.  max_gap
    and row_free are seq_kmer_blocks'.  Only a position index (make_kmer_hash) is accepted."""
    L = _lib.lib()
    need = "blocks need a position index"
    ints = [(min_len, "min_len must be a positive integer"), (max_gap, "max_gap must not be negative"),
            (max_dist, "max_dist must not be negative"), (max_drift, "max_drift must not be negative"),
            (min_hits, "min_hits must be a positive integer")]
    p, b, kk, (ml, mg, md, mr, mh) = _dot_plot_args(ex_ptr, seq, k, need, ints)
    g = C.c_void_p()
    nc, nb = C.c_int64(), C.c_int64()
    try:
        rcode = L.kmhg_chains_run(p.handle, b, len(b), kk, 1 if rc else 0, 1 if row_free else 0, ml,
                                  mg, md, mr, mh, C.byref(g), C.byref(nc), C.byref(nb), None)
        if rcode in (_lib.KMHG_EINVAL, _lib.KMHG_EOVERFLOW):
            raise KmerHashError(L.kmhg_last_error().decode())
        _lib.check(rcode)
        chains = np.empty(6 * nc.value, np.int32)
        blocks = np.empty(4 * nb.value, np.int32)
        member = np.empty(nb.value, np.int32)
        if nc.value:
            _lib.check(L.kmhg_chains_fill(g, chains.ctypes.data))
        if nb.value:
            _lib.check(L.kmhg_chains_member_fill(g, member.ctypes.data, blocks.ctypes.data))
    finally:
        L.kmhg_chains_free(g)
    return {"chains": chains.reshape(-1, 6), "blocks": blocks.reshape(-1, 4), "chain": member}


def raster_axis(lo: int, hi: int, bins: int) -> tuple[int, int]:
    """(bin width, bin count) of `bins` bins over lo..hi: width = ceil(length / bins), then
    count = ceil(length / width) -- at most `bins`, and the last bin may reach past hi."""
    n = hi - lo + 1
    width = -(-n // bins)
    return width, -(-n // width)


def _as_range(r, default_hi: int, what: str) -> tuple[int, int]:
    if r is None:
        return 1, default_hi
    if not isinstance(r, (list, tuple, np.ndarray)) or len(r) != 2:
        raise KmerHashError(what)
    lo, hi = _as_int(r[0], what), _as_int(r[1], what)
    if lo < 1 or hi < lo:
        raise KmerHashError(what)
    return lo, hi


def seq_kmer_raster(ex_ptr, seq, k, bins=1024, rc=False, i_range=None, j_range=None) -> dict:
    """seq.kmer.raster (not in the reference): the dot plot of seq against the index as a binned
    count matrix -- what one draws when the rows themselves are too many to hold or plot.

    Bins the rows of seq.kmer.pos (rc=False) or seq.kmer.pos.rc (rc=True) over i_range x j_range
    (inclusive 1-based (lo, hi) pairs; default 1..len(seq) and 1..index length) into `bins` bins
    per axis (a scalar or an (i, j) pair): bin width = ceil(range length / bins), bin count =
    ceil(range length / width).  Returns {"counts": int64 (n_i, n_j) matrix, "i0", "j0", "bin_i",
    "bin_j", "n_rows"}: counts[bi, bj] is the number of rows with (i - i0) // bin_i == bi and
    (j - j0) // bin_j == bj, n_rows the hit total of the whole query (inside the ranges or not).
    The rows are never written, so the result's size does not depend on the hit count and
    n_rows may exceed 2^31 - 1 where seq_kmer_pos refuses.  Only a position index
    (make_kmer_hash) is accepted; runs on the index's device."""
    p = _extract(ex_ptr)
    L = _lib.lib()
    inf = p.info()
    if inf.kind != 0:
        raise KmerHashError("a raster needs a position index")
    if isinstance(seq, (list, tuple)) and len(seq) != 1:
        raise KmerHashError("seq_r should be a single sequence")
    b = _as_seq_bytes(seq, "seq_r should be a single sequence")
    if isinstance(k, (list, tuple, np.ndarray)) and len(k) != 1:
        raise KmerHashError("k should be an integer of length 1")
    kk = _as_int(k, "k should be an integer of length 1")
    msg = "bins should be one or two positive integers"
    if isinstance(bins, (list, tuple, np.ndarray)):
        if len(bins) not in (1, 2):
            raise KmerHashError(msg)
        nb = [_as_int(x, msg) for x in bins] * (2 if len(bins) == 1 else 1)
    else:
        nb = [_as_int(bins, msg)] * 2
    if min(nb) < 1:
        raise KmerHashError(msg)
    i_lo, i_hi = _as_range(i_range, max(len(b), 1), "i.range should be c(lo, hi) with 1 <= lo <= hi")
    j_lo, j_hi = _as_range(j_range, max(int(inf.seq_len), 1),
                           "j.range should be c(lo, hi) with 1 <= lo <= hi")
    bin_i, n_i = raster_axis(i_lo, i_hi, nb[0])
    bin_j, n_j = raster_axis(j_lo, j_hi, nb[1])
    frame = (C.c_int64 * 6)(i_lo, j_lo, bin_i, bin_j, n_i, n_j)
    cells = n_i * n_j
    out = np.empty(cells if cells <= 1 << 26 else 1, np.uint32)   # (beyond: refused, nothing written)
    h = C.c_int64()
    rcode = L.kmhg_raster_run(p.handle, b, len(b), kk, 1 if rc else 0, frame, out.ctypes.data,
                              C.byref(h))
    if rcode in (_lib.KMHG_EINVAL, _lib.KMHG_EOVERFLOW):
        raise KmerHashError(L.kmhg_last_error().decode())
    _lib.check(rcode)
    return {"counts": out.astype(np.int64).reshape(n_j, n_i).T, "i0": i_lo, "j0": j_lo,
            "bin_i": bin_i, "bin_j": bin_j, "n_rows": h.value}


def _seq_kmer_pos(ex_ptr, seq, k, entry) -> np.ndarray:
    p = _extract(ex_ptr)
    if isinstance(seq, (list, tuple)) and len(seq) != 1:
        raise KmerHashError("seq_r should be a single sequence")
    b = _as_seq_bytes(seq, "seq_r should be a single sequence")
    if isinstance(k, (list, tuple, np.ndarray)) and len(k) != 1:
        raise KmerHashError("k should be an integer of length 1")
    kk = _as_int(k, "k should be an integer of length 1")
    L = _lib.lib()
    q = C.c_void_p()
    h = C.c_int64()
    rc = getattr(L, entry)(p.handle, b, len(b), kk, C.byref(q), C.byref(h))
    if rc == _lib.KMHG_EINVAL:
        raise KmerHashError(L.kmhg_last_error().decode())
    _lib.check(rc)
    try:
        if h.value > INT_MAX:
            raise KmerHashError("result has more than 2^31-1 columns (R matrix limit)")
        rows = np.empty(2 * h.value, np.int32)
        if h.value:
            _lib.check(L.kmhg_query_fill(q, rows.ctypes.data))
    finally:
        L.kmhg_query_free(q)
    return rows.reshape(-1, 2)


def count_kmers(seq, params, hash_ptr=None) -> ExtPtr:
    """count.kmers -> .Call("count_kmers", hash.ptr, params, seq)  (src/kmer_hash.c:548-591).

    seq: a character vector (str or list of str); params = (k, source, source_n).  Every valid
    window of every sequence adds one to entry `source` of its k-mer's vector of source_n
    counts.  hash_ptr None makes a new counts pointer; otherwise the counts are added to it and
    the same pointer is returned.  kmer.pos / seq.kmer.pos read the count vectors as positions,
    as the reference does (test.R:340-343)."""
    if isinstance(seq, (str, bytes, bytearray)):
        seq = [seq]
    if not isinstance(seq, (list, tuple)) or len(seq) < 1 or \
            not all(isinstance(x, (str, bytes, bytearray)) for x in seq):
        raise KmerHashError("seq_r should be a character vector of length at least one")
    try:
        prm = [int(x) for x in params]
    except (TypeError, ValueError):
        raise KmerHashError("k_r must be an integer vector of length 3") from None
    if len(prm) != 3:
        raise KmerHashError("k_r must be an integer vector of length 3")
    k, source, source_n = prm
    if k < 1 or k > 32:
        raise KmerHashError("k must be a positive integer less than 1+MAX_K")
    if source_n < 1 or source >= source_n:
        raise KmerHashError("source_n must be larger than 1 and larger than source")
    if hash_ptr is not None and (not isinstance(hash_ptr, ExtPtr) or
                                 hash_ptr.tag != KMER_HASH_TAG or not hash_ptr._h):
        # extract_ext_ptr returns NULL (src/kmer_hash.c:574-577)
        raise KmerHashError("failed to extract kmer_hash from external pointer")
    bs = [x.encode("latin-1") if isinstance(x, str) else bytes(x) for x in seq]
    arr = (C.c_char_p * len(bs))(*bs)
    lens = (C.c_size_t * len(bs))(*[len(b) for b in bs])
    h = C.c_void_p(hash_ptr._h.value if hash_ptr is not None and hash_ptr._h else None)
    L = _lib.lib()
    rc = L.kmhg_count(C.byref(h), arr, lens, len(bs), k, source, source_n)
    if rc == _lib.KMHG_EINVAL:
        raise KmerHashError(L.kmhg_last_error().decode())
    _lib.check(rc)
    if source < 0:   # kmer_count_insert: one warning() per window, nothing counted
        warnings.warn(f"source ({source % 2**64}) equal to or larger than source_n ({source_n})")
    if hash_ptr is not None:
        return hash_ptr
    return ExtPtr(h.value)


# ------------------------------------------------------------------ read counting (suffix hash)
def _int_vec(x, n: int | None, what: str) -> list[int]:
    if isinstance(x, (int, np.integer)):
        x = [x]
    try:
        v = [int(a) for a in x]
    except (TypeError, ValueError):
        raise KmerHashError(what) from None
    if n is not None and len(v) != n:
        raise KmerHashError(what)
    return v


def _extract_sh(ptr):
    # extract_ext_ptr(hash_ptr_r, suffix_hash_n_tag): NULL for anything else (src/kmer_hash.c:41-52)
    if isinstance(ptr, ExtPtr) and ptr.tag == SUFFIX_HASH_N_TAG and ptr._h:
        return ptr
    return None


def count_kmers_fq_sh_rp(fq_file, params, hash_ptr=None) -> ExtPtr:
    """count.kmers.fq.sh.rp -> .Call("count_kmers_fastq_sh_rp", hash.ptr, params, fq.file)
    (src/kmer_hash.c:810-857; reader src/kmer_reader.c:41-147).

    params = (k, prefix_bits, min_q, thread_n, max_reads, max_mem, source_n, source).  Counts the
    canonical k-mers of the FASTA/FASTQ file (plain or gzip) the reference's quality iterator
    accepts into entry `source` of a suffix hash of source_n counts.  A hash_ptr that is not a
    suffix hash is ignored and a new one returned, as extract_ext_ptr yields NULL for it."""
    if isinstance(fq_file, (list, tuple)):
        if len(fq_file) != 1:
            raise KmerHashError("fq_file should be a character vector of length at least one")
        fq_file = fq_file[0]
    if not isinstance(fq_file, (str, bytes)):
        raise KmerHashError("fq_file should be a character vector of length at least one")
    prm = _int_vec(params, 8, "k_r must be an integer vector of length 6 (k, prefix_bits, min_q, "
                              "thread_n, max_reads, max_mem, source_n, source")
    sh = _extract_sh(hash_ptr)
    h = C.c_void_p(sh._h.value if sh is not None else None)
    arr = (C.c_int32 * 8)(*[((x + 2**31) % 2**32) - 2**31 for x in prm])
    path = fq_file.encode() if isinstance(fq_file, str) else fq_file
    L = _lib.lib()
    rc = L.kmhg_sh_count_fastq(C.byref(h), path, arr)
    if rc == _lib.KMHG_EINVAL:
        raise KmerHashError(L.kmhg_last_error().decode())
    _lib.check(rc)
    if sh is not None:
        return sh
    return ExtPtr(h.value, tag=SUFFIX_HASH_N_TAG)


def seq_kmer_depth_sh(hash_ptr, seq, k) -> np.ndarray:
    """seq.kmer.depth.sh -> .Call("seq_kmer_depth_sh", hash.ptr, seq, k)
    (src/kmer_hash.c:859-879, seq_kmer_counts src/kmer_reader.c:155-193).

    Returns the (counts_n, L) int32 matrix R gets (no t() in the wrapper); NA is INT_MIN."""
    sh = _extract_sh(hash_ptr)
    if sh is None:
        raise KmerHashError("unable to obtain suffix_hash_n from external pointer")
    if isinstance(k, (list, tuple, np.ndarray)) and len(k) != 1:
        raise KmerHashError("k_r should be a single integer")
    kk = _as_int(k, "k_r should be a single integer")
    if isinstance(seq, (list, tuple)) and len(seq) != 1:
        raise KmerHashError("seq_r should be a character vector of length 1")
    b = _as_seq_bytes(seq, "seq_r should be a character vector of length 1")
    S = sh.info().sources
    out = np.empty(max(len(b) * S, 1), np.int32)
    L = _lib.lib()
    rc = L.kmhg_sh_depth(sh.handle, b, len(b), kk, out.ctypes.data)
    if rc == _lib.KMHG_EINVAL:
        raise KmerHashError(L.kmhg_last_error().decode())
    _lib.check(rc)
    return out[:len(b) * S].reshape(len(b), S).T


def kmer_spec_sh_n(hash_ptr, max_count, comb, comb_inner, source_min) -> np.ndarray:
    """kmer.spec.sh.n -> .Call("kmer_spectrum_suffix_hash_n", ...)  (src/kmer_hash.c:1010-1039,
    sh_count_spectrum_nc src/suffix_hash.c:338-421).

    Returns the (comb_n * counts_n, max_count + 1) float64 matrix; an invalid comb / comb_inner
    gives zeros and the reference's message, as its Rprintf branch does."""
    sh = _extract_sh(hash_ptr)
    if sh is None:
        raise KmerHashError("unable to obtain suffix_hash_n from external pointer")
    mc = _int_vec(max_count, 1, "max_count_r should be a single integer")[0]
    cb = _int_vec(comb, None, "comb_r should be an integer vector of length > 0")
    if len(cb) < 1:
        raise KmerHashError("comb_r should be an integer vector of length > 0")
    ci = _int_vec(comb_inner, None,
                  "comb_inner_r should be an integer vector of the same length as comb_r")
    if len(ci) != len(cb):
        raise KmerHashError("comb_inner_r should be an integer vector of the same length as comb_r")
    S = sh.info().sources
    sm = _int_vec(source_min, None,
                  "source_min_r should be an integer vector of length sh->counts_n")
    if len(sm) != S:
        raise KmerHashError("source_min_r should be an integer vector of length sh->counts_n")
    a32 = lambda v: np.array([((x + 2**31) % 2**32) - 2**31 for x in v], np.int32)  # noqa: E731
    cb_a, ci_a, sm_a = a32(cb), a32(ci), a32(sm)
    if mc < 0:
        raise KmerHashError("max_count must be >= 0")
    out = np.zeros(max((mc + 1) * len(cb) * S, 1), np.float64)
    st = C.c_int(0)
    L = _lib.lib()
    rc = L.kmhg_sh_spectrum(sh.handle, mc, cb_a.ctypes.data, ci_a.ctypes.data, len(cb),
                            sm_a.ctypes.data, len(sm), out.ctypes.data, C.byref(st))
    if rc == _lib.KMHG_EINVAL:
        raise KmerHashError(L.kmhg_last_error().decode())
    _lib.check(rc)
    if st.value != 1:
        warnings.warn(f"sh_count_spectrum_nc returned an error: {st.value}")
    return out[:(mc + 1) * len(cb) * S].reshape(mc + 1, len(cb) * S).T


# ------------------------------------------------------------------ single suffix hash
def count_kmers_fq_sh(fq_file, params, hash_ptr=None) -> ExtPtr:
    """count.kmers.fq.sh -> .Call("count_kmers_fastq_sh", hash.ptr, params, fq.file)
    (src/kmer_hash.c:715-806; walk seq_to_counts_sh :296-332).

    params = (k, report_n, prefix_bits, max_memory, min_quality, max_read_n).  Counts the canonical
    k-mers the reference's character-threshold walk accepts into a single suffix hash (tag
    "suffix_hash_250930", info.kind 3).  hash_ptr None makes a new one; anything else must be a
    pointer this function returned."""
    if isinstance(fq_file, (list, tuple)):
        if len(fq_file) != 1:
            raise KmerHashError("fq_file should be a character vector of length at least one")
        fq_file = fq_file[0]
    if not isinstance(fq_file, (str, bytes)):
        raise KmerHashError("fq_file should be a character vector of length at least one")
    prm = _int_vec(params, 6, "k_r must be an integer vector of length 3")
    prm = [((x + 2**31) % 2**32) - 2**31 for x in prm]
    if prm[1] < 1:
        warnings.warn("negative or 0 report n value specified: set to 1e6")
    if prm[0] < 1 or prm[0] > 32:
        raise KmerHashError("k must be a positive integer less than 1+MAX_K")
    if hash_ptr is not None and not (isinstance(hash_ptr, ExtPtr) and
                                     hash_ptr.tag == SUFFIX_HASH_TAG and hash_ptr._h):
        raise KmerHashError("Unable to extract suffix_hash from external pointer")
    h = C.c_void_p(hash_ptr._h.value if hash_ptr is not None else None)
    arr = (C.c_int32 * 6)(*prm)
    path = fq_file.encode() if isinstance(fq_file, str) else fq_file
    L = _lib.lib()
    rc = L.kmhg_sh1_count_fastq(C.byref(h), path, arr)
    if rc == _lib.KMHG_EINVAL:
        raise KmerHashError(L.kmhg_last_error().decode())
    _lib.check(rc)
    if hash_ptr is not None:
        return hash_ptr
    return ExtPtr(h.value, tag=SUFFIX_HASH_TAG)


def kmer_spec_sh(ptr, max_count) -> np.ndarray:
    """kmer.spec.sh -> .Call("kmer_spectrum_suffix_hash", ptr, max.count)
    (src/kmer_hash.c:993-1008, sh_count_spectrum src/suffix_hash.c:112-129).

    Returns max_count + 1 float64: entry min(count, max_count) gains one per distinct k-mer."""
    if not (isinstance(ptr, ExtPtr) and ptr.tag == SUFFIX_HASH_TAG and ptr._h):
        raise KmerHashError("unable to obtain a suffix_hash from external pointer")
    mc = _int_vec(max_count, 1, "max_count_r should be a single integer")[0]
    if mc < 1 or mc > (1 << 30):
        raise KmerHashError("Unsuitable value of max_count")
    out = np.zeros(mc + 1, np.float64)
    L = _lib.lib()
    rc = L.kmhg_sh1_spectrum(ptr.handle, mc, out.ctypes.data)
    if rc == _lib.KMHG_EINVAL:
        raise KmerHashError(L.kmhg_last_error().decode())
    _lib.check(rc)
    return out


def counts_table(ptr):
    """(keys, counts) rows of a counts pointer or suffix hash (tests and inspection)."""
    if not isinstance(ptr, ExtPtr):
        raise KmerHashError("ptr_r should be an external pointer")
    inf = ptr.info()
    keys = np.zeros(max(inf.n_kmers, 1), np.uint64)
    M = np.zeros(max(inf.n_kmers * inf.sources, 1), np.int32)
    _lib.check(_lib.lib().kmhg_counts_export(ptr.handle, keys.ctypes.data, M.ctypes.data))
    return keys[:inf.n_kmers], M[:inf.n_kmers * inf.sources].reshape(inf.n_kmers, inf.sources)
