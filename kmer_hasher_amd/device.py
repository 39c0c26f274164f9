"""Device-resident entry points (inputs already in HBM as torch uint8 tensors).

These drive the same C-ABI as ``api`` (kmhg_*_device variants) on the caller's current torch
stream, so bench.py can time the hot path with inputs resident in HBM and the multi-GPU layer
(``dist``) can move index images and hit rows with RCCL.  torch is plumbing here (device memory,
streams, torch.distributed); every result is computed by the HIP kernels in libkmhgpu.so.
"""
from __future__ import annotations

import ctypes as C
import json

import torch

from . import _lib


def _stream_ptr(stream=None):
    s = stream if stream is not None else torch.cuda.current_stream()
    return C.c_void_p(s.cuda_stream)


def _check_seq(t: torch.Tensor):
    if not (t.is_cuda and t.dtype == torch.uint8 and t.dim() == 1 and t.is_contiguous()):
        raise TypeError("sequence must be a contiguous 1-D torch.uint8 CUDA tensor")


class DeviceIndex:
    def __init__(self, handle: int):
        self._h = C.c_void_p(handle)

    @classmethod
    def build(cls, seq: torch.Tensor, k: int, stream=None, w: int = 1) -> "DeviceIndex":
        """w > 1: an index of the (w,k)-minimizer windows alone (kmhg_build_sampled_device);
        w = 1 calls kmhg_build_device as ever."""
        _check_seq(seq)
        with torch.cuda.device(seq.device):
            out = C.c_void_p()
            if w == 1:
                _lib.check(_lib.lib().kmhg_build_device(C.c_void_p(seq.data_ptr()), seq.numel(),
                                                        k, 0, _stream_ptr(stream), C.byref(out)))
            else:
                _lib.check(_lib.lib().kmhg_build_sampled_device(
                    C.c_void_p(seq.data_ptr()), seq.numel(), k, int(w), 0, _stream_ptr(stream),
                    C.byref(out)))
        return cls(out.value)

    @property
    def sampling(self) -> int:
        """The minimizer w the index was built with (kmhg_get_sampling); 1: every window."""
        w = C.c_int()
        _lib.check(_lib.lib().kmhg_get_sampling(self._h, C.byref(w)))
        return w.value

    @staticmethod
    def minimizer_mask(seq: torch.Tensor, k: int, w: int, rc: bool = False, stream=None):
        """The (w,k)-minimizer selection of an HBM-resident sequence
        (kmhg_minimizer_mask_device): (mask words, number selected); bit (s - 1) % 32 of int32
        word (s - 1) // 32 is window start s, of rc(seq) with rc."""
        _check_seq(seq)
        nw = max(seq.numel() - k + 1, 1)
        words = torch.empty(((nw + 31) // 32,), dtype=torch.int32, device=seq.device)
        n = C.c_int64()
        with torch.cuda.device(seq.device):
            _lib.check(_lib.lib().kmhg_minimizer_mask_device(
                C.c_void_p(seq.data_ptr()), seq.numel(), k, int(w), 1 if rc else 0,
                C.c_void_p(words.data_ptr()), _stream_ptr(stream), C.byref(n)))
        return words, n.value

    @classmethod
    def build_part(cls, seq: torch.Tensor, k: int, part: int, n_parts: int,
                   stream=None) -> "DevicePart":
        """Part `part` of `n_parts` of an owner-computes build (kmhg_build_device_part): the
        k-mers whose hash bucket lies in this part's range of the whole table, from every
        window of `seq`."""
        _check_seq(seq)
        with torch.cuda.device(seq.device):
            out = C.c_void_p()
            _lib.check(_lib.lib().kmhg_build_device_part(C.c_void_p(seq.data_ptr()), seq.numel(),
                                                         k, part, n_parts, _stream_ptr(stream),
                                                         C.byref(out)))
        p = DevicePart(out.value)
        p.k, p.L, p.device = k, seq.numel(), seq.device
        return p

    @classmethod
    def count(cls, seq: torch.Tensor, k: int, source: int, source_n: int,
              into: "DeviceIndex | None" = None, stream=None) -> "DeviceIndex":
        """count.kmers of one HBM-resident sequence (kmhg_count_device): adds to `into`, or
        makes a new counts index.  Synchronous (the merge reads the number of new k-mers)."""
        _check_seq(seq)
        h = C.c_void_p(into._h.value if into is not None else None)
        with torch.cuda.device(seq.device):
            _lib.check(_lib.lib().kmhg_count_device(C.byref(h), C.c_void_p(seq.data_ptr()),
                                                    seq.numel(), k, source, source_n,
                                                    _stream_ptr(stream)))
        return into if into is not None else cls(h.value)

    @classmethod
    def count_reads(cls, reads: "DeviceReads", params, into: "DeviceIndex | None" = None,
                    stream=None) -> "DeviceIndex":
        """count.kmers.fq.sh.rp over HBM-resident packed reads (kmhg_sh_count_reads_device):
        params = (k, prefix_bits, min_q, thread_n, max_reads, max_mem, source_n, source)."""
        h = C.c_void_p(into._h.value if into is not None else None)
        prm = (C.c_int32 * 8)(*[int(x) for x in params])
        with torch.cuda.device(reads.seq.device):
            _lib.check(_lib.lib().kmhg_sh_count_reads_device(
                C.byref(h), C.c_void_p(reads.seq.data_ptr()), C.c_void_p(reads.qual.data_ptr()),
                C.c_void_p(reads.off.data_ptr()), C.c_void_p(reads.hasq.data_ptr()), reads.n,
                prm, _stream_ptr(stream)))
        return into if into is not None else cls(h.value)

    def depth(self, seq: torch.Tensor, k: int, out: torch.Tensor | None = None,
              stream=None) -> torch.Tensor:
        """seq.kmer.depth.sh of an HBM-resident sequence: (L, counts_n) int32 (INT_MIN = NA)."""
        _check_seq(seq)
        S = self.info()["sources"]
        if out is None:
            out = torch.empty((seq.numel(), S), dtype=torch.int32, device=seq.device)
        if out.dtype != torch.int32 or not out.is_contiguous() or out.numel() < seq.numel() * S:
            raise ValueError(f"out must be a contiguous int32 tensor of >= {seq.numel() * S} "
                             "elements (L x counts_n)")
        with torch.cuda.device(seq.device):
            _lib.check(_lib.lib().kmhg_sh_depth_device(self._h, C.c_void_p(seq.data_ptr()),
                                                       seq.numel(), k, C.c_void_p(out.data_ptr()),
                                                       _stream_ptr(stream)))
        return out

    @property
    def handle(self):
        return self._h

    def wait(self) -> "DeviceIndex":
        """Block until the (asynchronous) build has finished; info/queries/readout also wait."""
        _lib.check(_lib.lib().kmhg_index_wait(self._h))
        return self

    def info(self) -> dict:
        inf = _lib.Info()
        _lib.check(_lib.lib().kmhg_index_info(self._h, C.byref(inf)))
        return {f: getattr(inf, f) for f, _ in _lib.Info._fields_}

    def set_max_occ(self, n: int = 0) -> "DeviceIndex":
        """The occurrence cap of later queries on this position index (kmhg_set_max_occ): 0 is
        off; with n >= 1 a query window whose k-mer occurs at more than n positions of the index
        yields no hit, in query*, segments, blocks, chains and raster alike."""
        _lib.check(_lib.lib().kmhg_set_max_occ(self._h, int(n)))
        return self

    @property
    def max_occ(self) -> int:
        n = C.c_int64()
        _lib.check(_lib.lib().kmhg_get_max_occ(self._h, C.byref(n)))
        return n.value

    def query(self, seq: torch.Tensor, k: int, stream=None) -> "DeviceQuery":
        _check_seq(seq)
        q = C.c_void_p()
        h = C.c_int64()
        with torch.cuda.device(seq.device):
            _lib.check(_lib.lib().kmhg_query_run_device(self._h, C.c_void_p(seq.data_ptr()),
                                                        seq.numel(), k, _stream_ptr(stream),
                                                        C.byref(q), C.byref(h)))
        return DeviceQuery(q.value, h.value, seq.device)

    def query_reads(self, reads, k: int, strands: int = 3, stream=None) -> "DeviceReadsQuery":
        """reads.kmer.pos on the device (kmhg_reads_query_run_device): every read of a packed
        batch against this position index, strands 1 forward, 2 reverse, 3 both.  `reads` is a
        DeviceReads, or a (seq, off) pair of CUDA tensors: seq uint8 with the bases of all reads
        and nothing else, off int64[n + 1] non-decreasing from 0 to seq.numel() (checked on the
        device: KMHG_EINVAL).  Rows (read, strand, i, j) as include/kmhgpu.h defines them."""
        if isinstance(reads, DeviceReads):
            seq, off, n_bases = reads.seq, reads.off, reads.n_bases
        else:
            seq, off = reads
            n_bases = seq.numel()
        _check_seq(seq)
        if not (off.is_cuda and off.dtype == torch.int64 and off.dim() == 1 and
                off.is_contiguous() and off.numel() >= 1 and off.device == seq.device):
            raise TypeError("offsets must be a contiguous 1-D torch.int64 CUDA tensor of n + 1 "
                            "entries on the bases' device")
        n_reads = off.numel() - 1
        q = C.c_void_p()
        h = C.c_int64()
        with torch.cuda.device(seq.device):
            _lib.check(_lib.lib().kmhg_reads_query_run_device(
                self._h, C.c_void_p(seq.data_ptr()), n_bases, C.c_void_p(off.data_ptr()), n_reads,
                k, strands, _stream_ptr(stream), C.byref(q), C.byref(h)))
        return DeviceReadsQuery(q.value, h.value, n_reads, k, seq.device)

    def query_range(self, seq: torch.Tensor, k: int, w0: int, w1: int, stream=None) -> "DeviceQuery":
        """Windows [w0, w1) of `seq` (the multi-GPU shard unit, see dist.py)."""
        _check_seq(seq)
        q = C.c_void_p()
        h = C.c_int64()
        with torch.cuda.device(seq.device):
            _lib.check(_lib.lib().kmhg_query_run_device_range(
                self._h, C.c_void_p(seq.data_ptr()), seq.numel(), k, w0, w1, _stream_ptr(stream),
                C.byref(q), C.byref(h)))
        return DeviceQuery(q.value, h.value, seq.device)

    def query_range_runs(self, seq: torch.Tensor, k: int, w0: int, w1: int, stream=None):
        """Windows [w0, w1) with the rows left as diagonal runs
        (kmhg_query_run_device_range_runs): ('runs', (n_runs, 3) int32 tensor, H), or
        ('rows', (H, 2) int32 tensor, H) where runs would not be smaller.  Either tensor owns
        the query."""
        _check_seq(seq)
        q = C.c_void_p()
        h, nr = C.c_int64(), C.c_int64()
        with torch.cuda.device(seq.device):
            _lib.check(_lib.lib().kmhg_query_run_device_range_runs(
                self._h, C.c_void_p(seq.data_ptr()), seq.numel(), k, w0, w1, _stream_ptr(stream),
                C.byref(q), C.byref(h), C.byref(nr)))
        dq = DeviceQuery(q.value, h.value, seq.device)
        if nr.value < 0:
            return "rows", dq.rows_view(), h.value
        return "runs", dq.runs_view(nr.value), h.value

    # The reverse strand: `seq` is the FORWARD sequence; the rows are those of query(rc(seq))
    # -- i the 1-based window end in rc(seq), whose window starts at forward position
    # seq.numel() - i + 1 -- and w0, w1 are window starts in rc(seq).  N stays N
    # (include/kmhgpu.h, kmhg_query_run_rc).  No reversed copy of the sequence is made.
    def query_rc(self, seq: torch.Tensor, k: int, stream=None) -> "DeviceQuery":
        return self.query_range_rc(seq, k, 0, max(seq.numel() - k + 1, 0), stream)

    def query_range_rc(self, seq: torch.Tensor, k: int, w0: int, w1: int,
                       stream=None) -> "DeviceQuery":
        _check_seq(seq)
        q = C.c_void_p()
        h = C.c_int64()
        with torch.cuda.device(seq.device):
            _lib.check(_lib.lib().kmhg_query_run_rc_device_range(
                self._h, C.c_void_p(seq.data_ptr()), seq.numel(), k, w0, w1, _stream_ptr(stream),
                C.byref(q), C.byref(h)))
        return DeviceQuery(q.value, h.value, seq.device)

    def query_range_runs_rc(self, seq: torch.Tensor, k: int, w0: int, w1: int, stream=None):
        """query_range_runs on the reverse strand: ('runs', ...) or ('rows', ...)."""
        _check_seq(seq)
        q = C.c_void_p()
        h, nr = C.c_int64(), C.c_int64()
        with torch.cuda.device(seq.device):
            _lib.check(_lib.lib().kmhg_query_run_rc_device_range_runs(
                self._h, C.c_void_p(seq.data_ptr()), seq.numel(), k, w0, w1, _stream_ptr(stream),
                C.byref(q), C.byref(h), C.byref(nr)))
        dq = DeviceQuery(q.value, h.value, seq.device)
        if nr.value < 0:
            return "rows", dq.rows_view(), h.value
        return "runs", dq.runs_view(nr.value), h.value

    def raster(self, seq: torch.Tensor, k: int, frame, rc: bool = False,
               out: torch.Tensor | None = None, stream=None) -> tuple[torch.Tensor, int]:
        """kmhg_raster_run_device (seq.kmer.raster, the row-free route): the rows of query(seq, k)
        -- of query_rc(seq, k) with rc -- binned into the frame (i_lo, j_lo, bin_i, bin_j, n_i,
        n_j) without ever being written: (int64 (n_i, n_j) counts, n_rows), n_rows the hit total,
        which may exceed 2^31 - 1 where query() refuses.  Equal to rows_raster of the query's
        rows wherever those exist.  Synchronous."""
        _check_seq(seq)
        fr, f, out = _raster_args(frame, out, seq.device)
        h = C.c_int64()
        with torch.cuda.device(seq.device):
            _lib.check(_lib.lib().kmhg_raster_run_device(
                self._h, C.c_void_p(seq.data_ptr()), seq.numel(), k, 1 if rc else 0, fr,
                C.c_void_p(out.data_ptr()), _stream_ptr(stream), C.byref(h)))
        return _raster_matrix(out, f), h.value

    def segments(self, seq: torch.Tensor, k: int, min_len: int = 1, rc: bool = False,
                 stream=None) -> tuple[torch.Tensor, int]:
        """kmhg_segments_run_device (seq.kmer.segs, the row-free route): the maximal diagonal
        segments of query(seq, k) -- of query_rc(seq, k) with rc -- found from the per-window
        records without the rows ever being written: ((S, 3) int32 {i, j, len}, n_rows), n_rows
        the hit total, which may exceed 2^31 - 1 where DeviceQuery.segments refuses.  Equal to
        query(seq, k).segments(min_len), byte for byte, wherever that exists.  Synchronous."""
        _check_seq(seq)
        g = C.c_void_p()
        n, h = C.c_int64(), C.c_int64()
        with torch.cuda.device(seq.device):
            _lib.check(_lib.lib().kmhg_segments_run_device(
                self._h, C.c_void_p(seq.data_ptr()), seq.numel(), k, 1 if rc else 0, int(min_len),
                _stream_ptr(stream), C.byref(g), C.byref(n), C.byref(h)))
        return _segs_tensor(g, n.value, seq.device), h.value

    def blocks(self, seq: torch.Tensor, k: int, max_gap: int, min_len: int = 1, min_hits: int = 1,
               rc: bool = False, stream=None) -> tuple[torch.Tensor, int]:
        """kmhg_blocks_run_device (seq.kmer.blocks, the row-free route): segments()'s front half
        followed by the block passes: ((B, 4) int32 {i, j, span, hits}, n_rows).  Equal to
        query(seq, k).blocks(max_gap, min_len, min_hits), byte for byte, wherever that exists.
        Synchronous."""
        _check_seq(seq)
        g = C.c_void_p()
        n, h = C.c_int64(), C.c_int64()
        with torch.cuda.device(seq.device):
            _lib.check(_lib.lib().kmhg_blocks_run_device(
                self._h, C.c_void_p(seq.data_ptr()), seq.numel(), k, 1 if rc else 0, int(min_len),
                int(max_gap), int(min_hits), _stream_ptr(stream), C.byref(g), C.byref(n),
                C.byref(h)))
        return _blocks_tensor(g, n.value, seq.device), h.value

    def chains(self, seq: torch.Tensor, k: int, max_dist: int = 5000, max_drift: int = 500,
               max_gap: int | None = None, min_len: int = 1, min_hits: int = 1, rc: bool = False,
               row_free: bool = False, stream=None):
        """kmhg_chains_run_device (seq.kmer.chains): the blocks of query(seq, k).blocks(max_gap,
        min_len) -- of blocks(seq, k, max_gap, min_len) with row_free -- chained by blocks_chains:
        ((C, 6) int32 chains, (B, 4) int32 blocks, (B,) int32 chain[b], n_rows).  max_gap=None
        means k; min_hits applies to the chains.  Synchronous."""
        _check_seq(seq)
        g = C.c_void_p()
        nc, nb, h = C.c_int64(), C.c_int64(), C.c_int64()
        with torch.cuda.device(seq.device):
            _lib.check(_lib.lib().kmhg_chains_run_device(
                self._h, C.c_void_p(seq.data_ptr()), seq.numel(), k, 1 if rc else 0,
                1 if row_free else 0, int(min_len), int(k if max_gap is None else max_gap),
                int(max_dist), int(max_drift), int(min_hits), _stream_ptr(stream), C.byref(g),
                C.byref(nc), C.byref(nb), C.byref(h)))
        return _chains_tensors(g, nc.value, nb.value, seq.device, True, stream) + (h.value,)

    def positions(self, opt: int, stream=None) -> dict:
        """kmer.pos into device tensors: {'kmer': uint8 (U, k+1), 'pos': int32 (N, 2),
        'pair.pos': int32 (P, 3), 'count': int32 (U,)} for the requested bits."""
        L = _lib.lib()
        nk, npos, npair, ncnt = C.c_int64(), C.c_int64(), C.c_int64(), C.c_int64()
        _lib.check(L.kmhg_positions_size(self._h, opt, C.byref(nk), C.byref(npos),
                                         C.byref(npair), C.byref(ncnt)))
        inf = self.info()
        dev = torch.device("cuda", inf["device"])
        out = {"kmer": None, "pos": None, "pair.pos": None, "count": None}
        if opt & 1:
            out["kmer"] = torch.empty((nk.value, inf["k"] + 1), dtype=torch.uint8, device=dev)
        if opt & 2:
            out["pos"] = torch.empty((npos.value, 2), dtype=torch.int32, device=dev)
        if opt & 4:
            out["pair.pos"] = torch.empty((npair.value, 3), dtype=torch.int32, device=dev)
        if opt & 8:
            out["count"] = torch.empty((ncnt.value,), dtype=torch.int32, device=dev)

        def p(t):
            return C.c_void_p(t.data_ptr()) if t is not None and t.numel() else None

        with torch.cuda.device(dev):
            _lib.check(L.kmhg_positions_fill_device(self._h, opt, p(out["kmer"]), p(out["pos"]),
                                                    p(out["pair.pos"]), p(out["count"]),
                                                    _stream_ptr(stream)))
        return out

    # ---- index image (multi-GPU replication) ---------------------------------------------
    def export_image(self, stream=None) -> tuple[torch.Tensor, list[torch.Tensor]]:
        sz = _lib.ImageSizes()
        hdr = (C.c_int64 * 8)()
        _lib.check(_lib.lib().kmhg_image_sizes_get(self._h, C.byref(sz), hdr))
        dev = torch.device("cuda", self.info()["device"])
        bufs = [torch.empty(max(1, getattr(sz, f)), dtype=torch.uint8, device=dev)
                for f, _ in _lib.ImageSizes._fields_]
        with torch.cuda.device(dev):
            _lib.check(_lib.lib().kmhg_image_export(self._h,
                                                    *[C.c_void_p(b.data_ptr()) for b in bufs],
                                                    _stream_ptr(stream)))
        header = torch.tensor(list(hdr), dtype=torch.int64)
        sizes = torch.tensor([getattr(sz, f) for f, _ in _lib.ImageSizes._fields_],
                             dtype=torch.int64)
        return torch.cat([header, sizes]), bufs

    @classmethod
    def import_image(cls, meta: torch.Tensor, bufs: list[torch.Tensor], stream=None):
        hdr = (C.c_int64 * 8)(*[int(x) for x in meta[:8].tolist()])
        sizes = [int(x) for x in meta[8:].tolist()]
        out = C.c_void_p()
        # a buffer of size 0 (no positions, no code block) is passed as NULL
        ptrs = [C.c_void_p(b.data_ptr() if i >= len(sizes) or sizes[i] else None)
                for i, b in enumerate(bufs)]
        with torch.cuda.device(bufs[0].device):
            _lib.check(_lib.lib().kmhg_image_import(hdr, *ptrs, _stream_ptr(stream), C.byref(out)))
        return cls(out.value)

    def free(self):
        if self._h:
            _lib.lib().kmhg_free(self._h)
            self._h = C.c_void_p(0)

    def __del__(self):
        try:
            self.free()
        except Exception:
            pass


PART_FIELDS = ("b0", "nb", "nb_total", "capb", "n_positions", "n_kmers", "n_pairs", "max_count",
               "side_owner", "codes_bytes")
SLOT_BYTES = 16


class DevicePart(DeviceIndex):
    """One part of an owner-computes build (DeviceIndex.build_part); dist.assemble_parts turns
    the parts of all ranks into the whole index."""

    def part_info(self) -> dict:
        a = (C.c_int64 * 10)()
        _lib.check(_lib.lib().kmhg_part_info(self._h, a))
        return dict(zip(PART_FIELDS, list(a)))

    def export_into(self, pos_base: int, table: torch.Tensor | None, side: torch.Tensor | None,
                    positions: torch.Tensor | None, codes: torch.Tensor | None, stream=None):
        """Write this part's rebased slots / side slot / positions / code block into the given
        uint8 device views (None = skip)."""
        def p(t):
            return C.c_void_p(t.data_ptr()) if t is not None and t.numel() else None
        with torch.cuda.device(self.device):
            _lib.check(_lib.lib().kmhg_part_export(self._h, pos_base, p(table), p(side),
                                                   p(positions), p(codes), _stream_ptr(stream)))


    def query_part(self, seq: torch.Tensor, k: int, stream=None) -> "DeviceQuery":
        """seq.kmer.pos of every window of `seq` against this part only
        (kmhg_query_run_device_part): the rows of the windows whose k-mer the part owns, in
        window order; merge_part_rows interleaves every part's rows."""
        _check_seq(seq)
        q = C.c_void_p()
        h = C.c_int64()
        with torch.cuda.device(seq.device):
            _lib.check(_lib.lib().kmhg_query_run_device_part(
                self._h, C.c_void_p(seq.data_ptr()), seq.numel(), k, _stream_ptr(stream),
                C.byref(q), C.byref(h)))
        return DeviceQuery(q.value, h.value, seq.device)

    # ---- kmer.pos over resident parts (no assembly) --------------------------------------
    def first_mask(self, stream=None) -> torch.Tensor:
        """kmhg_part_first_mask: ceil(L / 32) int32 words, one bit per first position of the
        k-mers this part holds.  The parts' masks are disjoint: their sum is their union."""
        mask = torch.empty((self.L + 31) // 32, dtype=torch.int32, device=self.device)
        with torch.cuda.device(self.device):
            _lib.check(_lib.lib().kmhg_part_first_mask(self._h, C.c_void_p(mask.data_ptr()),
                                                       _stream_ptr(stream)))
        return mask

    def positions_part(self, mask: torch.Tensor, opt: int, stream=None) -> dict:
        """kmhg_part_positions_fill_device: this part's kmer.pos rows labelled with their rows in
        the whole index, given the union `mask` of every part's first_mask.  {'labels': int32
        (U_part,), and for the requested bits 'kmer', 'pos', 'pair.pos', 'count' as
        DeviceIndex.positions}, all in ascending label."""
        if mask.dtype != torch.int32 or mask.numel() != (self.L + 31) // 32 or \
                mask.device != self.device or not mask.is_contiguous():
            raise ValueError("mask must be the contiguous int32 words of first_mask()")
        L = _lib.lib()
        nk, npos, npair = C.c_int64(), C.c_int64(), C.c_int64()
        _lib.check(L.kmhg_part_positions_size(self._h, opt, C.byref(nk), C.byref(npos),
                                              C.byref(npair)))
        dev = self.device
        out = {"labels": torch.empty((nk.value,), dtype=torch.int32, device=dev),
               "kmer": None, "pos": None, "pair.pos": None, "count": None}
        if opt & 1:
            out["kmer"] = torch.empty((nk.value, self.k + 1), dtype=torch.uint8, device=dev)
        if opt & 2:
            out["pos"] = torch.empty((npos.value, 2), dtype=torch.int32, device=dev)
        if opt & 4:
            out["pair.pos"] = torch.empty((npair.value, 3), dtype=torch.int32, device=dev)
        if opt & 8:
            out["count"] = torch.empty((nk.value,), dtype=torch.int32, device=dev)
        with torch.cuda.device(dev):
            _lib.check(L.kmhg_part_positions_fill_device(
                self._h, C.c_void_p(mask.data_ptr()), opt, _dptr(out["labels"]),
                _dptr(out["kmer"]), _dptr(out["pos"]), _dptr(out["pair.pos"]),
                _dptr(out["count"]), _stream_ptr(stream)))
        return out


def _dptr(t):
    """A tensor's device pointer, NULL for None or an empty tensor."""
    return C.c_void_p(t.data_ptr()) if t is not None and t.numel() else None


def merge_part_positions(segs: list[dict], opt: int, k: int, stream=None) -> dict:
    """kmhg_merge_part_positions: every part's positions_part() dict (on one device; each with
    'count' whenever opt has bit 2, 4 or 8) into the dict DeviceIndex.positions(opt) of the whole
    index returns: counts and strings placed by label, each k-mer's rows at its offset."""
    if (opt & 14) and any(s.get("count") is None for s in segs):
        raise ValueError("merging pos / pair.pos / count needs every part's 'count'")
    dev = segs[0]["labels"].device
    n = len(segs)
    nk = [int(s["labels"].numel()) for s in segs]
    npos = [int(s["pos"].shape[0]) if opt & 2 else 0 for s in segs]
    npair = [int(s["pair.pos"].shape[0]) if opt & 4 else 0 for s in segs]
    U, N, P = sum(nk), sum(npos), sum(npair)
    out = {"kmer": None, "pos": None, "pair.pos": None, "count": None}
    if opt & 1:
        out["kmer"] = torch.empty((U, k + 1), dtype=torch.uint8, device=dev)
    if opt & 2:
        out["pos"] = torch.empty((N, 2), dtype=torch.int32, device=dev)
    if opt & 4:
        out["pair.pos"] = torch.empty((P, 3), dtype=torch.int32, device=dev)
    if opt & 8:
        out["count"] = torch.empty((U,), dtype=torch.int32, device=dev)
    keep = [s[f].contiguous() if s.get(f) is not None else None
            for f in ("labels", "count", "kmer", "pos", "pair.pos") for s in segs]

    def ptrs(j):
        return (C.c_void_p * n)(*[t.data_ptr() if t is not None and t.numel() else None
                                  for t in keep[j * n:(j + 1) * n]])

    i64 = lambda v: (C.c_int64 * n)(*v)  # noqa: E731
    with torch.cuda.device(dev):
        _lib.check(_lib.lib().kmhg_merge_part_positions(
            n, opt, k, i64(nk), i64(npos), i64(npair), ptrs(0), ptrs(1), ptrs(2), ptrs(3),
            ptrs(4), _dptr(out["kmer"]), _dptr(out["pos"]), _dptr(out["pair.pos"]),
            _dptr(out["count"]), _stream_ptr(stream)))
    return out


def merge_part_rows(rows: torch.Tensor, seg_base: list[int], tile_off: torch.Tensor, k: int,
                    w0: int = 0, stream=None) -> torch.Tensor:
    """kmhg_merge_part_rows: `rows` (H, 2) int32 holds every part's rows (part r's from row
    seg_base[r]), `tile_off` (n_parts, n_tiles + 1) uint64 their per-tile offsets; returns the
    (H, 2) rows in the unsharded seq.kmer.pos order."""
    dev = rows.device
    n_parts, nt1 = tile_off.shape
    out = torch.empty_like(rows)
    base = torch.tensor(seg_base, dtype=torch.int64, device=dev)
    toff = tile_off.to(device=dev, dtype=torch.int64).contiguous()
    with torch.cuda.device(dev):
        _lib.check(_lib.lib().kmhg_merge_part_rows(
            C.c_void_p(rows.data_ptr()), C.c_void_p(base.data_ptr()),
            C.c_void_p(toff.data_ptr()), n_parts, nt1 - 1, k, w0, C.c_void_p(out.data_ptr()),
            _stream_ptr(stream)))
    return out


def seq_pack(seq: torch.Tensor, stream=None) -> tuple[torch.Tensor, torch.Tensor]:
    """kmhg_seq_pack: a uint8 device sequence as (code u32 words, N-flag u16 words), 16 chars
    each -- what crosses xGMI in place of the chars (6 B per 16)."""
    _check_seq(seq)
    words = (seq.numel() + 15) // 16
    code = torch.empty(max(1, words), dtype=torch.int32, device=seq.device)
    nbit = torch.empty(max(1, words), dtype=torch.int16, device=seq.device)
    with torch.cuda.device(seq.device):
        _lib.check(_lib.lib().kmhg_seq_pack(
            C.c_void_p(seq.data_ptr()), seq.numel(), C.c_void_p(code.data_ptr()),
            C.c_void_p(nbit.data_ptr()), _stream_ptr(stream)))
    return code[:words], nbit[:words]


def seq_unpack(code: torch.Tensor, nbit: torch.Tensor, word0: int, a: int, b: int,
               out: torch.Tensor, stream=None) -> torch.Tensor:
    """kmhg_seq_unpack: chars [a, b) of `out` (uint8, device) from words held from word0 on."""
    if b <= a:
        return out
    if out.numel() < b or out.dtype != torch.uint8 or not out.is_cuda:
        raise ValueError("out must be a uint8 CUDA tensor of at least b chars")
    if code.numel() < (b + 15) // 16 - word0 or nbit.numel() < (b + 15) // 16 - word0:
        raise ValueError("the packed words do not cover [a, b)")
    with torch.cuda.device(out.device):
        _lib.check(_lib.lib().kmhg_seq_unpack(
            C.c_void_p(code.data_ptr()), C.c_void_p(nbit.data_ptr()), word0, a, b,
            C.c_void_p(out.data_ptr()), _stream_ptr(stream)))
    return out


def rows_to_host(rows: torch.Tensor, out: torch.Tensor, stream=None) -> torch.Tensor:
    """kmhg_rows_to_host: (H, 2) int32 device rows into `out`, a contiguous host (H, 2) int32
    tensor (pinned or not), as kmhg_query_fill delivers a query: diagonal runs over PCIe,
    expanded by host threads.  Synchronous."""
    H = rows.shape[0]
    if out.shape != (H, 2) or out.dtype != torch.int32 or out.is_cuda or not out.is_contiguous():
        raise ValueError("out must be a contiguous host (H, 2) int32 tensor")
    if H == 0:
        return out
    rows = rows.contiguous()
    with torch.cuda.device(rows.device):
        _lib.check(_lib.lib().kmhg_rows_to_host(C.c_void_p(rows.data_ptr()), H,
                                                C.c_void_p(out.data_ptr()), _stream_ptr(stream)))
    return out


def rows_to_runs(rows: torch.Tensor, stream=None) -> torch.Tensor | None:
    """kmhg_rows_runs: the (H, 2) int32 rows as diagonal runs, an (n_runs, 3) int32 tensor of
    {first row index, i, j} -- or None when runs would not be smaller than the rows (12 B per
    run against 8 B per row)."""
    H = rows.shape[0]
    if H == 0:
        return None
    dev = rows.device
    rows = rows.contiguous()
    n = C.c_int64()
    cap = max(1, H // 16)                    # a dot plot's runs: tens of rows each
    with torch.cuda.device(dev):
        for _ in range(2):
            runs = torch.empty((cap, 3), dtype=torch.int32, device=dev)
            _lib.check(_lib.lib().kmhg_rows_runs(
                C.c_void_p(rows.data_ptr()), H, C.c_void_p(runs.data_ptr()), cap, C.byref(n),
                _stream_ptr(stream)))
            if 3 * n.value >= 2 * H:
                return None
            if n.value <= cap:
                return runs[:n.value]
            cap = n.value
    raise RuntimeError("kmhg_rows_runs: run count changed between calls")


def runs_expand(runs: torch.Tensor, n_rows: int, out: torch.Tensor, stream=None) -> torch.Tensor:
    """kmhg_runs_expand: (n_runs, 3) int32 runs back to their n_rows (i, j) rows in `out` (a
    contiguous (n_rows, 2) int32 device tensor)."""
    if n_rows == 0:
        return out
    if out.shape != (n_rows, 2) or out.dtype != torch.int32 or not out.is_contiguous():
        raise ValueError("out must be a contiguous (n_rows, 2) int32 tensor")
    runs = runs.to(device=out.device, dtype=torch.int32).contiguous()
    with torch.cuda.device(out.device):
        _lib.check(_lib.lib().kmhg_runs_expand(
            C.c_void_p(runs.data_ptr()), runs.shape[0], n_rows, C.c_void_p(out.data_ptr()),
            _stream_ptr(stream)))
    return out


def _handle_tensor(kind: str, h: C.c_void_p, n: int, cols: int, device) -> torch.Tensor:
    """The (n, cols) int32 tensor of a kmhg_segs or kmhg_blocks handle (kind "segs" or "blocks"),
    which it owns (rows_view's contract)."""
    g = _DeviceRecords(kind, h)
    if not n:
        g.free()
        return torch.empty((0, cols), dtype=torch.int32, device=device)
    d = C.c_void_p()
    _lib.check(getattr(_lib.lib(), f"kmhg_{kind}_device")(h, C.byref(d), None))
    return torch.as_tensor(_RowsBuffer(g, d.value, (n, cols)), device=device)


def _segs_tensor(h: C.c_void_p, n: int, device) -> torch.Tensor:
    return _handle_tensor("segs", h, n, 3, device)


def _blocks_tensor(h: C.c_void_p, n: int, device) -> torch.Tensor:
    return _handle_tensor("blocks", h, n, 4, device)


def rows_segments(rows: torch.Tensor, min_len: int = 1, stream=None) -> torch.Tensor:
    """kmhg_rows_segments (seq.kmer.segs): the (H, 2) int32 device rows of a seq.kmer.pos result
    -- i, j >= 1, strictly ascending by (i, j) -- as their maximal diagonal segments, an (S, 3)
    int32 tensor of {i, j, len} ordered by (i, j): (i + t, j + t) is a row for 0 <= t < len and
    neither (i - 1, j - 1) nor (i + len, j + len) is.  min_len keeps the segments of at least
    that many rows.  Decided from the rows alone (include/kmhgpu.h).  Synchronous."""
    if not (rows.is_cuda and rows.dtype == torch.int32 and rows.dim() == 2 and rows.shape[1] == 2):
        raise TypeError("rows must be an (H, 2) torch.int32 CUDA tensor")
    rows = rows.contiguous()
    g = C.c_void_p()
    n = C.c_int64()
    with torch.cuda.device(rows.device):
        _lib.check(_lib.lib().kmhg_rows_segments(
            C.c_void_p(rows.data_ptr() if rows.shape[0] else None), rows.shape[0], int(min_len),
            _stream_ptr(stream), C.byref(g), C.byref(n)))
    return _segs_tensor(g, n.value, rows.device)


def rows_blocks(rows: torch.Tensor, max_gap: int, min_len: int = 1, min_hits: int = 1,
                stream=None) -> torch.Tensor:
    """kmhg_rows_blocks (seq.kmer.blocks): the segments rows_segments(rows, min_len) gives, merged
    on every diagonal across gaps of at most max_gap windows, as a (B, 4) int32 tensor of
    {i, j, span, hits} ordered by (i, j): span = the windows from the block's first row to its
    last, hits = its rows.  min_hits keeps the blocks of at least that many rows
    (include/kmhgpu.h).  Synchronous."""
    if not (rows.is_cuda and rows.dtype == torch.int32 and rows.dim() == 2 and rows.shape[1] == 2):
        raise TypeError("rows must be an (H, 2) torch.int32 CUDA tensor")
    rows = rows.contiguous()
    g = C.c_void_p()
    n = C.c_int64()
    with torch.cuda.device(rows.device):
        _lib.check(_lib.lib().kmhg_rows_blocks(
            C.c_void_p(rows.data_ptr() if rows.shape[0] else None), rows.shape[0], int(min_len),
            int(max_gap), int(min_hits), _stream_ptr(stream), C.byref(g), C.byref(n)))
    return _blocks_tensor(g, n.value, rows.device)


def _chains_tensors(h: C.c_void_p, n_chains: int, n_blocks: int, device, with_blocks: bool,
                    stream=None):
    """The tensors of a kmhg_chains handle, copied out of it on `stream`; the handle is freed.
    ((C, 6) int32 chains, (B,) int32 chain[b]) and, with_blocks, the (B, 4) int32 blocks."""
    L = _lib.lib()
    try:
        chains = torch.empty((n_chains, 6), dtype=torch.int32, device=device)
        member = torch.empty((n_blocks,), dtype=torch.int32, device=device)
        blocks = torch.empty((n_blocks, 4), dtype=torch.int32, device=device) if with_blocks \
            else None
        if n_blocks:
            with torch.cuda.device(device):
                _lib.check(L.kmhg_chains_copy_device(
                    h, C.c_void_p(chains.data_ptr() if n_chains else None),
                    C.c_void_p(member.data_ptr()),
                    C.c_void_p(blocks.data_ptr()) if with_blocks else None, _stream_ptr(stream)))
    finally:
        L.kmhg_chains_free(h)             # (waits for the stream the chains were made on)
    return (chains, blocks, member) if with_blocks else (chains, member)


def blocks_chains(blocks: torch.Tensor, max_dist: int, max_drift: int, min_hits: int = 1,
                  stream=None) -> tuple[torch.Tensor, torch.Tensor]:
    """kmhg_blocks_chains (seq.kmer.chains): the (B, 4) int32 device blocks {i, j, span, hits} of
    rows_blocks -- strictly ascending by (i, j) -- linked across diagonals: block a may precede
    block b when b starts after a's last row in both coordinates, the larger gap is at most
    max_dist and the two gaps differ by at most max_drift; every block takes its nearest such
    predecessor, and a link holds where the predecessor's nearest follower is that block
    (include/kmhgpu.h).  Returns (chains, member): (C, 6) int32 {i, j, i.end, j.end, hits, blocks}
    of the chains with hits >= min_hits, ordered by (i, j), and (B,) int32, the 1-based chain of
    every block (0: dropped).  Synchronous."""
    if not (blocks.is_cuda and blocks.dtype == torch.int32 and blocks.dim() == 2 and
            blocks.shape[1] == 4):
        raise TypeError("blocks must be a (B, 4) torch.int32 CUDA tensor")
    blocks = blocks.contiguous()
    if blocks.shape[0] and blocks.data_ptr() % 16:
        blocks = blocks.clone()
    g = C.c_void_p()
    n = C.c_int64()
    with torch.cuda.device(blocks.device):
        _lib.check(_lib.lib().kmhg_blocks_chains(
            C.c_void_p(blocks.data_ptr() if blocks.shape[0] else None), blocks.shape[0],
            int(max_dist), int(max_drift), int(min_hits), _stream_ptr(stream), C.byref(g),
            C.byref(n)))
    return _chains_tensors(g, n.value, blocks.shape[0], blocks.device, False, stream)


def _raster_args(frame, out, device):
    """The int64[6] frame {i_lo, j_lo, bin_i, bin_j, n_i, n_j} and the int32 tensor of n_i * n_j
    elements the library fills with u32 bits (`out`, or a new one).  A frame the library will
    refuse gets a one-element buffer: the refusal comes before anything is written."""
    f = [int(x) for x in frame]
    if len(f) != 6:
        raise ValueError("frame must be (i_lo, j_lo, bin_i, bin_j, n_i, n_j)")
    cells = f[4] * f[5] if 1 <= f[4] and 1 <= f[5] and f[4] * f[5] <= 1 << 26 else 1
    if out is None:
        out = torch.empty(cells, dtype=torch.int32, device=device)
    if not (out.is_cuda and out.dtype == torch.int32 and out.is_contiguous() and
            out.numel() >= cells):
        raise ValueError(f"out must be a contiguous int32 CUDA tensor of >= {cells} elements")
    return (C.c_int64 * 6)(*f), f, out


def _raster_matrix(out: torch.Tensor, f) -> torch.Tensor:
    """The u32 counts as an int64 (n_i, n_j) tensor (cell (bi, bj) at bi + n_i * bj)."""
    n_i, n_j = f[4], f[5]
    return (out[:n_i * n_j].to(torch.int64) & 0xFFFFFFFF).view(n_j, n_i).T


def rows_raster(rows: torch.Tensor, frame, out: torch.Tensor | None = None,
                stream=None) -> torch.Tensor:
    """kmhg_rows_raster (seq.kmer.raster): (H, 2) int32 device rows, in any order, binned into the
    frame (i_lo, j_lo, bin_i, bin_j, n_i, n_j): an int64 (n_i, n_j) tensor whose cell [bi, bj]
    counts the rows with (i - i_lo) // bin_i == bi and (j - j_lo) // bin_j == bj; rows outside
    the frame are not counted (include/kmhgpu.h).  `out`: the int32 tensor of n_i * n_j elements
    the library fills (u32 bits)."""
    if not (rows.is_cuda and rows.dtype == torch.int32 and rows.dim() == 2 and rows.shape[1] == 2):
        raise TypeError("rows must be an (H, 2) torch.int32 CUDA tensor")
    rows = rows.contiguous()
    fr, f, out = _raster_args(frame, out, rows.device)
    with torch.cuda.device(rows.device):
        _lib.check(_lib.lib().kmhg_rows_raster(
            C.c_void_p(rows.data_ptr() if rows.shape[0] else None), rows.shape[0], fr,
            C.c_void_p(out.data_ptr()), _stream_ptr(stream)))
    return _raster_matrix(out, f)


class _DeviceRecords:
    """Owner of a kmhg_segs or kmhg_blocks handle (freed with the last tensor made from it)."""

    def __init__(self, kind: str, h: C.c_void_p):
        self._kind = kind
        self._h = h

    def free(self):
        if self._h:
            getattr(_lib.lib(), f"kmhg_{self._kind}_free")(self._h)
            self._h = C.c_void_p(0)

    def __del__(self):
        try:
            self.free()
        except Exception:
            pass


class DeviceQuery:
    def __init__(self, handle: int, n_rows: int, device: torch.device | None = None):
        self._h = C.c_void_p(handle)
        self.n_rows = n_rows
        # the device the query ran on (the query sequence's): rows_view of an empty result lands
        # there too, like a non-empty one
        self.device = device if device is not None else \
            torch.device("cuda", torch.cuda.current_device())

    def copy_to(self, dst: torch.Tensor, stream=None) -> torch.Tensor:
        """Copy the (H, 2) int32 rows into `dst` (device, >= 2*H int32)."""
        if dst.numel() < 2 * self.n_rows or dst.dtype != torch.int32 or not dst.is_cuda:
            raise ValueError("destination too small or not an int32 CUDA tensor")
        with torch.cuda.device(dst.device):
            _lib.check(_lib.lib().kmhg_query_copy_device(self._h, C.c_void_p(dst.data_ptr()),
                                                         _stream_ptr(stream)))
        return dst

    def rows(self, device=None) -> torch.Tensor:
        dev = device or torch.device("cuda", torch.cuda.current_device())
        t = torch.empty((self.n_rows, 2), dtype=torch.int32, device=dev)
        if self.n_rows:
            self.copy_to(t)
        return t

    def tile_offsets(self, stream=None) -> torch.Tensor:
        """A part query's n_tiles + 1 per-tile row offsets (uint64 as int64, on its device)."""
        n = C.c_int64()
        _lib.check(_lib.lib().kmhg_query_tile_offsets(self._h, None, C.byref(n), None))
        out = torch.empty(n.value + 1, dtype=torch.int64, device=self.device)
        with torch.cuda.device(self.device):
            _lib.check(_lib.lib().kmhg_query_tile_offsets(self._h, C.c_void_p(out.data_ptr()),
                                                          C.byref(n), _stream_ptr(stream)))
        return out

    def rows_view(self) -> torch.Tensor:
        """The (H, 2) int32 rows where the emit kernel wrote them (kmhg_query_rows_device), as a
        tensor that owns this query: no copy, and the rows' buffer goes back to the library's pool
        (stream-ordered on the query's stream) when the last tensor using it is gone.  Used on
        the query's stream, as every result of the library is."""
        if not self.n_rows:
            return torch.empty((0, 2), dtype=torch.int32, device=self.device)
        d = C.c_void_p()
        _lib.check(_lib.lib().kmhg_query_rows_device(self._h, C.byref(d)))
        return torch.as_tensor(_RowsBuffer(self, d.value))   # on the rows' own device

    def segments(self, min_len: int = 1) -> torch.Tensor:
        """kmhg_query_segments: this query's rows as maximal diagonal segments, (S, 3) int32
        {i, j, len} on the query's device (rows_segments of its rows; a KMHG_DEVICES query is
        gathered there first)."""
        g = C.c_void_p()
        n = C.c_int64()
        _lib.check(_lib.lib().kmhg_query_segments(self._h, int(min_len), C.byref(g), C.byref(n)))
        return _segs_tensor(g, n.value, self.device)

    def blocks(self, max_gap: int, min_len: int = 1, min_hits: int = 1) -> torch.Tensor:
        """kmhg_query_blocks: this query's segments merged across gaps of at most max_gap windows,
        (B, 4) int32 {i, j, span, hits} on the query's device (rows_blocks of its rows; a
        KMHG_DEVICES query is gathered there first)."""
        g = C.c_void_p()
        n = C.c_int64()
        _lib.check(_lib.lib().kmhg_query_blocks(self._h, int(min_len), int(max_gap), int(min_hits),
                                                C.byref(g), C.byref(n)))
        return _blocks_tensor(g, n.value, self.device)

    def chains(self, max_dist: int = 5000, max_drift: int = 500, max_gap: int = 0,
               min_len: int = 1, min_hits: int = 1):
        """This query's blocks(max_gap, min_len) chained by blocks_chains(max_dist, max_drift,
        min_hits): ((C, 6) int32 chains, (B, 4) int32 blocks, (B,) int32 chain[b]) on the query's
        device.  (The query does not know its k: max_gap is the caller's, 0 = the segments.)"""
        blocks = self.blocks(max_gap, min_len)
        chains, member = blocks_chains(blocks, max_dist, max_drift, min_hits)
        return chains, blocks, member

    def raster(self, frame, out: torch.Tensor | None = None, stream=None) -> torch.Tensor:
        """kmhg_query_raster: this query's rows binned into `frame`, an int64 (n_i, n_j) tensor on
        the query's device (rows_raster of its rows; a KMHG_DEVICES query is gathered first)."""
        fr, f, out = _raster_args(frame, out, self.device)
        with torch.cuda.device(self.device):
            _lib.check(_lib.lib().kmhg_query_raster(self._h, fr, C.c_void_p(out.data_ptr()),
                                                    _stream_ptr(stream)))
        return _raster_matrix(out, f)

    def runs_view(self, n_runs: int) -> torch.Tensor:
        """The (n_runs, 3) int32 runs of a runs query (kmhg_query_runs_device), as a tensor that
        owns this query (rows_view's contract)."""
        if not n_runs:
            return torch.empty((0, 3), dtype=torch.int32, device=self.device)
        d = C.c_void_p()
        _lib.check(_lib.lib().kmhg_query_runs_device(self._h, C.byref(d)))
        return torch.as_tensor(_RowsBuffer(self, d.value, (n_runs, 3)))

    def free(self):
        if self._h:
            _lib.lib().kmhg_query_free(self._h)
            self._h = C.c_void_p(0)

    def __del__(self):
        try:
            self.free()
        except Exception:
            pass


class DeviceReadsQuery:
    """The rows of DeviceIndex.query_reads, held by the library until free()."""

    def __init__(self, handle: int, n_rows: int, n_reads: int, k: int, device: torch.device):
        self._h = C.c_void_p(handle)
        self.n_rows, self.n_reads, self.k, self.device = n_rows, n_reads, k, device

    def rows(self, stream=None) -> torch.Tensor:
        """A copy of the (H, 4) int32 rows (read, strand, i, j) on the query's device."""
        t = torch.empty((self.n_rows, 4), dtype=torch.int32, device=self.device)
        if self.n_rows:
            with torch.cuda.device(self.device):
                _lib.check(_lib.lib().kmhg_rquery_copy_device(self._h, C.c_void_p(t.data_ptr()),
                                                              _stream_ptr(stream)))
        return t

    def votes(self, band: int = 64, stream=None) -> torch.Tensor:
        """reads.kmer.vote of these rows (kmhg_rquery_votes_device): (n_reads, 6) int32
        (read, strand, pos, hits, second, total) on the query's device."""
        t = torch.empty((self.n_reads, 6), dtype=torch.int32, device=self.device)
        with torch.cuda.device(self.device):
            _lib.check(_lib.lib().kmhg_rquery_votes_device(self._h, int(band),
                                                           C.c_void_p(t.data_ptr()),
                                                           _stream_ptr(stream)))
        return t

    def free(self):
        if self._h:
            _lib.lib().kmhg_rquery_free(self._h)
            self._h = C.c_void_p(0)

    def __del__(self):
        try:
            self.free()
        except Exception:
            pass


def rows_votes(rows: torch.Tensor, n_reads: int, k: int, band: int = 64,
               stream=None) -> torch.Tensor:
    """reads.kmer.vote of any (H, 4) int32 CUDA rows (read, strand, i, j) of a query at `k`, in
    any order (kmhg_rrows_votes): (n_reads, 6) int32 on the rows' device.  A row votes for
    pos = j - i + k, which is why the query's k is an argument."""
    if not (rows.is_cuda and rows.dtype == torch.int32 and rows.dim() == 2 and
            rows.shape[1] == 4 and rows.is_contiguous()):
        raise TypeError("rows must be a contiguous (H, 4) torch.int32 CUDA tensor")
    t = torch.empty((int(n_reads), 6), dtype=torch.int32, device=rows.device)
    with torch.cuda.device(rows.device):
        _lib.check(_lib.lib().kmhg_rrows_votes(C.c_void_p(rows.data_ptr()), rows.shape[0],
                                               int(n_reads), int(k), int(band),
                                               C.c_void_p(t.data_ptr()), _stream_ptr(stream)))
    return t


class _RowsBuffer:
    """__cuda_array_interface__ of a query's device rows; torch keeps this object (and so the
    query) alive for as long as the tensor made from it."""

    def __init__(self, q, ptr: int, shape: tuple | None = None):
        self.q = q
        self.__cuda_array_interface__ = {"shape": shape or (q.n_rows, 2), "typestr": "<i4",
                                         "data": (ptr, False), "version": 3, "strides": None,
                                         "stream": None}


def timing_enable(on: bool = True):
    _lib.check(_lib.lib().kmhg_timing_enable(1 if on else 0))


def timing_select(kernel: str | None):
    """Record events only around `kernel` (None = every kernel)."""
    _lib.check(_lib.lib().kmhg_timing_select(kernel.encode() if kernel else None))


def timing_reset():
    _lib.check(_lib.lib().kmhg_timing_reset())


def timing_report() -> dict:
    buf = C.create_string_buffer(1 << 16)
    _lib.check(_lib.lib().kmhg_timing_report(buf, len(buf)))
    return json.loads(buf.value.decode())


class DeviceReads:
    """Packed reads in HBM for kmhg_sh_count_reads_device: bases and qualities (8-B aligned,
    16 B of padding), int64 offsets[n + 1], has_qual[n] (0 = FASTA record)."""

    def __init__(self, seq, qual, off, hasq):
        self.seq, self.qual, self.off, self.hasq = seq, qual, off, hasq
        self.n = int(hasq.numel())

    @classmethod
    def from_arrays(cls, seq, qual, device, has_qual=None) -> "DeviceReads":
        """seq / qual: (n_reads, read_len) uint8 numpy arrays (synth.reads)."""
        import numpy as np
        n, rl = seq.shape
        flat = np.zeros(n * rl + 16, np.uint8)
        flat[:n * rl] = seq.reshape(-1)
        qf = np.zeros(n * rl + 16, np.uint8)
        qf[:n * rl] = qual.reshape(-1)
        off = np.arange(n + 1, dtype=np.int64) * rl
        hq = np.ones(n, np.uint8) if has_qual is None else has_qual.astype(np.uint8)
        t = lambda a: torch.from_numpy(a).to(device)  # noqa: E731
        return cls(t(flat), t(qf), t(off), t(hq))

    @property
    def n_bases(self) -> int:
        return int(self.off[-1].item())
