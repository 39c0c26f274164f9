// kmhg_readsq_dev.h -- launchers of kmhg_readsq.hip (reads.kmer.pos / reads.kmer.vote on the
// device).  The rules the kernels evaluate are kmhg_readsq.h's.
#pragma once
#include <hip/hip_runtime.h>
#include "kmhg_common.h"

namespace kmhg {

// *bad (zeroed by the caller) <- 1 if off[0 .. n_reads] breaks rq_off_ok_at anywhere.
void launch_rq_check(const int64_t* off, int64_t n_reads, int64_t n_bases, uint32_t* bad,
                     hipStream_t s);
// The records (put_qrec) of the V = ns * n_bases > 0 virtual entries and the hit total of every
// tile of TILE entries; launch_qrec_mask and launch_scan_u64 then run as for a single query.
// Whatever off holds, nothing outside seq[0, n_bases) and off[0 .. n_reads] is read.
void launch_rq_probe(const uint8_t* seq, int64_t n_bases, const int64_t* off, int64_t n_reads,
                     int k, int ns, bool rev_only, const Slot* T, Geom g, uint32_t* qrec,
                     uint2* qmulti, uint64_t* tile_rows, hipStream_t s);
// The rows (read, strand, i, j), 16 B each, at the scanned tile offsets; rows at or beyond `cap`
// are dropped (the caller emits again into an exact buffer).
void launch_rq_emit(const uint32_t* qrec, const uint2* qmulti, const int64_t* off, int64_t n_reads,
                    int64_t n_bases, int k, int ns, bool rev_only, const int32_t* positions,
                    const uint64_t* tile_row0, int32_t* out, uint64_t cap, hipStream_t s);
// reads.kmer.vote of n rows (n <= 2^31 - 1): out = n_reads x VOTE_COLS.  keys: 2 n u64; cells, votes:
// n each; n_cells: one u32; best, second, total: n_reads each; temp: vote_temp_bytes(n).  *bad
// (zeroed by the caller) <- 1 for a row whose read is outside 1 .. n_reads or whose strand is not
// +-1; such a row is counted for read 1 and no access leaves the arrays.
hipError_t vote_temp_bytes(uint64_t n, size_t* bytes);
hipError_t launch_votes(const int32_t* rows, uint64_t n, int64_t n_reads, int k, int64_t band,
                        uint64_t* keys, uint64_t* cells, uint32_t* votes, uint32_t* n_cells,
                        void* temp, size_t temp_bytes, uint64_t* best, uint32_t* second,
                        uint32_t* total, int32_t* out, uint32_t* bad, hipStream_t s);

}  // namespace kmhg
