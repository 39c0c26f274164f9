// kmhg_parts_read.h -- launch wrappers of kmer.pos over owner-computes parts (kmhg_parts_read.hip
// and the label variants of the readout kernels in kmhg_kernels.hip).
//
// kmer.pos labels a k-mer by the rank of its first position among all k-mers' first positions
// (k_read_first / k_read_order).  Every k-mer lives in exactly one part, so the parts' first
// positions are disjoint and their union is the whole index's: a part marks its own in a bitmap
// of L bits, the ranks OR (= sum) the bitmaps, and a k-mer's global label is the number of set
// bits at or before its first position.  The index itself never moves.
#pragma once
#include <hip/hip_runtime.h>
#include "kmhg_common.h"

namespace kmhg {

inline uint64_t mask_words(int64_t L) { return (uint64_t)((L + 31) / 32); }

// mask (mask_words(L) u32, zeroed by the caller): bit (p - 1) & 31 of word (p - 1) >> 5 set for
// the first position p (1-based) of every occupied slot of T
void launch_part_mask(const Slot* T, uint64_t nslots, const int32_t* positions, int64_t L,
                      uint32_t* mask, hipStream_t s);
// wprefix[w] = set bits of mask words [0, w): one look-back chain over tiles of TILE words
// (`status` = tiles_for(W) zeroed u64, `ticket` a zeroed u32)
void launch_mask_prefix(const uint32_t* mask, uint64_t W, uint64_t* status, uint32_t* ticket,
                        uint32_t* wprefix, hipStream_t s);
// labels[c] = set bits of the merged mask at or before the first position of the part's row c
// (rinfo = the part's own first-occurrence readout order): its 1-based row in the whole kmer.pos
void launch_part_labels(const uint2* rinfo, uint32_t U, const int32_t* positions,
                        const uint32_t* mask, const uint32_t* wprefix, uint64_t W,
                        int32_t* labels, hipStream_t s);
// k_read_pos / k_read_pairs writing labels[row] instead of row + 1 (kmhg_kernels.hip)
void launch_read_pos_labels(const uint2* rinfo, const uint32_t* canon_off, uint32_t U,
                            uint64_t nrows, const int32_t* positions, uint32_t* tile_key,
                            const int32_t* labels, int2* out, hipStream_t s);
void launch_read_pairs_labels(const uint32_t* pkeys, const uint64_t* pair_off, uint32_t M,
                              uint64_t nrows, const uint2* rinfo, const int32_t* positions,
                              uint32_t* tile_key, const int32_t* labels, int32_t* out,
                              hipStream_t s);

// ---- the root's merge (kmhg_merge_part_positions) -------------------------------------------
// one part's counts / strings to their global rows: gcount[labels[i] - 1] = counts[i] (gcount
// optional), the k + 1 chars of string i to row labels[i] - 1 of gkmers (kmers optional)
void launch_merge_keys(const int32_t* labels, const int32_t* counts, const char* kmers,
                       uint32_t Up, int k, uint32_t U, int32_t* gcount, char* gkmers,
                       hipStream_t s);
// a[i] = counts[i] (pairs = false) or counts[i] * (counts[i] - 1) / 2 (pairs = true)
void launch_rows_per_key(const int32_t* counts, uint32_t n, bool pairs, uint64_t* a,
                         hipStream_t s);
// delta[labels[i] - 1] = goff[labels[i] - 1] - loff[i]: where the part's row run of key i goes
void launch_merge_delta(const int32_t* labels, const uint64_t* loff, const uint64_t* goff,
                        uint32_t Up, uint32_t U, int64_t* delta, hipStream_t s);
// out row (j + delta[label of row j - 1]) = part row j, rows of W int32 whose first is the label
void launch_merge_rows(const int32_t* rows, uint64_t n_rows, int W, const int64_t* delta,
                       uint32_t U, uint64_t n_out, int32_t* out, hipStream_t s);

}  // namespace kmhg
