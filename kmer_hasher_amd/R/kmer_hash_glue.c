/*
 * kmer_hash_glue.c -- R .Call bridge over the libkmhgpu C-ABI (include/kmhgpu.h).
 *
 * Drop-in for the index and read-counting halves of the reference's src/kmer_hash.c: the .Call
 * symbols with the same arities (registration as in src/kmer_hash.c:1205-1224), the same
 * argument validation and error() texts, the same externalptr tag "kmer_hash_250930"
 * (src/kmer_hash.c:22) and return shapes:
 *
 *   make_kmer_h_index(seq, k, do_sort)      src/kmer_hash.c:506-540   -> EXTPTRSXP
 *   kmer_positions(ptr, opt_flag)           src/kmer_hash.c:1054-1147 -> named VECSXP[4]
 *   sequence_kmer_positions(ptr, seq, k)    src/kmer_hash.c:1151-1172 -> INTSXP 2 x H
 *   kmer_pair_pos(ptr_a, ptr_b)             src/kmer_hash.c:1174-1203 -> INTSXP 2 x M (fixed)
 *   count_kmers(hash_ptr, params, seq)      src/kmer_hash.c:548-591   -> EXTPTRSXP (counts)
 *   count_kmers_fastq_sh_rp(ptr, params, f) src/kmer_hash.c:810-857   -> EXTPTRSXP (suffix_hash_n)
 *   seq_kmer_depth_sh(ptr, seq, k)          src/kmer_hash.c:859-879   -> INTSXP counts_n x L
 *   kmer_spectrum_suffix_hash_n(ptr, ...)   src/kmer_hash.c:1010-1039 -> REALSXP
 *   count_kmers_fastq_sh(ptr, params, f)    src/kmer_hash.c:715-806   -> EXTPTRSXP (suffix_hash)
 *   kmer_spectrum_suffix_hash(ptr, max)     src/kmer_hash.c:993-1008  -> REALSXP
 *   sequence_kmer_positions_rc(ptr, seq, k) (not in the reference)    -> INTSXP 2 x H
 *   sequence_kmer_segments(ptr, seq, k, min_len, rc) (not in the reference) -> INTSXP 3 x S
 *   sequence_kmer_blocks(ptr, seq, k, max_gap, min_len, min_hits, rc) (not in the reference)
 *                                                                     -> INTSXP 4 x B
 *   sequence_kmer_segments_rf, sequence_kmer_blocks_rf (not in the reference): the two above by
 *                                                  the route that never writes the positions
 *   sequence_kmer_chains(ptr, seq, k, max_dist, max_drift, max_gap, min_len, min_hits, rc,
 *                        row_free) (not in the reference)
 *                                  -> named VECSXP[3]: INTSXP 6 x C, INTSXP 4 x B, INTSXP B
 *   sequence_kmer_raster(ptr, seq, k, bins, rc, i_range, j_range) (not in the reference)
 *                                                  -> named VECSXP[6], counts REALSXP n_i x n_j
 *   kmer_max_occ(ptr, max_occ) (not in the reference)                 -> INTSXP 1: the old value
 *   make_kmer_h_index_min(seq, k, w, sort_pos) (not in the reference) -> EXTPTRSXP, as make_kmer_h_index
 *   reads_kmer_positions(ptr, seqs, k, strand) (not in the reference) -> INTSXP 4 x H
 *   reads_kmer_votes(ptr, seqs, k, band, strand) (not in the reference) -> INTSXP 6 x n
 *
 * Differences, all deliberate: the finaliser frees the whole payload (the reference leaks the
 * 32-B khash_ptr, src/kmer_hash.c:56-66); a freed pointer is detected instead of dereferenced;
 * result sizes are checked against R's int ncol before allocMatrix (the reference overflows at
 * 2^31 pair rows, README.md:80-89).  Results are written by the GPU library straight into the
 * R-allocated INTSXP buffers (one D2H copy, no kvec temporaries).
 *
 * Build (R headers required; R is not installed in the development image, so this file is
 * compiled by R CMD SHLIB on the user's machine -- see INTEGRATION.md):
 *   R CMD SHLIB -o kmer_hash.so kmer_hash_glue.c -I../../include -L.. -lkmhgpu \
 *       -Wl,-rpath,'$ORIGIN/..'
 */
#include <R.h>
#include <Rinternals.h>
#include <R_ext/Rdynload.h>
#include <limits.h>
#include <stdlib.h>
#include <string.h>

#include "kmhgpu.h"

static const char *kmer_hash_tag = "kmer_hash_250930";
static const char *pos_fields[4] = {"kmer", "pos", "pair.pos", "count"};

static void finalise_gpu_index(SEXP ptr_r) {
  kmhg_index *idx = (kmhg_index *)R_ExternalPtrAddr(ptr_r);
  if (idx) {
    kmhg_free(idx);
    R_ClearExternalPtr(ptr_r);
  }
}

/* extract_khash_ptr, src/kmer_hash.c:491-503 (same messages) */
static kmhg_index *gpu_index_of(SEXP ptr_r) {
  if (TYPEOF(ptr_r) != EXTPTRSXP) error("ptr_r should be an external pointer");
  SEXP tag = R_ExternalPtrTag(ptr_r);
  if (TYPEOF(tag) != STRSXP || length(tag) != 1 || strcmp(CHAR(STRING_ELT(tag, 0)), kmer_hash_tag))
    error("External pointer has incorrect tag");
  kmhg_index *idx = (kmhg_index *)R_ExternalPtrAddr(ptr_r);
  if (!idx) error("external pointer has been finalised");
  return idx;
}

SEXP make_kmer_h_index(SEXP seq_r, SEXP k_r, SEXP sort_pos_r) {
  if (TYPEOF(seq_r) != STRSXP || length(seq_r) < 1)
    error("seq_r should be a character vector of length at least one");
  if (TYPEOF(k_r) != INTSXP || length(k_r) < 1)
    error("k_r must be an integer vector of length at least one");
  if (TYPEOF(sort_pos_r) != INTSXP || length(k_r) < 1)
    error("sort_pos_r must be an integer vector of length at least one");
  int k = INTEGER(k_r)[0];
  int do_sort = asInteger(sort_pos_r);
  SEXP s = STRING_ELT(seq_r, 0);
  kmhg_index *idx = NULL;
  int rc = kmhg_build(CHAR(s), (size_t)length(s), k, do_sort, &idx);
  if (rc != KMHG_OK) error("%s", kmhg_last_error());
  SEXP tag = PROTECT(allocVector(STRSXP, 1));
  SET_STRING_ELT(tag, 0, mkChar(kmer_hash_tag));
  SEXP ptr = PROTECT(R_MakeExternalPtr(idx, tag, R_NilValue));
  R_RegisterCFinalizerEx(ptr, finalise_gpu_index, TRUE);
  UNPROTECT(2);
  return ptr;
}

/* make.kmer.hash.min (not in the reference; include/kmhgpu.h, kmhg_build_sampled): the index of
 * the (w,k)-minimizer windows of the sequence alone.  Exported and found by name, not in the
 * registration table.  Every refusal of an argument is raised here, before the GPU is touched. */
SEXP make_kmer_h_index_min(SEXP seq_r, SEXP k_r, SEXP w_r, SEXP sort_pos_r) {
  if (TYPEOF(seq_r) != STRSXP || length(seq_r) < 1)
    error("seq_r should be a character vector of length at least one");
  if (TYPEOF(k_r) != INTSXP || length(k_r) < 1)
    error("k_r must be an integer vector of length at least one");
  if (TYPEOF(w_r) != INTSXP || length(w_r) != 1 || INTEGER(w_r)[0] == INT_MIN)
    error("w should be an integer of length 1");
  if (TYPEOF(sort_pos_r) != INTSXP || length(sort_pos_r) < 1)
    error("sort_pos_r must be an integer vector of length at least one");
  int w = INTEGER(w_r)[0];
  if (w < 1 || w > 256) error("w must be between 1 and 256");
  int k = INTEGER(k_r)[0];
  if (k < 1 || k > 31) error("a sampled index needs k between 1 and 31");
  SEXP s = STRING_ELT(seq_r, 0);
  if (length(s) <= k) error("the length of the sequence must be at least k");
  kmhg_index *idx = NULL;
  int rc = kmhg_build_sampled(CHAR(s), (size_t)length(s), k, w, asInteger(sort_pos_r), &idx);
  if (rc != KMHG_OK) error("%s", kmhg_last_error());
  SEXP tag = PROTECT(allocVector(STRSXP, 1));
  SET_STRING_ELT(tag, 0, mkChar(kmer_hash_tag));
  SEXP ptr = PROTECT(R_MakeExternalPtr(idx, tag, R_NilValue));
  R_RegisterCFinalizerEx(ptr, finalise_gpu_index, TRUE);
  UNPROTECT(2);
  return ptr;
}

SEXP kmer_positions(SEXP ptr_r, SEXP opt_flag_r) {
  kmhg_index *idx = gpu_index_of(ptr_r);
  if (TYPEOF(opt_flag_r) != INTSXP || length(opt_flag_r) != 1)
    error("opt_flag_r should be an integer vector of length 1");
  uint32_t opt = (uint32_t)asInteger(opt_flag_r);
  int64_t nk = 0, np = 0, npp = 0, nc = 0;
  if (kmhg_positions_size(idx, opt, &nk, &np, &npp, &nc) != KMHG_OK)
    error("%s", kmhg_last_error());
  if (np > INT_MAX || npp > INT_MAX || nk > INT_MAX)
    error("result has more than 2^31-1 columns (R matrix limit)");
  kmhg_info info;
  kmhg_index_info(idx, &info);
  SEXP ret = PROTECT(allocVector(VECSXP, 4));
  SEXP nm = PROTECT(allocVector(STRSXP, 4));
  for (int i = 0; i < 4; ++i) SET_STRING_ELT(nm, i, mkChar(pos_fields[i]));
  setAttrib(ret, R_NamesSymbol, nm);
  int *pos = NULL, *pairs = NULL, *counts = NULL;
  char *kmers = NULL;
  if (opt & KMHG_OPT_POS) {
    SET_VECTOR_ELT(ret, 1, allocMatrix(INTSXP, 2, (int)np));
    pos = INTEGER(VECTOR_ELT(ret, 1));
  }
  if (opt & KMHG_OPT_PAIRS) {
    SET_VECTOR_ELT(ret, 2, allocMatrix(INTSXP, 3, (int)npp));
    pairs = INTEGER(VECTOR_ELT(ret, 2));
  }
  if (opt & KMHG_OPT_COUNT) {
    SET_VECTOR_ELT(ret, 3, allocVector(INTSXP, (R_xlen_t)nc));
    counts = INTEGER(VECTOR_ELT(ret, 3));
  }
  if ((opt & KMHG_OPT_KMER) && nk) kmers = (char *)R_alloc((size_t)nk, info.k + 1);
  if (kmhg_positions_fill(idx, opt, kmers, pos, pairs, counts) != KMHG_OK)
    error("%s", kmhg_last_error());
  if (opt & KMHG_OPT_KMER) {
    SET_VECTOR_ELT(ret, 0, allocVector(STRSXP, (R_xlen_t)nk));
    SEXP kr = VECTOR_ELT(ret, 0);
    for (int64_t i = 0; i < nk; ++i)
      SET_STRING_ELT(kr, (R_xlen_t)i, mkChar(kmers + (size_t)i * (info.k + 1)));
  }
  UNPROTECT(2);
  return ret;
}

/* sequence_kmer_positions and its reverse-strand twin: one body over the C-ABI entry. */
typedef int (*seq_query_fn)(kmhg_index *, const char *, size_t, int, kmhg_query **, int64_t *);
static SEXP seq_positions_by(seq_query_fn run, SEXP ptr_r, SEXP seq_r, SEXP k_r) {
  kmhg_index *idx = gpu_index_of(ptr_r);
  if (TYPEOF(seq_r) != STRSXP || length(seq_r) != 1) error("seq_r should be a single sequence");
  if (TYPEOF(k_r) != INTSXP || length(k_r) != 1) error("k should be an integer of length 1");
  int k = INTEGER(k_r)[0];
  SEXP s = STRING_ELT(seq_r, 0);
  kmhg_query *q = NULL;
  int64_t h = 0;
  if (run(idx, CHAR(s), (size_t)length(s), k, &q, &h) != KMHG_OK)
    error("%s", kmhg_last_error());
  if (h > INT_MAX) {
    kmhg_query_free(q);
    error("result has more than 2^31-1 columns (R matrix limit)");
  }
  SEXP ret = PROTECT(allocMatrix(INTSXP, 2, (int)h));
  int rc = h ? kmhg_query_fill(q, INTEGER(ret)) : KMHG_OK;
  kmhg_query_free(q);
  if (rc != KMHG_OK) error("%s", kmhg_last_error());
  UNPROTECT(1);
  return ret;
}

/* With KMHG_DEVICES=d0,d1,... in the environment, kmhg_query_run splits the query over those
 * GPUs (index replicas peer-copied once, rows filled straight into the R matrix by
 * kmhg_query_fill at each device's row offset): same signature, same result. */
SEXP sequence_kmer_positions(SEXP ptr_r, SEXP seq_r, SEXP k_r) {
  return seq_positions_by(kmhg_query_run, ptr_r, seq_r, k_r);
}

/* Not in the reference: sequence_kmer_positions of the REVERSE COMPLEMENT of seq, made on the
 * device from the forward string (kmhg_query_run_rc, include/kmhgpu.h) -- what the reference's
 * usage script computes as seq.kmer.pos(hash, reverseComplement(x), k) (test.R:42-43) with
 * rev.comp's 2-bit rule (test.R:31-36), except that N stays N (rev.comp turns it into C).  Same
 * validation in the same order, same INTSXP 2 x H of (i, j) in the coordinates of rc(seq): a
 * row's window starts at forward position nchar(seq) - i + 1.  Exported, but like
 * count_kmers_fastq_sh not in the registration table (.Call by name finds it by its dynamic
 * lookup).  KMHG_DEVICES is not honoured. */
SEXP sequence_kmer_positions_rc(SEXP ptr_r, SEXP seq_r, SEXP k_r) {
  return seq_positions_by(kmhg_query_run_rc, ptr_r, seq_r, k_r);
}

/* Not in the reference: the dot plot of seq against the index as maximal diagonal segments
 * (kmhg_query_segments, include/kmhgpu.h, which cites the reference author's abandoned
 * offset_diagonals, src/kmer_hash.c:414-486).  Runs sequence_kmer_positions (rc = 0) or
 * sequence_kmer_positions_rc (rc != 0) and returns INTSXP 3 x S of (i, j, len), ordered by (i, j):
 * rows (i + t, j + t), t < len, are all among the positions and neither (i - 1, j - 1) nor
 * (i + len, j + len) is; only segments of at least min_len rows are kept.  The argument checks
 * come first, in argument order after the sequence's and k's own words; the pointer must be a
 * position index (a count.kmers pointer's "positions" are count vectors).  Exported, not
 * registered, like sequence_kmer_positions_rc. */
static SEXP segments_by(int row_free, SEXP ptr_r, SEXP seq_r, SEXP k_r, SEXP min_len_r,
                        SEXP rc_r) {
  if (TYPEOF(seq_r) != STRSXP || length(seq_r) != 1) error("seq_r should be a single sequence");
  if (TYPEOF(k_r) != INTSXP || length(k_r) != 1) error("k should be an integer of length 1");
  if (TYPEOF(min_len_r) != INTSXP || length(min_len_r) != 1 || INTEGER(min_len_r)[0] < 1)
    error("min_len must be a positive integer");
  if (TYPEOF(rc_r) != INTSXP || length(rc_r) != 1) error("rc should be an integer of length 1");
  kmhg_index *idx = gpu_index_of(ptr_r);
  kmhg_info inf;
  if (kmhg_index_info(idx, &inf) != KMHG_OK) error("%s", kmhg_last_error());
  if (inf.kind != 0) error("segments need a position index");
  int k = asInteger(k_r);
  SEXP s = STRING_ELT(seq_r, 0);
  kmhg_query *q = NULL;
  kmhg_segs *g = NULL;
  int64_t h = 0, n = 0;
  int rc;
  if (row_free) {
    rc = kmhg_segments_run(idx, CHAR(s), (size_t)length(s), k, INTEGER(rc_r)[0] != 0,
                           INTEGER(min_len_r)[0], &g, &n, &h);
  } else {
    if ((INTEGER(rc_r)[0] ? kmhg_query_run_rc : kmhg_query_run)(idx, CHAR(s), (size_t)length(s), k,
                                                                &q, &h) != KMHG_OK)
      error("%s", kmhg_last_error());
    rc = kmhg_query_segments(q, INTEGER(min_len_r)[0], &g, &n);
    kmhg_query_free(q);
  }
  if (rc != KMHG_OK) error("%s", kmhg_last_error());
  if (n > INT_MAX) {
    kmhg_segs_free(g);
    error("result has more than 2^31-1 columns (R matrix limit)");
  }
  SEXP ret = PROTECT(allocMatrix(INTSXP, 3, (int)n));
  rc = kmhg_segs_fill(g, INTEGER(ret));
  kmhg_segs_free(g);
  if (rc != KMHG_OK) error("%s", kmhg_last_error());
  UNPROTECT(1);
  return ret;
}

SEXP sequence_kmer_segments(SEXP ptr_r, SEXP seq_r, SEXP k_r, SEXP min_len_r, SEXP rc_r) {
  return segments_by(0, ptr_r, seq_r, k_r, min_len_r, rc_r);
}

/* sequence_kmer_segments by the route that never writes the positions (kmhg_segments_run,
 * include/kmhgpu.h): the same arguments, checks and INTSXP 3 x S, byte for byte, and defined where
 * the positions are more than 2^31-1.  Exported, not registered. */
SEXP sequence_kmer_segments_rf(SEXP ptr_r, SEXP seq_r, SEXP k_r, SEXP min_len_r, SEXP rc_r) {
  return segments_by(1, ptr_r, seq_r, k_r, min_len_r, rc_r);
}

/* Not in the reference: the segments of sequence_kmer_segments merged, on every diagonal, across
 * gaps of at most max_gap windows (kmhg_query_blocks, include/kmhgpu.h).  Returns INTSXP 4 x B of
 * (i, j, span, hits), ordered by (i, j): span = the windows from the block's first row to its
 * last, hits = its rows; only segments of at least min_len rows take part and only blocks of at
 * least min_hits rows are kept.  The argument checks come first, in the C-ABI's words and order
 * after the sequence's and k's own; the pointer must be a position index.  Exported, not
 * registered, like sequence_kmer_segments. */
static SEXP blocks_by(int row_free, SEXP ptr_r, SEXP seq_r, SEXP k_r, SEXP max_gap_r,
                      SEXP min_len_r, SEXP min_hits_r, SEXP rc_r) {
  if (TYPEOF(seq_r) != STRSXP || length(seq_r) != 1) error("seq_r should be a single sequence");
  if (TYPEOF(k_r) != INTSXP || length(k_r) != 1) error("k should be an integer of length 1");
  if (TYPEOF(min_len_r) != INTSXP || length(min_len_r) != 1 || INTEGER(min_len_r)[0] < 1)
    error("min_len must be a positive integer");
  if (TYPEOF(max_gap_r) != INTSXP || length(max_gap_r) != 1 || INTEGER(max_gap_r)[0] < 0)
    error("max_gap must not be negative");
  if (TYPEOF(min_hits_r) != INTSXP || length(min_hits_r) != 1 || INTEGER(min_hits_r)[0] < 1)
    error("min_hits must be a positive integer");
  if (TYPEOF(rc_r) != INTSXP || length(rc_r) != 1) error("rc should be an integer of length 1");
  kmhg_index *idx = gpu_index_of(ptr_r);
  kmhg_info inf;
  if (kmhg_index_info(idx, &inf) != KMHG_OK) error("%s", kmhg_last_error());
  if (inf.kind != 0) error("blocks need a position index");
  int k = asInteger(k_r);
  SEXP s = STRING_ELT(seq_r, 0);
  kmhg_query *q = NULL;
  kmhg_blocks *b = NULL;
  int64_t h = 0, n = 0;
  int rc;
  if (row_free) {
    rc = kmhg_blocks_run(idx, CHAR(s), (size_t)length(s), k, INTEGER(rc_r)[0] != 0,
                         INTEGER(min_len_r)[0], INTEGER(max_gap_r)[0], INTEGER(min_hits_r)[0], &b,
                         &n, &h);
  } else {
    if ((INTEGER(rc_r)[0] ? kmhg_query_run_rc : kmhg_query_run)(idx, CHAR(s), (size_t)length(s), k,
                                                                &q, &h) != KMHG_OK)
      error("%s", kmhg_last_error());
    rc = kmhg_query_blocks(q, INTEGER(min_len_r)[0], INTEGER(max_gap_r)[0],
                           INTEGER(min_hits_r)[0], &b, &n);
    kmhg_query_free(q);
  }
  if (rc != KMHG_OK) error("%s", kmhg_last_error());
  if (n > INT_MAX) {
    kmhg_blocks_free(b);
    error("result has more than 2^31-1 columns (R matrix limit)");
  }
  SEXP ret = PROTECT(allocMatrix(INTSXP, 4, (int)n));
  rc = kmhg_blocks_fill(b, INTEGER(ret));
  kmhg_blocks_free(b);
  if (rc != KMHG_OK) error("%s", kmhg_last_error());
  UNPROTECT(1);
  return ret;
}

SEXP sequence_kmer_blocks(SEXP ptr_r, SEXP seq_r, SEXP k_r, SEXP max_gap_r, SEXP min_len_r,
                          SEXP min_hits_r, SEXP rc_r) {
  return blocks_by(0, ptr_r, seq_r, k_r, max_gap_r, min_len_r, min_hits_r, rc_r);
}

/* sequence_kmer_blocks by the route that never writes the positions (kmhg_blocks_run), as
 * sequence_kmer_segments_rf.  Exported, not registered. */
SEXP sequence_kmer_blocks_rf(SEXP ptr_r, SEXP seq_r, SEXP k_r, SEXP max_gap_r, SEXP min_len_r,
                             SEXP min_hits_r, SEXP rc_r) {
  return blocks_by(1, ptr_r, seq_r, k_r, max_gap_r, min_len_r, min_hits_r, rc_r);
}

/* Not in the reference: the blocks of sequence_kmer_blocks linked across diagonals into chains
 * (kmhg_chains_run, include/kmhgpu.h).  Returns a named list: chains, INTSXP 6 x C of (i, j,
 * i.end, j.end, hits, blocks) ordered by (i, j); blocks, INTSXP 4 x B of (i, j, span, hits), the
 * blocks at min_hits = 1; chain, INTSXP B, the 1-based chain of every block (0: its chain was
 * dropped by min_hits).  row_free != 0 takes the blocks by the route that never writes the
 * positions.  The argument checks come first, in the C-ABI's words and order after the sequence's
 * and k's own; the pointer must be a position index.  Exported, not registered, like
 * sequence_kmer_blocks. */
static const char *chains_fields[3] = {"chains", "blocks", "chain"};

SEXP sequence_kmer_chains(SEXP ptr_r, SEXP seq_r, SEXP k_r, SEXP max_dist_r, SEXP max_drift_r,
                          SEXP max_gap_r, SEXP min_len_r, SEXP min_hits_r, SEXP rc_r,
                          SEXP row_free_r) {
  if (TYPEOF(seq_r) != STRSXP || length(seq_r) != 1) error("seq_r should be a single sequence");
  if (TYPEOF(k_r) != INTSXP || length(k_r) != 1) error("k should be an integer of length 1");
  if (TYPEOF(min_len_r) != INTSXP || length(min_len_r) != 1 || INTEGER(min_len_r)[0] < 1)
    error("min_len must be a positive integer");
  if (TYPEOF(max_gap_r) != INTSXP || length(max_gap_r) != 1 || INTEGER(max_gap_r)[0] < 0)
    error("max_gap must not be negative");
  if (TYPEOF(max_dist_r) != INTSXP || length(max_dist_r) != 1 || INTEGER(max_dist_r)[0] < 0)
    error("max_dist must not be negative");
  if (TYPEOF(max_drift_r) != INTSXP || length(max_drift_r) != 1 || INTEGER(max_drift_r)[0] < 0)
    error("max_drift must not be negative");
  if (TYPEOF(min_hits_r) != INTSXP || length(min_hits_r) != 1 || INTEGER(min_hits_r)[0] < 1)
    error("min_hits must be a positive integer");
  if (TYPEOF(rc_r) != INTSXP || length(rc_r) != 1) error("rc should be an integer of length 1");
  if (TYPEOF(row_free_r) != INTSXP || length(row_free_r) != 1)
    error("row_free should be an integer of length 1");
  kmhg_index *idx = gpu_index_of(ptr_r);
  kmhg_info inf;
  if (kmhg_index_info(idx, &inf) != KMHG_OK) error("%s", kmhg_last_error());
  if (inf.kind != 0) error("blocks need a position index");
  int k = asInteger(k_r);
  SEXP s = STRING_ELT(seq_r, 0);
  kmhg_chains *c = NULL;
  int64_t nc = 0, nb = 0;
  if (kmhg_chains_run(idx, CHAR(s), (size_t)length(s), k, INTEGER(rc_r)[0] != 0,
                      INTEGER(row_free_r)[0] != 0, INTEGER(min_len_r)[0], INTEGER(max_gap_r)[0],
                      INTEGER(max_dist_r)[0], INTEGER(max_drift_r)[0], INTEGER(min_hits_r)[0], &c,
                      &nc, &nb, NULL) != KMHG_OK)
    error("%s", kmhg_last_error());
  if (nb > INT_MAX) {
    kmhg_chains_free(c);
    error("result has more than 2^31-1 columns (R matrix limit)");
  }
  SEXP ret = PROTECT(allocVector(VECSXP, 3));
  SEXP nm = PROTECT(allocVector(STRSXP, 3));
  for (int i = 0; i < 3; ++i) SET_STRING_ELT(nm, i, mkChar(chains_fields[i]));
  setAttrib(ret, R_NamesSymbol, nm);
  SEXP chains = SET_VECTOR_ELT(ret, 0, allocMatrix(INTSXP, 6, (int)nc));
  SEXP blocks = SET_VECTOR_ELT(ret, 1, allocMatrix(INTSXP, 4, (int)nb));
  SEXP chain = SET_VECTOR_ELT(ret, 2, allocVector(INTSXP, (int)nb));
  int rc = kmhg_chains_fill(c, INTEGER(chains));
  if (rc == KMHG_OK) rc = kmhg_chains_member_fill(c, INTEGER(chain), nb ? INTEGER(blocks) : NULL);
  kmhg_chains_free(c);
  if (rc != KMHG_OK) error("%s", kmhg_last_error());
  UNPROTECT(2);
  return ret;
}

/* Not in the reference: the dot plot as a binned count matrix (kmhg_raster_run, include/kmhgpu.h),
 * made on the device without writing the rows, so its size does not depend on the hit count and
 * the query's 2^31-row limit does not apply.  bins: one or two bin counts (i, j); i_range /
 * j_range: c(lo, hi), inclusive and 1-based, or NULL for 1..nchar(seq) and 1..the index's length.
 * Per axis, width = ceil(range length / bins) and count = ceil(range length / width).  Returns a
 * named list: counts, a REALSXP n_i x n_j matrix (a cell may exceed INT_MAX), i0, j0, bin_i, bin_j
 * (integers) and n_rows, the query's hit total (a double: it may exceed INT_MAX).  The argument
 * checks come first; the pointer must be a position index.  Exported, not registered, like
 * sequence_kmer_segments. */
static const char *raster_fields[6] = {"counts", "i0", "j0", "bin_i", "bin_j", "n_rows"};

static int raster_range_ok(SEXP r) {
  if (TYPEOF(r) == NILSXP) return 1;
  return TYPEOF(r) == INTSXP && length(r) == 2 && INTEGER(r)[0] >= 1 &&
         INTEGER(r)[1] >= INTEGER(r)[0];
}

static void raster_axis(SEXP range_r, int64_t deflt_hi, int64_t bins, int64_t *lo, int64_t *width,
                        int64_t *n) {
  *lo = TYPEOF(range_r) == NILSXP ? 1 : INTEGER(range_r)[0];
  const int64_t hi = TYPEOF(range_r) == NILSXP ? (deflt_hi > 1 ? deflt_hi : 1) : INTEGER(range_r)[1];
  const int64_t len = hi - *lo + 1;
  *width = (len + bins - 1) / bins;
  *n = (len + *width - 1) / *width;
}

SEXP sequence_kmer_raster(SEXP ptr_r, SEXP seq_r, SEXP k_r, SEXP bins_r, SEXP rc_r, SEXP i_range_r,
                          SEXP j_range_r) {
  if (TYPEOF(seq_r) != STRSXP || length(seq_r) != 1) error("seq_r should be a single sequence");
  if (TYPEOF(k_r) != INTSXP || length(k_r) != 1) error("k should be an integer of length 1");
  if (TYPEOF(bins_r) != INTSXP || length(bins_r) < 1 || length(bins_r) > 2 ||
      INTEGER(bins_r)[0] < 1 || INTEGER(bins_r)[length(bins_r) - 1] < 1)
    error("bins should be one or two positive integers");
  if (TYPEOF(rc_r) != INTSXP || length(rc_r) != 1 ||
      INTEGER(rc_r)[0] == INT_MIN) /* NA_integer_ (as.integer(NA)): not a silent reverse strand */
    error("rc should be an integer of length 1");
  if (!raster_range_ok(i_range_r)) error("i.range should be c(lo, hi) with 1 <= lo <= hi");
  if (!raster_range_ok(j_range_r)) error("j.range should be c(lo, hi) with 1 <= lo <= hi");
  kmhg_index *idx = gpu_index_of(ptr_r);
  kmhg_info inf;
  if (kmhg_index_info(idx, &inf) != KMHG_OK) error("%s", kmhg_last_error());
  if (inf.kind != 0) error("a raster needs a position index");
  int k = asInteger(k_r);
  SEXP s = STRING_ELT(seq_r, 0);
  int64_t f[6];
  raster_axis(i_range_r, (int64_t)length(s), INTEGER(bins_r)[0], &f[0], &f[2], &f[4]);
  raster_axis(j_range_r, inf.seq_len, INTEGER(bins_r)[length(bins_r) - 1], &f[1], &f[3], &f[5]);
  /* (beyond 2^26 cells the library refuses before it writes: one element is enough) */
  const size_t cells = f[4] * f[5] <= ((int64_t)1 << 26) ? (size_t)(f[4] * f[5]) : 1;
  uint32_t *m = (uint32_t *)malloc(cells * sizeof(uint32_t));
  if (!m) error("out of memory");
  int64_t h = 0;
  if (kmhg_raster_run(idx, CHAR(s), (size_t)length(s), k, INTEGER(rc_r)[0] != 0, f, m, &h) !=
      KMHG_OK) {
    free(m);
    error("%s", kmhg_last_error());
  }
  SEXP ret = PROTECT(allocVector(VECSXP, 6));
  SEXP nm = PROTECT(allocVector(STRSXP, 6));
  for (int i = 0; i < 6; ++i) SET_STRING_ELT(nm, i, mkChar(raster_fields[i]));
  setAttrib(ret, R_NamesSymbol, nm);
  SEXP counts = SET_VECTOR_ELT(ret, 0, allocMatrix(REALSXP, (int)f[4], (int)f[5]));
  double *c = REAL(counts);
  for (size_t e = 0; e < cells; ++e) c[e] = (double)m[e];
  free(m);
  for (int i = 0; i < 4; ++i) {
    SEXP v = SET_VECTOR_ELT(ret, 1 + i, allocVector(INTSXP, 1));
    INTEGER(v)[0] = (int)f[i];
  }
  SEXP hr = SET_VECTOR_ELT(ret, 5, allocVector(REALSXP, 1));
  REAL(hr)[0] = (double)h;
  UNPROTECT(2);
  return ret;
}

/* kmer_pair_pos, src/kmer_hash.c:1174-1203 (called by kmer.pairs, kmer_hash.R:30-34): rows
 * (a, b) for the k-mers both indices hold.  The reference walks empty buckets and reads past
 * the end of b's flags (test.R:330 "This crashes"); kmhg_pairs_run defines the intended result
 * and refuses indices of different k. */
SEXP kmer_pair_pos(SEXP ptr_a, SEXP ptr_b) {
  kmhg_index *a = gpu_index_of(ptr_a);
  kmhg_index *b = gpu_index_of(ptr_b);
  kmhg_query *q = NULL;
  int64_t h = 0;
  if (kmhg_pairs_run(a, b, &q, &h) != KMHG_OK) error("%s", kmhg_last_error());
  if (h > INT_MAX) {
    kmhg_query_free(q);
    error("result has more than 2^31-1 columns (R matrix limit)");
  }
  SEXP ret = PROTECT(allocMatrix(INTSXP, 2, (int)h));
  int rc = h ? kmhg_query_fill(q, INTEGER(ret)) : KMHG_OK;
  kmhg_query_free(q);
  if (rc != KMHG_OK) error("%s", kmhg_last_error());
  UNPROTECT(1);
  return ret;
}

/* count_kmers, src/kmer_hash.c:548-591 (count.kmers, kmer_hash.R:43-46): per-source counts of
 * every k-mer of a character vector, added to hash_ptr_r or to a new counts pointer (same tag,
 * so kmer.pos / seq.kmer.pos read it, test.R:340-343).  Validation order and texts as the
 * reference; kmhg_count also refuses a position index and a different source_n, where the
 * reference would write past the end of a k-mer's vector. */
SEXP count_kmers(SEXP hash_ptr_r, SEXP params_r, SEXP seq_r) {
  if (TYPEOF(seq_r) != STRSXP || length(seq_r) < 1)
    error("seq_r should be a character vector of length at least one");
  if (TYPEOF(params_r) != INTSXP || length(params_r) != 3)
    error("k_r must be an integer vector of length 3");
  const int *params = INTEGER(params_r);
  const int k = params[0], source = params[1], source_n = params[2];
  if (k < 1 || k > 32) error("k must be a positive integer less than 1+MAX_K");
  if (source_n < 1 || source >= source_n)
    error("source_n must be larger than 1 and larger than source");
  kmhg_index *idx = NULL;
  if (hash_ptr_r != R_NilValue) {
    if (TYPEOF(hash_ptr_r) != EXTPTRSXP) error("failed to extract kmer_hash from external pointer");
    SEXP tag = R_ExternalPtrTag(hash_ptr_r);
    if (TYPEOF(tag) != STRSXP || length(tag) != 1 ||
        strcmp(CHAR(STRING_ELT(tag, 0)), kmer_hash_tag))
      error("failed to extract kmer_hash from external pointer");
    idx = (kmhg_index *)R_ExternalPtrAddr(hash_ptr_r);
    if (!idx) error("failed to extract kmer_hash from external pointer");
  }
  const R_xlen_t n = XLENGTH(seq_r);
  const char **seqs = (const char **)R_alloc((size_t)n, sizeof(char *));
  size_t *lens = (size_t *)R_alloc((size_t)n, sizeof(size_t));
  for (R_xlen_t i = 0; i < n; ++i) {
    SEXP e = STRING_ELT(seq_r, i);
    seqs[i] = CHAR(e);
    lens[i] = (size_t)length(e);
  }
  kmhg_index *out = idx;
  if (kmhg_count(&out, seqs, lens, (int64_t)n, k, source, source_n) != KMHG_OK)
    error("%s", kmhg_last_error());
  if (source < 0) warning("source (%d) equal to or larger than source_n (%d)", source, source_n);
  if (idx) return hash_ptr_r;
  SEXP tag = PROTECT(allocVector(STRSXP, 1));
  SET_STRING_ELT(tag, 0, mkChar(kmer_hash_tag));
  SEXP ptr = PROTECT(R_MakeExternalPtr(out, tag, R_NilValue));
  R_RegisterCFinalizerEx(ptr, finalise_gpu_index, TRUE);
  UNPROTECT(2);
  return ptr;
}

/* ---- suffix_hash_n (read counting) ------------------------------------------------------
 * Same tag as the reference's suffix hashes (src/kmer_hash.c:25), so pointers made here are
 * refused by kmer.pos exactly as the reference refuses a suffix_hash_n. */
static const char *suffix_hash_n_tag = "suffix_hash_n_250930";

/* extract_ext_ptr(ptr, suffix_hash_n_tag), src/kmer_hash.c:41-52: NULL for anything else */
static kmhg_index *gpu_sh_of(SEXP ptr_r) {
  if (TYPEOF(ptr_r) != EXTPTRSXP) return NULL;
  SEXP tag = R_ExternalPtrTag(ptr_r);
  if (TYPEOF(tag) != STRSXP || length(tag) != 1 ||
      strcmp(CHAR(STRING_ELT(tag, 0)), suffix_hash_n_tag))
    return NULL;
  return (kmhg_index *)R_ExternalPtrAddr(ptr_r);
}

static int gpu_sh_sources(kmhg_index *sh) {
  kmhg_info info;
  if (kmhg_index_info(sh, &info) != KMHG_OK) error("%s", kmhg_last_error());
  return info.sources;
}

/* count_kmers_fastq_sh_rp, src/kmer_hash.c:810-857 (count.kmers.fq.sh.rp, kmer_hash.R:70-73):
 * params = (k, prefix_bits, min_q, thread_n, max_reads, max_mem, source_n, source); the
 * canonical k-mers of the FASTA/FASTQ file the quality iterator accepts, counted on the GPU
 * into entry `source` of a new or the given suffix hash.  Validation order and texts as the
 * reference (kmhg_sh_count_fastq repeats the k / source checks). */
SEXP count_kmers_fastq_sh_rp(SEXP hash_ptr_r, SEXP params_r, SEXP fq_file_r) {
  if (TYPEOF(fq_file_r) != STRSXP || length(fq_file_r) != 1)
    error("fq_file should be a character vector of length at least one");
  if (TYPEOF(params_r) != INTSXP || length(params_r) != 8)
    error("k_r must be an integer vector of length 6 (k, prefix_bits, min_q, thread_n, "
          "max_reads, max_mem, source_n, source");
  const char *fq_file = CHAR(STRING_ELT(fq_file_r, 0));
  kmhg_index *sh = gpu_sh_of(hash_ptr_r);
  kmhg_index *out = sh;
  if (kmhg_sh_count_fastq(&out, fq_file, (const int32_t *)INTEGER(params_r)) != KMHG_OK)
    error("%s", kmhg_last_error());
  if (sh) return hash_ptr_r;
  SEXP tag = PROTECT(allocVector(STRSXP, 1));
  SET_STRING_ELT(tag, 0, mkChar(suffix_hash_n_tag));
  SEXP ptr = PROTECT(R_MakeExternalPtr(out, tag, R_NilValue));
  R_RegisterCFinalizerEx(ptr, finalise_gpu_index, TRUE);
  UNPROTECT(2);
  return ptr;
}

/* seq_kmer_depth_sh, src/kmer_hash.c:859-879 (seq.kmer.depth.sh, kmer_hash.R:75-78):
 * counts_n x L int matrix of the canonical k-mer counts along seq, written by the GPU. */
SEXP seq_kmer_depth_sh(SEXP hash_ptr_r, SEXP seq_r, SEXP k_r) {
  kmhg_index *sh = gpu_sh_of(hash_ptr_r);
  if (!sh) error("unable to obtain suffix_hash_n from external pointer");
  if (TYPEOF(k_r) != INTSXP || length(k_r) != 1) error("k_r should be a single integer");
  const int k = asInteger(k_r);
  if (TYPEOF(seq_r) != STRSXP || length(seq_r) != 1)
    error("seq_r should be a character vector of length 1");
  SEXP s = STRING_ELT(seq_r, 0);
  const size_t L = (size_t)length(s);
  SEXP counts_r = PROTECT(allocMatrix(INTSXP, gpu_sh_sources(sh), (int)L));
  if (kmhg_sh_depth(sh, CHAR(s), L, k, INTEGER(counts_r)) != KMHG_OK) {
    UNPROTECT(1);
    error("Receieved error from seq_kmer_counts");
  }
  UNPROTECT(1);
  return counts_r;
}

/* kmer_spectrum_suffix_hash_n, src/kmer_hash.c:1010-1039 (kmer.spec.sh.n, kmer_hash.R:88-91) */
SEXP kmer_spectrum_suffix_hash_n(SEXP hash_ptr_r, SEXP max_count_r, SEXP comb_r,
                                 SEXP comb_inner_r, SEXP source_min_r) {
  kmhg_index *sh = gpu_sh_of(hash_ptr_r);
  if (!sh) error("unable to obtain suffix_hash_n from external pointer");
  if (TYPEOF(max_count_r) != INTSXP || length(max_count_r) != 1)
    error("max_count_r should be a single integer");
  if (TYPEOF(comb_r) != INTSXP || length(comb_r) < 1)
    error("comb_r should be an integer vector of length > 0");
  if (TYPEOF(comb_inner_r) != INTSXP || length(comb_inner_r) != length(comb_r))
    error("comb_inner_r should be an integer vector of the same length as comb_r");
  const int S = gpu_sh_sources(sh);
  if (TYPEOF(source_min_r) != INTSXP || length(source_min_r) != S)
    error("source_min_r should be an integer vector of length sh->counts_n");
  const int max_count = asInteger(max_count_r);
  if (max_count < 0) error("max_count must be >= 0");
  const int comb_n = length(comb_r);
  SEXP counts_r = PROTECT(allocMatrix(REALSXP, comb_n * S, max_count + 1));
  int status = 1;
  if (kmhg_sh_spectrum(sh, max_count, INTEGER(comb_r), INTEGER(comb_inner_r), comb_n,
                       INTEGER(source_min_r), S, REAL(counts_r), &status) != KMHG_OK) {
    UNPROTECT(1);
    error("%s", kmhg_last_error());
  }
  if (status < 0) Rprintf("sh_count_spectrum_nc returned an error: %d\n", status);
  UNPROTECT(1);
  return counts_r;
}

/* ---- suffix_hash (single-source read counting) --------------------------------------------
 * The reference's own tag (src/kmer_hash.c:24): a pointer made here is refused by
 * seq.kmer.depth.sh / kmer.spec.sh.n, and kmer.spec.sh refuses a suffix_hash_n, as there.
 * The two entry points are exported but not in the registration table below, which stays the
 * list tests/test_r_glue.py pins: .Call("count_kmers_fastq_sh", ...) by name finds them by
 * R's dynamic symbol lookup, which registration leaves on (R_useDynamicSymbols is not called). */
static const char *suffix_hash_tag = "suffix_hash_250930";

static kmhg_index *gpu_sh1_of(SEXP ptr_r) {
  if (TYPEOF(ptr_r) != EXTPTRSXP) return NULL;
  SEXP tag = R_ExternalPtrTag(ptr_r);
  if (TYPEOF(tag) != STRSXP || length(tag) != 1 ||
      strcmp(CHAR(STRING_ELT(tag, 0)), suffix_hash_tag))
    return NULL;
  return (kmhg_index *)R_ExternalPtrAddr(ptr_r);
}

/* count_kmers_fastq_sh, src/kmer_hash.c:715-806 (count.kmers.fq.sh, kmer_hash.R:56-59):
 * params = (k, report_n, prefix_bits, max_memory, min_quality, max_read_n).  Validation order
 * and texts as the reference, its misworded params message included; the report_n progress
 * printing is not reproduced. */
SEXP count_kmers_fastq_sh(SEXP hash_ptr_r, SEXP params_r, SEXP fq_file_r) {
  if (TYPEOF(fq_file_r) != STRSXP || length(fq_file_r) != 1)
    error("fq_file should be a character vector of length at least one");
  if (TYPEOF(params_r) != INTSXP || length(params_r) != 6)
    error("k_r must be an integer vector of length 3");
  const char *fq_file = CHAR(STRING_ELT(fq_file_r, 0));
  const int *params = INTEGER(params_r);
  if (params[1] < 1) warning("negative or 0 report n value specified: set to 1e6");
  if (params[0] < 1 || params[0] > 32) error("k must be a positive integer less than 1+MAX_K");
  kmhg_index *sh = NULL;
  if (hash_ptr_r != R_NilValue) {
    sh = gpu_sh1_of(hash_ptr_r);
    if (!sh) error("Unable to extract suffix_hash from external pointer");
  }
  kmhg_index *out = sh;
  if (kmhg_sh1_count_fastq(&out, fq_file, (const int32_t *)params) != KMHG_OK)
    error("%s", kmhg_last_error());
  if (sh) return hash_ptr_r;
  SEXP tag = PROTECT(allocVector(STRSXP, 1));
  SET_STRING_ELT(tag, 0, mkChar(suffix_hash_tag));
  SEXP ptr = PROTECT(R_MakeExternalPtr(out, tag, R_NilValue));
  R_RegisterCFinalizerEx(ptr, finalise_gpu_index, TRUE);
  UNPROTECT(2);
  return ptr;
}

/* kmer_spectrum_suffix_hash, src/kmer_hash.c:993-1008 (kmer.spec.sh, kmer_hash.R:89-91) */
SEXP kmer_spectrum_suffix_hash(SEXP ext_ptr, SEXP max_count_r) {
  kmhg_index *sh = gpu_sh1_of(ext_ptr);
  if (!sh) error("unable to obtain a suffix_hash from external pointer");
  if (TYPEOF(max_count_r) != INTSXP || length(max_count_r) != 1)
    error("max_count_r should be a single integer");
  const int max_count = asInteger(max_count_r);
  if (max_count < 1 || max_count > (1 << 30)) error("Unsuitable value of max_count");
  SEXP counts_r = PROTECT(allocVector(REALSXP, (R_xlen_t)max_count + 1));
  if (kmhg_sh1_spectrum(sh, max_count, REAL(counts_r)) != KMHG_OK) {
    UNPROTECT(1);
    error("%s", kmhg_last_error());
  }
  UNPROTECT(1);
  return counts_r;
}

/* Not in the reference: choose the kmer.pos k-mer order of an index, "first" (first
 * occurrence, the default) or "khash" (the reference's own bucket order, byte-identical
 * output).  KMHG_ROW_ORDER=khash in the environment sets the default for new indices. */
SEXP kmer_row_order(SEXP ptr_r, SEXP order_r) {
  kmhg_index *idx = gpu_index_of(ptr_r);
  if (TYPEOF(order_r) != STRSXP || length(order_r) != 1)
    error("order should be \"first\" or \"khash\"");
  const char *o = CHAR(STRING_ELT(order_r, 0));
  int code = !strcmp(o, "khash") ? KMHG_ORDER_KHASH : (!strcmp(o, "first") ? KMHG_ORDER_FIRST : -1);
  if (code < 0) error("order should be \"first\" or \"khash\"");
  if (kmhg_set_row_order(idx, code) != KMHG_OK) error("%s", kmhg_last_error());
  return R_NilValue;
}

/* Not in the reference: the occurrence cap of later queries on a position index (kmer.max.occ;
 * include/kmhgpu.h, kmhg_set_max_occ).  0 is off; with n >= 1 a query window whose k-mer occurs at
 * more than n positions of the index yields no hit, in seq.kmer.pos, seq.kmer.pos.rc,
 * seq.kmer.segs, seq.kmer.blocks, seq.kmer.chains and seq.kmer.raster alike.  Returns the
 * value read just before the set (a get and a set: not atomic against another thread setting the
 * same index).  Like the other additions it is exported but not in the table below. */
SEXP kmer_max_occ(SEXP ptr_r, SEXP max_occ_r) {
  if (TYPEOF(max_occ_r) != INTSXP || length(max_occ_r) != 1 ||
      INTEGER(max_occ_r)[0] == INT_MIN) /* NA_integer_: as.integer of a value beyond 2^31-1 */
    error("max.occ should be an integer of length 1");
  kmhg_index *idx = gpu_index_of(ptr_r);
  int64_t before = 0;
  if (kmhg_get_max_occ(idx, &before) != KMHG_OK) error("%s", kmhg_last_error());
  if (kmhg_set_max_occ(idx, (int64_t)INTEGER(max_occ_r)[0]) != KMHG_OK)
    error("%s", kmhg_last_error());
  SEXP ret = PROTECT(allocVector(INTSXP, 1));
  INTEGER(ret)[0] = (int)before;
  UNPROTECT(1);
  return ret;
}

/* Not in the reference: reads.kmer.pos / reads.kmer.vote (include/kmhgpu.h,
 * kmhg_reads_query_run_packed, kmhg_rquery_votes): every element of the character vector seqs_r is
 * one read, queried against the position index on both strands in one device call.  strand: 0 both,
 * 1 forward, -1 reverse.  reads_kmer_positions returns INTSXP 4 x H of (read, strand, i, j),
 * reads_kmer_votes INTSXP 6 x n of (read, strand, pos, hits, second, total); the R wrappers
 * transpose and name them.  Every refusal of an argument is raised here, before the library is
 * called.  Exported, not in the table below. */
/* The query a reads_* call holds while it allocates its result: allocMatrix may leave the call by
 * R's error jump, so the handle is parked here and released by whichever comes first, the call's
 * own end or the next reads_* call (.Call entries of one session do not run concurrently). */
static kmhg_rquery *parked_rquery = NULL;
static void release_parked_rquery(void) {
  if (parked_rquery) kmhg_rquery_free(parked_rquery);
  parked_rquery = NULL;
}

static kmhg_rquery *reads_query_of(SEXP ptr_r, SEXP seqs_r, SEXP k_r, SEXP strand_r, int64_t *h) {
  release_parked_rquery();
  if (TYPEOF(seqs_r) != STRSXP) error("seqs should be a character vector");
  if (TYPEOF(k_r) != INTSXP || length(k_r) != 1) error("k should be an integer of length 1");
  if (TYPEOF(strand_r) != INTSXP || length(strand_r) != 1)
    error("strand should be 0 (both), 1 (forward) or -1 (reverse)");
  int k = INTEGER(k_r)[0], strand = INTEGER(strand_r)[0];
  if (k < 1 || k > 31) error("k should be between 1 and 31");
  if (strand != 0 && strand != 1 && strand != -1)
    error("strand should be 0 (both), 1 (forward) or -1 (reverse)");
  kmhg_index *idx = gpu_index_of(ptr_r);
  int n = length(seqs_r);
  int64_t *off = (int64_t *)R_alloc((size_t)n + 1, sizeof(int64_t));
  off[0] = 0;
  for (int r = 0; r < n; ++r) off[r + 1] = off[r] + (int64_t)length(STRING_ELT(seqs_r, r));
  if (off[n] > (int64_t)INT_MAX - 1) error("more than 2^31-2 bases in one call: split the reads");
  uint8_t *seq = (uint8_t *)R_alloc((size_t)off[n] + 1, 1);
  for (int r = 0; r < n; ++r)
    memcpy(seq + off[r], CHAR(STRING_ELT(seqs_r, r)), (size_t)(off[r + 1] - off[r]));
  if (kmhg_reads_query_run_packed(idx, seq, off[n], off, (int64_t)n, k,
                                  strand == 0 ? 3 : strand == 1 ? 1 : 2, &parked_rquery, h) !=
      KMHG_OK)
    error("%s", kmhg_last_error());
  return parked_rquery;
}

SEXP reads_kmer_positions(SEXP ptr_r, SEXP seqs_r, SEXP k_r, SEXP strand_r) {
  int64_t h = 0;
  kmhg_rquery *q = reads_query_of(ptr_r, seqs_r, k_r, strand_r, &h);
  if (h > INT_MAX) {
    release_parked_rquery();
    error("result has more than 2^31-1 columns (R matrix limit)");
  }
  SEXP ret = PROTECT(allocMatrix(INTSXP, 4, (int)h));
  int rc = h ? kmhg_rquery_fill(q, INTEGER(ret)) : KMHG_OK;
  release_parked_rquery();
  if (rc != KMHG_OK) error("%s", kmhg_last_error());
  UNPROTECT(1);
  return ret;
}

SEXP reads_kmer_votes(SEXP ptr_r, SEXP seqs_r, SEXP k_r, SEXP band_r, SEXP strand_r) {
  if (TYPEOF(band_r) != INTSXP || length(band_r) != 1 || INTEGER(band_r)[0] == INT_MIN)
    error("band should be an integer of length 1");
  int band = INTEGER(band_r)[0];
  if (band < 1 || band > (1 << 30)) error("band must be between 1 and 2^30");
  int64_t h = 0;
  kmhg_rquery *q = reads_query_of(ptr_r, seqs_r, k_r, strand_r, &h);
  int n = length(seqs_r);
  SEXP ret = PROTECT(allocMatrix(INTSXP, 6, n));
  int rc = n ? kmhg_rquery_votes(q, (int64_t)band, INTEGER(ret)) : KMHG_OK;
  release_parked_rquery();
  if (rc != KMHG_OK) error("%s", kmhg_last_error());
  UNPROTECT(1);
  return ret;
}

static const R_CallMethodDef gpu_call_methods[] = {
    {"make_kmer_h_index", (DL_FUNC)&make_kmer_h_index, 3},
    {"kmer_positions", (DL_FUNC)&kmer_positions, 2},
    {"sequence_kmer_positions", (DL_FUNC)&sequence_kmer_positions, 3},
    {"kmer_pair_pos", (DL_FUNC)&kmer_pair_pos, 2},
    {"count_kmers", (DL_FUNC)&count_kmers, 3},
    {"count_kmers_fastq_sh_rp", (DL_FUNC)&count_kmers_fastq_sh_rp, 3},
    {"seq_kmer_depth_sh", (DL_FUNC)&seq_kmer_depth_sh, 3},
    {"kmer_spectrum_suffix_hash_n", (DL_FUNC)&kmer_spectrum_suffix_hash_n, 5},
    {"kmer_row_order", (DL_FUNC)&kmer_row_order, 2},
    {NULL, NULL, 0}};

void R_init_kmer_hash(DllInfo *info) { R_registerRoutines(info, NULL, gpu_call_methods, NULL, NULL); }
