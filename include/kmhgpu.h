/*
 * kmhgpu.h -- C-ABI of the MI355X k-mer position index (libkmhgpu.so).
 *
 * Drop-in boundary for the hot path of lmjakt/kmer_hasheR.  Plain pointers and sizes only; no
 * torch or HIP types in the signatures (streams are passed as `void*` = hipStream_t, NULL = the
 * HIP null stream; host-pointer entry points run on a library-owned stream and return synced).  Every function returns KMHG_OK (0) or an error code; the message is
 * in kmhg_last_error() (thread-local).  Where the reference raises an R error() the message is
 * the reference's own text.
 *
 * Reference interfaces replaced (paths relative to the reference checkout):
 *   kmhg_build / kmhg_build_device
 *        <- .Call("make_kmer_h_index", seq, k, do.sort)      src/kmer_hash.c:506-540
 *           (+ seq_to_hash, src/kmer_pos.c:66-98; sort_kmer_pos, src/kmer_pos.c:21-33)
 *   kmhg_free
 *        <- finalise_khash_ptr (externalptr finaliser)       src/kmer_hash.c:56-66
 *           (+ clear_kmer_h, src/kmer_pos.c:10-19)
 *   kmhg_positions_size / kmhg_positions_fill / kmhg_positions_fill_device
 *        <- .Call("kmer_positions", ptr, opt.flag)           src/kmer_hash.c:1054-1147
 *           (+ kmer_seq decode, src/kmer_hash.c:123-133)
 *   kmhg_query_run / kmhg_query_run_device / kmhg_query_fill / kmhg_query_rows_device
 *        <- .Call("sequence_kmer_positions", ptr, seq, k)    src/kmer_hash.c:1151-1172
 *           (+ seq_kmer_positions, src/kmer_pos.c:110-136)
 *   kmhg_count / kmhg_count_device
 *        <- .Call("count_kmers", hash.ptr, params, seq)       src/kmer_hash.c:548-591
 *   kmhg_build_device_part / kmhg_part_info / kmhg_part_export
 *        <- the owner-computes partition of the reader pool  src/kmer_reader.c:28-39, 101-108
 *           (multi-GPU make.kmer.hash; no single reference entry point)
 *   kmhg_part_first_mask / kmhg_part_positions_size / kmhg_part_positions_fill_device /
 *   kmhg_merge_part_positions
 *        <- .Call("kmer_positions", ptr, opt.flag)           src/kmer_hash.c:1054-1147
 *           over that partition (src/kmer_reader.c:28-39), the parts never assembled
 *   KMHG_DEVICES=d0,d1,... (environment): kmhg_query_run splits seq.kmer.pos over those devices
 *           (index peer-copied once per device, rows copied straight into the caller's buffer)
 *   registration of the three symbols with arities 3/2/3    src/kmer_hash.c:1205-1224
 *           is done by the R glue (kmer_hasher_amd/R/kmer_hash_glue.c) over this ABI.
 *
 * Output layouts are the R matrices' column-major data, exactly what the reference memcpy's:
 *   pos      2 x N int32   (i, pos)      i = 1-based k-mer index, pos = 1-based window start
 *   pair.pos 3 x P int32   (i, x, y)     x < y, j-outer / k-inner inside a k-mer
 *   count    N_kmers int32
 *   kmer     N_kmers strings of k chars, each followed by a NUL (stride k+1)
 *   query    2 x H int32   (i, j)        i = 1-based END of the query window, j = index pos
 * K-mer order (the `i` labels): by default distinct k-mers ranked by first occurrence; the sets,
 * counts, position lists and pairs per k-mer equal the reference's, and seq.kmer.pos rows are
 * identical including order (DESIGN.md "Parity").  With KMHG_ORDER_KHASH (kmhg_set_row_order, or
 * KMHG_ROW_ORDER=khash in the environment when the index is built) kmer.pos is labelled in the
 * reference's own khash bucket order, i.e. byte-identical to its output.
 */
#ifndef KMHGPU_H
#define KMHGPU_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define KMHG_OK 0
#define KMHG_EINVAL 1     /* argument rejected (message = the reference's R error text) */
#define KMHG_ENOMEM 2     /* device or host allocation failed */
#define KMHG_EDEVICE 3    /* HIP runtime error */
#define KMHG_EOVERFLOW 4  /* result exceeds int32 / R matrix limits */

/* opt.flag bits of kmer.pos (src/kmer_hash.c:17; src/kmer_pos.h:8-12) */
#define KMHG_OPT_KMER 1u
#define KMHG_OPT_POS 2u
#define KMHG_OPT_PAIRS 4u
#define KMHG_OPT_COUNT 8u

/* kmer.pos k-mer (row) order */
#define KMHG_ORDER_FIRST 0   /* ranked by first occurrence (default) */
#define KMHG_ORDER_KHASH 1   /* the reference's khash 0.2.8 bucket order, src/kmer_hash.c:1096-1124 */

typedef struct kmhg_index kmhg_index;
typedef struct kmhg_query kmhg_query;

typedef struct {
  int32_t k;             /* index k-mer length */
  int32_t device;        /* HIP device ordinal holding the index */
  int64_t seq_len;       /* L */
  int64_t n_kmers;       /* distinct k-mers (kh_size) */
  int64_t n_positions;   /* windows indexed (rows of kmer.pos $pos) */
  int64_t n_pairs;       /* sum C(n,2) (rows of kmer.pos $pair.pos) */
  int64_t max_count;     /* largest position list */
  int64_t table_slots;   /* hash-table capacity */
  int64_t device_bytes;  /* device memory held by the index */
  int32_t sources;       /* counts index (count.kmers): source_n; 0 for a position index */
  int32_t kind;          /* 0 position index, 1 counts index, 2 suffix hash (canonical counts),
                            3 single suffix hash (count.kmers.fq.sh) */
  int64_t kmer_count;    /* khash_ptr.kmer_count: distinct k-mers added (both kinds) */
  int32_t build;         /* KMHG_BUILD_*: how the table was built (0 = imported / assembled) */
  int32_t fallback;      /* 1: a partitioned build was rebuilt with the global-atomic build (a
                            bucket's LDS table overflowed or its stream failed the order check) */
} kmhg_info;

/* kmhg_info.build */
#define KMHG_BUILD_GLOBAL 1              /* global-atomic insert (KMHG_BUILD=v1, or the fallback) */
#define KMHG_BUILD_PARTITIONED 2         /* radix partition + per-bucket LDS tables (default) */
#define KMHG_BUILD_PARTITIONED_BALLOT 3  /* the same with ballot ranks: the device failed the
                                            LDS lane-order self-check */

const char *kmhg_last_error(void);
int kmhg_version(void);

/* make.kmer.hash.  seq: host chars, L = its length (the sequence ends at L or at the first NUL,
 * as a C string does).  Errors: "k must be a positive integer less than 1+MAX_K",
 * "the length of the sequence must be at least k".  do_sort is accepted for API identity; the
 * engine always stores positions ascending, which is what sort_kmer_pos would produce. */
int kmhg_build(const char *seq, size_t L, int k, int do_sort, kmhg_index **out);
/* Same, for a device-resident sequence (no NULs assumed) on `stream`.  Asynchronous: it returns
 * once the build is queued, so back-to-back builds pipeline host and device work.  The first
 * call that reads the index (info, kmer.pos, a query, export, kmhg_index_wait) waits for it;
 * until then `d_seq` must stay valid and unmodified (the overflow fallback re-reads it).
 * kmhg_free of an index never used does not wait. */
int kmhg_build_device(const void *d_seq, size_t L, int k, int do_sort, void *stream,
                      kmhg_index **out);
/* Wait for an asynchronous build to finish (no-op for a finished index). */
int kmhg_index_wait(kmhg_index *idx);
int kmhg_free(kmhg_index *idx);
int kmhg_index_info(const kmhg_index *idx, kmhg_info *info);

/* Row order of later kmer.pos calls on this index (KMHG_ORDER_*).  The khash order is replayed
 * on the host from the distinct keys (src/khash.h:230-348 semantics), once per index. */
int kmhg_set_row_order(kmhg_index *idx, int order);
int kmhg_get_row_order(const kmhg_index *idx, int *order);
/* The occurrence cap of later queries on this position index, a setting like the row order.
 * 0 (the default) is off: every entry behaves and launches exactly as without it.  With
 * max_occ = n >= 1 a query window whose k-mer occurs at more than n positions of the index yields
 * no hit, as if those rows had been deleted from seq.kmer.pos's result before anything else looked
 * at it; a window with exactly n occurrences keeps all of them, and n = 1 keeps unique k-mers
 * only.  It applies to seq.kmer.pos and seq.kmer.pos.rc (kmhg_query_run*, their range, runs and
 * part entries, either strand, KMHG_DEVICES included -- a device's copy of the index takes this
 * index's value on every call), to seq.kmer.segs, seq.kmer.blocks and seq.kmer.chains on both of
 * their routes, and to seq.kmer.raster.  The hit totals the row-free entries return are the totals
 * after masking, and the 2^31-row checks apply to what remains.  kmer.pos, kmer.pairs, the entries
 * that take the caller's rows (kmhg_rows_*) and all counting entries ignore it.  Every query entry
 * reads the value once, when it is called.  The setting is not part of an exported image (an
 * imported index starts at 0) and kmhg_index_info does not report it.
 * Errors: "max.occ must be between 0 and 2^31-1"; "External pointer has incorrect tag" for a
 * canonical or suffix-hash index; "max.occ needs a position index" for a counts index.  A part of
 * an owner-computes build is accepted: a key's occurrences all live in its owner's part. */
int kmhg_set_max_occ(kmhg_index *idx, int64_t max_occ);
int kmhg_get_max_occ(const kmhg_index *idx, int64_t *max_occ);

/* make.kmer.hash.min (not in the reference): a position index of the (w,k)-minimizer windows of
 * the sequence alone, about 2 / (w + 1) of them on random input.  With Nw = L - k + 1 window
 * starts, h(s) the 64-bit mix of window s's k-mer code that the build takes its bucket from (a
 * bijection: equal h, equal k-mer) and a span any w consecutive window starts inside [1, Nw] that
 * the unsampled build would all index, window s is selected iff it is the leftmost minimum of h in
 * some span that contains it.  Windows in no span (fewer than w indexable windows in a row) are
 * never selected; w = 1 selects every indexable window and takes kmhg_build's own path, kernel
 * for kernel.  The index records its w (kmhg_get_sampling: 1 for every index of the other
 * entries, counts and suffix-hash indexes included).  kmer.pos and kmer.pairs read it like any
 * index and see only the selected positions.  A seq.kmer.pos-family query at the index's own k
 * applies the same rule to the QUERY sequence (for the rc entries to rc(seq), in rc coordinates,
 * N staying N) and returns exactly the rows (i, j) of the unsampled query with i selected in the
 * query and j selected in the indexed sequence, in the unsampled order; segments, blocks, chains
 * and the raster derive from those rows.  kmhg_set_max_occ applies on top (the intersection; a
 * k-mer's occurrences are counted in the sampled index, which holds its selected positions only).
 * The range entries (*_range, *_range_runs, forward and rc) select over the whole sequence of L
 * chars they are given and mask only the windows [w_begin, w_end): they read up to w - 1 windows
 * beyond the range on both sides.  A query at another k behaves as on an unsampled index.  Such
 * an index never takes the diagonal shortcut of the probe.
 * Errors: "w must be between 1 and 256"; "a sampled index needs k <= 31"; kmhg_build's own;
 * "a sampled index needs the partitioned build" where the global-atomic build is forced, and
 * KMHG_EOVERFLOW if a bucket overflowed (the fallback build does not sample);
 * "a sampled index is queried on its own device" for a KMHG_DEVICES query;
 * "index images do not carry a sampling" for kmhg_image_export.  kmhg_build_device_part has no
 * sampled form.  The device entry waits once on `stream` (the number selected sizes the table)
 * and is asynchronous after that, like kmhg_build_device. */
int kmhg_build_sampled(const char *seq, size_t L, int k, int w, int do_sort, kmhg_index **out);
int kmhg_build_sampled_device(const void *d_seq, size_t L, int k, int w, int do_sort,
                              void *stream, kmhg_index **out);
int kmhg_get_sampling(const kmhg_index *idx, int *w);
/* The selection itself.  Device: bit (s - 1) % 32 of d_mask_words[(s - 1) / 32] = window start s
 * of the strand (rc != 0: of rc(seq)) is selected; ceil(Nw / 32) words, every one written, bits
 * past Nw zero; *n_selected = their number.  Waits for `stream`.  Host (CPU only, the same rule
 * from the same header): mask[s - 1] = 0 / 1, Nw bytes.  Errors: the sampling entries' and
 * seq.kmer.pos's argument rules. */
int kmhg_minimizer_mask_device(const void *d_seq, size_t L, int k, int w, int rc,
                               uint32_t *d_mask_words, void *stream, int64_t *n_selected);
int kmhg_minimizer_mask(const char *seq, size_t L, int k, int w, int rc, uint8_t *mask);
/* The host replay itself: order[r] = index (into keys) of the r-th live khash bucket after
 * kh_put of the n distinct keys in the given order.  Host-only, no device work. */
int kmhg_khash_order(const uint64_t *keys, int64_t n, uint32_t *order);

/* kmer.pos, two-phase: sizes first so the caller (R's allocMatrix) can allocate, then fill.
 * Unset opt bits give 0 sizes and the corresponding pointers may be NULL. */
int kmhg_positions_size(kmhg_index *idx, uint32_t opt, int64_t *n_kmers, int64_t *n_pos_rows,
                        int64_t *n_pair_rows, int64_t *n_counts);
int kmhg_positions_fill(kmhg_index *idx, uint32_t opt, char *kmers, int32_t *pos,
                        int32_t *pairs, int32_t *counts);
int kmhg_positions_fill_device(kmhg_index *idx, uint32_t opt, char *d_kmers, int32_t *d_pos,
                               int32_t *d_pairs, int32_t *d_counts, void *stream);

/* seq.kmer.pos.  Errors: "the sequence should be longer than k and k should not be longer than
 * 31" (also for k < 1, where the reference's behaviour is undefined). */
int kmhg_query_run(kmhg_index *idx, const char *seq, size_t L, int k, kmhg_query **q,
                   int64_t *n_rows);
int kmhg_query_run_device(kmhg_index *idx, const void *d_seq, size_t L, int k, void *stream,
                          kmhg_query **q, int64_t *n_rows);
/* Windows [w_begin, w_end) (0-based window starts, w_end <= L - k + 1) of a device-resident
 * query: the unit of the multi-GPU query shard.  Window validity still sees the whole sequence
 * (the char before a window, the true sequence end), so consecutive ranges concatenate to the
 * unsharded result row for row. */
int kmhg_query_run_device_range(kmhg_index *idx, const void *d_seq, size_t L, int k,
                                int64_t w_begin, int64_t w_end, void *stream, kmhg_query **q,
                                int64_t *n_rows);
/* The same range query with its rows left as diagonal runs (the format of kmhg_rows_runs, the
 * sharded gather's): made from the query's per-window records, the rows are never written.
 * *n_runs >= 0: the query holds n_runs runs (kmhg_query_runs_device, 3 int32 each; rows
 * through kmhg_runs_expand); *n_runs = -1: runs would not be smaller and it holds the rows as
 * kmhg_query_run_device_range's do.  The rows / fill / copy entries refuse a runs query. */
int kmhg_query_run_device_range_runs(kmhg_index *idx, const void *d_seq, size_t L, int k,
                                     int64_t w_begin, int64_t w_end, void *stream,
                                     kmhg_query **q, int64_t *n_rows, int64_t *n_runs);
int kmhg_query_runs_device(kmhg_query *q, const int32_t **d_runs);   /* owned by q */
/* seq.kmer.pos.rc: the query's REVERSE COMPLEMENT against the index, made on the device from the
 * forward sequence (the dot plot's second strand: the reference's usage script calls
 * seq.kmer.pos(hash, reverseComplement(x), k), test.R:42-43, 49-52, 72-73, with the 2-bit rule
 * (v + 2) %% 4 of its rev.comp, test.R:31-36).  `seq` / `d_seq` is the sequence S as the forward
 * entries read it, of length L (kmhg_query_run_rc ends S at its first NUL or at L; the device
 * entries use L bytes); no reversed copy is made on the host or the device.  For p in [0, L)
 *   rc(S)[p] = 'N'                                   if S[L-1-p] is 'N' or 'n',
 *            = "ACTG"[((S[L-1-p] >> 1) & 3) ^ 2]     otherwise.
 * One deviation from rev.comp: it would turn an N into a C (it complements N's 2-bit code);
 * here an N stays an N and breaks windows on both strands.  Every other byte, ambiguity codes
 * included, is complemented by its 2-bit code as the reference encodes it (no IUPAC rule).
 * The result is exactly the reference's sequence_kmer_positions(index, rc(S), k)
 * (src/kmer_hash.c:1151-1172, src/kmer_pos.c:110-136): rows (i, j) ordered by i then j, i the
 * 1-based END of the window in rc(S) -- that window STARTS at forward position L - i + 1
 * (1-based) of S and is read leftwards on the opposite strand -- and j the index positions,
 * ascending.  Window validity is the reference's rule applied to rc(S), end-drop quirk included;
 * the quirk is not mirror-symmetric: a final N-free segment of rc(S) of exactly k chars is
 * dropped, which in S is an INITIAL segment of exactly k chars followed by N (or a whole
 * sequence of k chars).  Errors and their words are the forward entries'; the query k is
 * independent of the index k; a counts index is accepted and a part index refused as by the
 * forward whole-index entries.  w_begin / w_end are window starts in rc(S), and consecutive
 * ranges concatenate to the unsharded rc result row for row.  The kmhg_query is an ordinary
 * query handle.  KMHG_DEVICES is not honoured by kmhg_query_run_rc: it runs on the index's
 * device. */
int kmhg_query_run_rc(kmhg_index *idx, const char *seq, size_t L, int k, kmhg_query **q,
                      int64_t *n_rows);
int kmhg_query_run_rc_device_range(kmhg_index *idx, const void *d_seq, size_t L, int k,
                                   int64_t w_begin, int64_t w_end, void *stream, kmhg_query **q,
                                   int64_t *n_rows);
int kmhg_query_run_rc_device_range_runs(kmhg_index *idx, const void *d_seq, size_t L, int k,
                                        int64_t w_begin, int64_t w_end, void *stream,
                                        kmhg_query **q, int64_t *n_rows, int64_t *n_runs);
/* seq.kmer.pos over a PART of an owner-computes build (kmhg_build_device_part), without
 * assembling the parts: every window of the query is hashed and only the windows whose k-mer
 * this part owns are probed, so the rows are those windows' rows, in window order.  With one
 * such query per part (one per rank), kmhg_merge_part_rows on the root interleaves them into
 * exactly the unsharded seq.kmer.pos rows (src/kmer_pos.c:110-136 behind
 * src/kmer_hash.c:1151-1172; the partition is the reference reader pool's,
 * src/kmer_reader.c:28-39).  kmhg_query_tile_offsets writes the query's n_tiles + 1 per-tile row
 * offsets (tiles of 2048 windows; [n_tiles] = n_rows) to device memory on `stream`. */
int kmhg_query_run_device_part(kmhg_index *part, const void *d_seq, size_t L, int k,
                               void *stream, kmhg_query **q, int64_t *n_rows);
int kmhg_query_tile_offsets(kmhg_query *q, uint64_t *d_out, int64_t *n_tiles, void *stream);
/* The root's merge: n_parts segments of (i, j) rows in device memory, part r's at
 * d_rows + 2 * d_seg_base[r] int32, with its tile offsets at d_tile_off + r * (n_tiles + 1);
 * writes the sum of their rows to d_out ordered by window end i, then j, on `stream`. */
int kmhg_merge_part_rows(const void *d_rows, const uint64_t *d_seg_base,
                         const uint64_t *d_tile_off, int n_parts, int64_t n_tiles, int k,
                         int64_t w0, void *d_out, void *stream);
/* kmer.pos over the PARTS of an owner-computes build (kmhg_build_device_part), without assembling
 * them: .Call("kmer_positions", ptr, opt.flag), src/kmer_hash.c:1054-1147, of an index that
 * stays split over the ranks as the reference's reader pool splits its k-mers
 * (src/kmer_reader.c:28-39).  A k-mer's row label is its rank by first occurrence; every k-mer
 * lives in one part, so the parts' first positions are disjoint and only an L-bit mask has to
 * meet: each part marks its own (kmhg_part_first_mask), the caller ORs the masks (an all-reduce
 * SUM of the words: no bit is set twice), each part writes its rows labelled with their rows in
 * the whole result (kmhg_part_positions_fill_device), and the root places every part's segments
 * (kmhg_merge_part_positions).  The merged result is byte for byte kmhg_positions_fill_device of
 * the single-device index in KMHG_ORDER_FIRST.
 * Limits: position indexes only, first-occurrence order only.  KMHG_ORDER_KHASH on a part is
 * refused: the khash replay needs every key on one host, which is what not assembling avoids.
 * kmhg_positions_size / _fill / _fill_device on a part keep refusing ("must be assembled").
 * Errors: "not a part index" for any other index.
 *
 * kmhg_part_first_mask: d_mask <- ceil(L / 32) u32 words, bit (p - 1) & 31 of word (p - 1) >> 5
 *   set for the 1-based first position p of every k-mer the part holds (all zero for a part that
 *   owns no bucket).
 * kmhg_part_positions_size: the part's own distinct k-mers (always: the labels are always
 *   written), and its pos / pair rows for the set opt bits.  Needs no mask.
 * kmhg_part_positions_fill_device: d_global_mask = the OR of every part's mask.  Writes, in
 *   ascending label: d_labels[n_kmers] (always), and for the set opt bits d_counts[n_kmers],
 *   d_kmers (n_kmers strings, stride k + 1), d_pos (label, pos) rows, d_pairs (label, x, y) rows
 *   (j-outer / k-inner); pointers of unset bits may be NULL. */
int kmhg_part_first_mask(kmhg_index *part, uint32_t *d_mask, void *stream);
int kmhg_part_positions_size(kmhg_index *part, uint32_t opt, int64_t *n_kmers,
                             int64_t *n_pos_rows, int64_t *n_pair_rows);
int kmhg_part_positions_fill_device(kmhg_index *part, const uint32_t *d_global_mask, uint32_t opt,
                                    int32_t *d_labels, char *d_kmers, int32_t *d_pos,
                                    int32_t *d_pairs, int32_t *d_counts, void *stream);
/* The root's merge of n_parts such segments, all in device memory on `stream`'s device.  Host
 * arrays of n_parts entries: the parts' sizes (n_kmers; n_pos_rows / n_pair_rows for their opt
 * bits) and device pointers (a part without k-mers, or without rows of a kind, may pass NULL
 * there).  d_counts is read whenever opt has POS, PAIRS or COUNT -- the row offsets are scans of
 * the merged counts -- so the parts are filled with KMHG_OPT_COUNT added in that case.  Writes the
 * outputs of the set opt bits, sized by the sums of the parts' sizes: counts and strings placed
 * by label, each k-mer's row run copied to its offset.  KMHG_EOVERFLOW ("result has more than
 * 2^31-1 rows") when a sum exceeds int32. */
int kmhg_merge_part_positions(int n_parts, uint32_t opt, int k, const int64_t *n_kmers,
                              const int64_t *n_pos_rows, const int64_t *n_pair_rows,
                              const int32_t *const *d_labels, const int32_t *const *d_counts,
                              const char *const *d_kmers, const int32_t *const *d_pos,
                              const int32_t *const *d_pairs, char *d_out_kmers,
                              int32_t *d_out_pos, int32_t *d_out_pairs, int32_t *d_out_counts,
                              void *stream);
/* A device sequence as it crosses xGMI (C1 scatter / broadcast of the multi-GPU query and of
 * the owner-computes build): what the reference reads of a char -- its 2-bit code (c >> 1) & 3
 * and its N test, src/kmer_pos.c:81-83 -- as 16 chars per u32 code word and u16 N-flag word
 * (ceil(L / 16) of each; 6 B per 16 chars).  kmhg_seq_unpack writes chars [a, b) back ("ACTG"
 * by code, or 'N', which every entry point reads as the original) from the words held at
 * d_code / d_nbit starting with word `word0` (<= a / 16), on `stream`. */
int kmhg_seq_pack(const void *d_seq, int64_t L, uint32_t *d_code, uint16_t *d_nbit,
                  void *stream);
int kmhg_seq_unpack(const uint32_t *d_code, const uint16_t *d_nbit, int64_t word0, int64_t a,
                    int64_t b, void *d_seq, void *stream);
/* The sharded query's row gather format (src/kmer_pos.c:110-136's rows, moved between ranks):
 * n_rows (i, j) int32 rows in device memory as diagonal runs -- maximal stretches of rows
 * (i, j), (i + 1, j + 1), ... -- each run 3 int32 {its first row's index, i, j}.
 * kmhg_rows_runs counts the runs (*n_runs; it waits for `stream`) and writes them to d_runs when
 * *n_runs <= cap_runs (else nothing: the caller sends rows); kmhg_runs_expand writes the n_rows
 * rows back to d_rows on `stream`.  n_rows < 2^31. */
/* n_rows (i, j) rows in device memory into host memory (2 * n_rows int32, e.g. an R matrix or
 * one rank's slice of a node-shared matrix), as kmhg_query_fill copies a query's rows: from
 * 512 K rows on as diagonal runs over PCIe, expanded by host threads.  Synchronous. */
int kmhg_rows_to_host(const void *d_rows, int64_t n_rows, int32_t *rows, void *stream);
int kmhg_rows_runs(const void *d_rows, int64_t n_rows, void *d_runs, int64_t cap_runs,
                   int64_t *n_runs, void *stream);
int kmhg_runs_expand(const void *d_runs, int64_t n_runs, int64_t n_rows, void *d_rows,
                     void *stream);
int kmhg_query_fill(kmhg_query *q, int32_t *rows);               /* host, 2 * n_rows int32 */
int kmhg_query_rows_device(kmhg_query *q, const int32_t **d_rows); /* owned by q */
/* Device-to-device copy of the 2 x n_rows int32 rows into caller memory on `stream`. */
int kmhg_query_copy_device(kmhg_query *q, void *d_dst, void *stream);
int kmhg_query_free(kmhg_query *q);

/* seq.kmer.segs (not in the reference): a seq.kmer.pos result as maximal diagonal segments.
 * The rows R are the (i, j) int32 rows of sequence_kmer_positions (src/kmer_pos.c:110-136), with
 * i, j >= 1 and strictly ascending by (i, j), as every route of this library delivers them.  A
 * segment (i, j, len) is a maximal diagonal stretch of R:
 *   (i + t, j + t) is in R for 0 <= t < len;  (i - 1, j - 1) is not;  (i + len, j + len) is not.
 * len counts rows (windows): the exact match covers len + k - 1 bases.  The result is 3 x S int32
 * in R's column-major order, {i, j, len} per segment, ordered by (i, j) of the first row -- the
 * order of the start rows among R.  min_len >= 1 keeps the segments with len >= min_len, in the
 * same order.  The segments partition R: the min_len = 1 result, expanded and sorted by (i, j),
 * is R.  Membership is decided from the ROWS alone, never from sequence characters, so the
 * result is right for a query k that differs from the index k, for reverse-strand rows
 * (kmhg_query_run_rc), for merged multi-GPU rows and for kmer.pairs rows, with no window rule
 * restated.  The reference's author started on this and commented it out (offset_diagonals,
 * src/kmer_hash.c:414-486: "there is something to be said for a non-heuristic function for
 * identifying the structure of the underlying sequences"); the run format above (kmhg_rows_runs)
 * joins only rows adjacent in row order and so breaks at every window with several hits.
 *
 * kmhg_rows_segments: any such rows in device memory, n_rows < 2^31, on `stream`, which it
 * waits for; n_rows = 0 gives 0 segments and d_rows is not read.  kmhg_query_segments: the rows
 * of a query handle, on its device (a KMHG_DEVICES query is gathered there first, as by
 * kmhg_query_rows_device; a handle that holds runs is refused in that entry's words).  Errors,
 * KMHG_EINVAL: "min_len must be a positive integer"; "rows are not in ascending (i, j) order"
 * (also for a repeated row); "rows must have i, j >= 1".  The kmhg_segs handle owns the result:
 * kmhg_segs_device gives its device pointer (valid until kmhg_segs_free), kmhg_segs_copy_device
 * copies it into caller device memory on `stream`, kmhg_segs_fill into host memory (3 * n_segs
 * int32).  kmhg_segs_free(NULL) is a no-op.
 *
 * kmhg_segments_run_device: the row-free route.  The query (d_seq, L, k; rc != 0: its reverse
 * strand, as kmhg_query_run_rc) is probed as by kmhg_query_run_device, and the segments' first
 * and last rows are found straight from the per-window records: hit j of window s starts a
 * segment iff s is the first window, j == 1, or j - 1 is no hit of window s - 1, and ends one iff
 * s is the last window, j == 2^31 - 1, or j + 1 is no hit of window s + 1 -- the definition above
 * with each lookup confined to one neighbour window's hits.  No row is written and no buffer
 * grows with the number of hits, so *n_rows, the int64 hit total, may exceed 2^31 - 1 where
 * kmhg_rows_segments / kmhg_query_segments refuse ("bad row count").  The result is exactly what
 * kmhg_query_segments gives on the rows of the same query, byte for byte, wherever those are
 * accepted; *n_rows = 0 gives an empty handle and is no error.  Refusals, in this order,
 * KMHG_EINVAL: "null argument"; "min_len must be a positive integer"; the query entries' own for
 * k / L (KMHG_EOVERFLOW for L >= 2^31 - 1); a counts index made by the .sh route and a part
 * index in the query entries' words; any other index with sources: "segments need a position
 * index".  Then, once the totals are known: KMHG_EOVERFLOW "result has more than 2^31-1
 * segments".  Query k need not be the index k; KMHG_DEVICES is not honoured (the index's own
 * device, as the rc entries); there is no range variant.  Synchronous on `stream`.
 * kmhg_segments_run: the same from a host string (read as by kmhg_raster_run). */
typedef struct kmhg_segs kmhg_segs;
int kmhg_rows_segments(const void *d_rows, int64_t n_rows, int64_t min_len, void *stream,
                       kmhg_segs **out, int64_t *n_segs);
int kmhg_query_segments(kmhg_query *q, int64_t min_len, kmhg_segs **out, int64_t *n_segs);
int kmhg_segments_run_device(kmhg_index *idx, const void *d_seq, size_t L, int k, int rc,
                             int64_t min_len, void *stream, kmhg_segs **out, int64_t *n_segs,
                             int64_t *n_rows);
int kmhg_segments_run(kmhg_index *idx, const char *seq, size_t L, int k, int rc, int64_t min_len,
                      kmhg_segs **out, int64_t *n_segs, int64_t *n_rows);
int kmhg_segs_device(kmhg_segs *g, const int32_t **d_segs, int64_t *n_segs);
int kmhg_segs_copy_device(kmhg_segs *g, void *d_dst, void *stream);
int kmhg_segs_fill(kmhg_segs *g, int32_t *segs);                 /* host, 3 * n_segs int32 */
int kmhg_segs_free(kmhg_segs *g);

/* seq.kmer.blocks (not in the reference): the diagonal segments merged across small gaps.
 * Input: rows R as for seq.kmer.segs -- i, j >= 1, strictly ascending by (i, j), n_rows < 2^31 --
 * and three parameters, min_len >= 1, max_gap >= 0, min_hits >= 1.
 *  1. G = the maximal diagonal segments of R with len >= min_len: exactly the result of
 *     kmhg_rows_segments(..., min_len).
 *  2. On each diagonal d = j - i, G's segments are ordered by i.  For consecutive segments a, b
 *     of one diagonal, gap(a, b) = b.i - (a.i + a.len); segments are maximal, so it is >= 1.  A
 *     segment dropped by min_len does not take part: the gap between its kept neighbours spans it.
 *  3. A block is a maximal chain of consecutive kept segments of one diagonal in which every gap
 *     is <= max_gap.
 *  4. A block's record is four int32 {i, j, span, hits}: i, j are those of its first segment;
 *     span = last.i + last.len - i, the windows from its first row to its last inclusive (at most
 *     2^31 - 1); hits = the sum of len, the rows of R in the block.  span - hits is the sum of its
 *     gaps.
 *  5. Only blocks with hits >= min_hits are kept.
 *  6. Blocks are ordered by the (i, j) of their first row (first rows are distinct rows of R).
 * So max_gap = 0 gives the segments as (i, j, len, len); any max_gap >= 2^31 - 2 gives one block
 * per diagonal that has a kept segment; the hits of all blocks at min_hits = 1 sum to the len of
 * all kept segments; and raising max_gap only ever unions blocks.  With max_gap = k one isolated
 * substitution between two sequences, which removes k consecutive windows from a diagonal, is
 * bridged.  The result is 4 x B int32 in R's column-major order and the same bytes on every run.
 *
 * kmhg_rows_blocks / kmhg_query_blocks take their rows as kmhg_rows_segments /
 * kmhg_query_segments do (n_rows = 0 gives an empty handle and d_rows is not read; a KMHG_DEVICES
 * query is gathered first; a handle that holds runs is refused in kmhg_query_segments' words).
 * Refusals, KMHG_EINVAL, before any device work and in this order: "null argument"; "min_len must
 * be a positive integer"; "max_gap must not be negative"; "min_hits must be a positive integer";
 * "bad row count".  The row faults keep seq.kmer.segs' words.  min_len, max_gap or min_hits beyond
 * int32 are legal: they give an empty result, or "any gap".  The kmhg_blocks handle owns the
 * result as a kmhg_segs handle does (kmhg_blocks_fill: 4 * n_blocks int32);
 * kmhg_blocks_free(NULL) is a no-op.
 *
 * kmhg_blocks_run_device / kmhg_blocks_run: the row-free route, kmhg_segments_run_device's front
 * half followed by the same block passes: exactly what kmhg_query_blocks gives on the rows of the
 * same query, byte for byte, wherever those are accepted, and defined beyond 2^31 - 1 rows (a
 * block lies on one diagonal, so its hits stay below 2^31 whatever *n_rows, the hit total, is).
 * Refusals as kmhg_segments_run_device's, with the three parameter refusals above after "null
 * argument" and "blocks need a position index" for an index with sources. */
typedef struct kmhg_blocks kmhg_blocks;
int kmhg_rows_blocks(const void *d_rows, int64_t n_rows, int64_t min_len, int64_t max_gap,
                     int64_t min_hits, void *stream, kmhg_blocks **out, int64_t *n_blocks);
int kmhg_query_blocks(kmhg_query *q, int64_t min_len, int64_t max_gap, int64_t min_hits,
                      kmhg_blocks **out, int64_t *n_blocks);
int kmhg_blocks_run_device(kmhg_index *idx, const void *d_seq, size_t L, int k, int rc,
                           int64_t min_len, int64_t max_gap, int64_t min_hits, void *stream,
                           kmhg_blocks **out, int64_t *n_blocks, int64_t *n_rows);
int kmhg_blocks_run(kmhg_index *idx, const char *seq, size_t L, int k, int rc, int64_t min_len,
                    int64_t max_gap, int64_t min_hits, kmhg_blocks **out, int64_t *n_blocks,
                    int64_t *n_rows);
int kmhg_blocks_device(kmhg_blocks *b, const int32_t **d_blocks, int64_t *n_blocks);
int kmhg_blocks_copy_device(kmhg_blocks *b, void *d_dst, void *stream);
int kmhg_blocks_fill(kmhg_blocks *b, int32_t *blocks);           /* host, 4 * n_blocks int32 */
int kmhg_blocks_free(kmhg_blocks *b);

/* seq.kmer.chains (not in the reference): the blocks linked across diagonals into chains.  A
 * substitution stays on its diagonal and seq.kmer.blocks bridges it; an indel shifts the diagonal
 * and splits an alignment into blocks, which this step joins again.
 * Input: B blocks {i, j, span, hits} as seq.kmer.blocks returns them, in strictly ascending (i, j)
 * order -- the index b = 0 .. B - 1 is that order -- and three parameters, max_dist >= 0,
 * max_drift >= 0, min_hits >= 1.  For block b, ei = i + span - 1 and ej = j + span - 1 are its last
 * row.
 *  1. Candidates.  a may precede b when, with gi = i_b - ei_a - 1 and gj = j_b - ej_a - 1:
 *     gi >= 0 and gj >= 0 (the blocks do not overlap in either coordinate);
 *     max(gi, gj) <= max_dist; and |gj - gi| <= max_drift (|gj - gi| is the diagonal shift).
 *  2. Cost.  cost(a, b) = gi + gj, below 2^32.  Keys are the u64 cost << 32 | index.
 *  3. Predecessor.  pred(b) is the candidate a with the smallest key cost(a, b) << 32 | a; none
 *     if b has no candidate.
 *  4. Child.  Among all b with pred(b) = a, child(a) is the one with the smallest key
 *     cost(a, b) << 32 | b.
 *  5. Links.  Link a -> b exists iff pred(b) = a and child(a) = b.  Every block then has at most
 *     one link in and at most one link out; the links form disjoint paths, and those paths are the
 *     chains.  A block that lost the contest for its predecessor starts a chain of its own: it
 *     does not fall back to a second choice.
 *  6. A chain's record is six int32 {i, j, i.end, j.end, hits, blocks}: i, j of its first block;
 *     i.end, j.end the ei, ej of its last block; hits the sum of its blocks' hits (a chain's blocks
 *     are disjoint in i, so the sum stays below 2^31); blocks the count of its blocks.
 *  7. Chains with hits >= min_hits are kept, ordered by the (i, j) of their first block.
 *  8. Membership.  chain[b] is the 1-based index of block b's chain among the kept chains, 0 if
 *     that chain was dropped: what lets a caller draw a chain as a polyline.
 * So max_dist = 0 gives every block as its own chain {i, j, ei, ej, hits, 1} (two blocks with
 * gi = gj = 0 would be one block); max_drift = 0 with max_dist = D >= max_gap reproduces
 * seq.kmer.blocks(max_gap = D) on the same segments, {i, j, i.end - i + 1, hits} being those
 * blocks' {i, j, span, hits}; at min_hits = 1 the chains' hits sum to the blocks' hits and their
 * block counts to B.  This is greedy nearest-neighbour chaining, not the optimal-score dynamic
 * program of minimap2.  The result is 6 x C int32 in R's column-major order plus B int32, and the
 * same bytes on every run: every reduction is an integer minimum or sum.
 *
 * kmhg_blocks_chains chains any such blocks in device memory (16-byte aligned), on `stream`, which
 * it waits for.  Refusals, KMHG_EINVAL, before any device work and in this order: "null argument"
 * (out); "max_dist must not be negative"; "max_drift must not be negative"; "min_hits must be a
 * positive integer"; "bad block count" (n_blocks < 0 or > 2^31 - 1); "null argument" (d_blocks
 * with n_blocks > 0); "blocks must be 16-byte aligned" (d_blocks, whose records are read as one
 * 16-byte load each).  max_dist and max_drift beyond int32 are legal and mean "any"; a min_hits
 * beyond int32 keeps no chain.  Then, from the device: "blocks are not in ascending (i, j) order"
 * (also for a repeated block); "blocks must have i, j >= 1, 1 <= hits <= span and ends within
 * 2^31 - 1".  n_blocks = 0 gives an empty handle and d_blocks is not read.
 *
 * kmhg_chains_run_device / kmhg_chains_run: the query (as kmhg_blocks_run_device /
 * kmhg_blocks_run name it) to chains in one call.  Its blocks are those of kmhg_query_blocks on
 * the query's rows (row_free = 0) or of kmhg_blocks_run_device (row_free != 0), with min_len and
 * max_gap as given and every block kept (min_hits applies to the chains); they stay in the handle,
 * where chain[b] refers to them.  Refusals as those entries', with "max_dist must not be negative",
 * "max_drift must not be negative" after max_gap's.  *n_rows <- the hit total.  KMHG_DEVICES is
 * not honoured.
 *
 * The kmhg_chains handle owns the result.  kmhg_chains_device gives the device pointers (valid
 * until kmhg_chains_free): the chains, chain[] (d_member) and the blocks (d_blocks: NULL from
 * kmhg_blocks_chains, whose blocks are the caller's); every output but d_chains is optional.
 * kmhg_chains_copy_device copies the chains (6 * n_chains int32), chain[] (n_blocks int32) and,
 * where d_blocks is not NULL, the handle's blocks into caller device memory on `stream`;
 * kmhg_chains_fill the chains into host memory;
 * kmhg_chains_member_fill chain[] and, where `blocks` is not NULL, the handle's blocks (4 *
 * n_blocks int32; "the handle holds no blocks" after kmhg_blocks_chains).
 * kmhg_chains_free(NULL) is a no-op. */
typedef struct kmhg_chains kmhg_chains;
int kmhg_blocks_chains(const void *d_blocks, int64_t n_blocks, int64_t max_dist, int64_t max_drift,
                       int64_t min_hits, void *stream, kmhg_chains **out, int64_t *n_chains);
int kmhg_chains_run_device(kmhg_index *idx, const void *d_seq, size_t L, int k, int rc,
                           int row_free, int64_t min_len, int64_t max_gap, int64_t max_dist,
                           int64_t max_drift, int64_t min_hits, void *stream, kmhg_chains **out,
                           int64_t *n_chains, int64_t *n_blocks, int64_t *n_rows);
int kmhg_chains_run(kmhg_index *idx, const char *seq, size_t L, int k, int rc, int row_free,
                    int64_t min_len, int64_t max_gap, int64_t max_dist, int64_t max_drift,
                    int64_t min_hits, kmhg_chains **out, int64_t *n_chains, int64_t *n_blocks,
                    int64_t *n_rows);
int kmhg_chains_device(kmhg_chains *c, const int32_t **d_chains, int64_t *n_chains,
                       const int32_t **d_member, const int32_t **d_blocks, int64_t *n_blocks);
int kmhg_chains_copy_device(kmhg_chains *c, void *d_chains, void *d_member, void *d_blocks,
                            void *stream);
int kmhg_chains_fill(kmhg_chains *c, int32_t *chains);           /* host, 6 * n_chains int32 */
int kmhg_chains_member_fill(kmhg_chains *c, int32_t *member, int32_t *blocks);
int kmhg_chains_free(kmhg_chains *c);

/* seq.kmer.raster (not in the reference): the dot plot as a binned count matrix, the one product
 * whose size does not grow with the number of hits.  The rows R are (i, j) int32 rows as for
 * seq.kmer.segs.  A frame is six int64 {i_lo, j_lo, bin_i, bin_j, n_i, n_j} with
 *   i_lo, j_lo >= 1;  bin_i, bin_j >= 1;  n_i, n_j >= 1;  n_i * n_j <= 2^26 cells;
 *   i_lo + n_i * bin_i - 1 <= 2^31 - 1 and j_lo + n_j * bin_j - 1 <= 2^31 - 1.
 * The result is n_i * n_j uint32 counts, cell (bi, bj) at index bi + n_i * bj (R's column-major
 * order of an n_i x n_j matrix):
 *   M[bi, bj] = #{ (i, j) in R : i_lo <= i, (i - i_lo) / bin_i == bi < n_i,
 *                                j_lo <= j, (j - j_lo) / bin_j == bj < n_j }
 * with integer division.  Rows outside the frame are not counted and are no error.  Integer adds
 * commute, so the result is the same bytes on every run.
 * Overflow rule: rows are distinct, so a cell holds at most min(H, bin_i * bin_j) of H rows; the
 * entries refuse with KMHG_EOVERFLOW "a raster cell could exceed 2^32-1 rows" only when
 * bin_i * bin_j >= 2^32 and H >= 2^32, and nothing saturates otherwise.
 *
 * All entries write into caller device memory d_out (n_i * n_j uint32) on `stream` and zero it
 * themselves.
 * kmhg_rows_raster: any n_rows < 2^31 rows in device memory -- rc rows, kmer.pairs rows, merged
 * multi-GPU rows -- in ANY order: unlike segments the rows need not be sorted, there is no order
 * check and no i, j >= 1 check (such rows lie outside every frame).  n_rows = 0 gives zeros and
 * d_rows is not read.  Asynchronous on `stream`.
 * kmhg_query_raster: the rows of a query handle, on its device (a KMHG_DEVICES query is gathered
 * there first; a handle that holds runs is refused in kmhg_query_segments' words).
 * kmhg_raster_run_device: the row-free route.  The query (d_seq, L, k; rc != 0: its reverse
 * strand, as kmhg_query_run_rc) is probed as by kmhg_query_run_device and every hit is added into
 * its cell straight from the per-window records: no row is written, so *n_rows, the int64 hit
 * total, may exceed 2^31 - 1 where the query entries refuse.  It gives exactly kmhg_rows_raster of
 * the rows kmhg_query_run[_rc] would deliver wherever those exist.  The query entries' refusals
 * hold in their words (k / L, a counts index, a part index); query k need not be the index k;
 * KMHG_DEVICES is not honoured (the index's own device, as the rc entries).  Synchronous.
 * kmhg_raster_run: the same from a host string into a host buffer `out` (n_i * n_j uint32).
 * Refusals, KMHG_EINVAL, before any device work and in this order: "null argument"; "bin widths
 * must be positive integers"; "bin counts must be positive integers"; "a raster has at most 2^26
 * cells"; "the frame must lie within 1..2^31-1 on both axes"; then "bad row count" (the rows
 * entry) or the query entries' own. */
int kmhg_rows_raster(const void *d_rows, int64_t n_rows, const int64_t frame[6], void *d_out,
                     void *stream);
int kmhg_query_raster(kmhg_query *q, const int64_t frame[6], void *d_out, void *stream);
int kmhg_raster_run_device(kmhg_index *idx, const void *d_seq, size_t L, int k, int rc,
                           const int64_t frame[6], void *d_out, void *stream, int64_t *n_rows);
int kmhg_raster_run(kmhg_index *idx, const char *seq, size_t L, int k, int rc,
                    const int64_t frame[6], uint32_t *out, int64_t *n_rows);

/* kmer.pairs <- .Call("kmer_pair_pos", ptr_a, ptr_b)           src/kmer_hash.c:1174-1203
 * Rows (a, b) = (position in index a, position in index b) for every k-mer both indices hold:
 * a's k-mers in a's kmer.pos row order (kmhg_set_row_order), a's positions outer, b's inner;
 * the result is a query handle holding 2 x n_rows int32, read like a seq.kmer.pos result.
 * Defined where the reference is broken: only a's live k-mers are visited (the reference reads
 * empty buckets and calls kh_exist(b, kh_end(b)), src/kmer_hash.c:1182-1185; test.R:330 "This
 * crashes"), and both indices must have the same k ("the two indices must have the same k").
 * Either index may be a counts index: its count vectors are read where a position index has
 * positions (zeros included), as kmer.pos reads them.
 * Refusals, KMHG_EINVAL, in this order: "null argument"; "External pointer has incorrect tag"
 * (a suffix hash as a or b); "a part index must be assembled before it is read" (a part of an
 * owner-computes build as a or b, refused before its build is waited for); "the two indices
 * must have the same k"; "the two indices must be on the same device".  More than 2^31-1 rows
 * are not refused here: n_rows is exact and the handle holds every row on the device; the host
 * matrix (kmer.pairs) is what refuses them.
 * kmhg_pairs_run is synchronous on the library's stream.  kmhg_pairs_run_device runs on `stream`
 * and does not synchronise it: n_rows is final when it returns, the rows are complete in stream
 * order (the caller synchronises `stream` before reading them from another stream or the host). */
int kmhg_pairs_run(kmhg_index *a, kmhg_index *b, kmhg_query **q, int64_t *n_rows);
int kmhg_pairs_run_device(kmhg_index *a, kmhg_index *b, void *stream, kmhg_query **q,
                          int64_t *n_rows);

/* count.kmers <- .Call("count_kmers", hash.ptr, c(k, source, source_n), seq)
 *                                                            src/kmer_hash.c:548-591
 *        (+ seq_to_counts :220-251, kmer_count_insert :185-208)
 * Per-source k-mer counts: every valid window (the window walk of make.kmer.hash) of every
 * sequence adds one to entry `source` of its k-mer's vector of source_n ints.  *idx == NULL
 * makes a new counts index, else the counts are added to *idx (same k and source_n).  Sequences
 * of length <= k are skipped; windows never span two sequences.  A negative source counts
 * nothing (the reference warns for every window).  Errors, in the reference's order and words:
 * "seq_r should be a character vector of length at least one", "k must be a positive integer
 * less than 1+MAX_K", "source_n must be larger than 1 and larger than source", "mismatch between
 * specified k and that given in the external pointer"; and, where the reference would write
 * out of bounds, a position index or a different source_n is refused.
 * A counts index reads like a position index whose "positions" are the count vectors, as the
 * reference's kmer_positions / sequence_kmer_positions read them: kmer.pos gives count = source_n
 * per k-mer and pos rows (i, count_s) for s = 0..source_n-1, seq.kmer.pos rows (i, count_s);
 * k-mers are ranked by first insertion, or in khash order (kmhg_set_row_order). */
int kmhg_count(kmhg_index **idx, const char *const *seqs, const size_t *lens, int64_t n_seqs,
               int k, int source, int source_n);
/* One device-resident sequence on `stream` (synchronous). */
int kmhg_count_device(kmhg_index **idx, const void *d_seq, size_t L, int k, int source,
                      int source_n, void *stream);

/* ---- read counting: the suffix_hash_n path (SURVEY.md §8 f next-4, depth half) -------------
 * A suffix hash is a counts index of CANONICAL k-mers (min of forward and reverse complement,
 * info.kind = 2, info.sources = counts_n), the reference's suffix_hash_n (src/suffix_hash.c).
 *
 * count.kmers.fq.sh.rp <- .Call("count_kmers_fastq_sh_rp", hash.ptr, params, fq.file)
 *                                                       src/kmer_hash.c:810-857
 *        (+ init_kmer_reader_pool(_sh) / kmer_reader_read src/kmer_reader.c:41-147, the k-mer
 *         iterator src/kmer_util.c:64-162, sh_n_add_kmer src/suffix_hash.c:179-285)
 * params = (k, prefix_bits, min_q, thread_n, max_reads, max_mem, source_n, source).  Reads the
 * FASTA/FASTQ file (plain or gzip) as the reference's kseq does, the first max_reads records
 * (negative: all), skips records of length <= k, and adds one to entry `source` of every
 * canonical k-mer the quality iterator accepts (threshold q_to_ll['!' + min_q]; FASTA records
 * only break at N).  *sh == NULL makes a new suffix hash of source_n counts; into an existing one
 * a different k or a source >= its counts_n prints the reference's message and counts nothing.
 * prefix_bits, thread_n and max_mem do not change the counts.  Errors (reference order and
 * words): "k must be a positive integer less than 1+MAX_K", "Source_n must be in the range
 * 1 - 4", "source_i must be less than source_n"; deviations on the reference's undefined paths:
 * k = 32 and (k < 16, prefix_bits > 2k) are refused. */
int kmhg_sh_count_fastq(kmhg_index **sh, const char *path, const int32_t params[8]);

/* The host reader alone (kseq semantics): records up to max_reads, those longer than k kept,
 * packed as bases / qualities (0 for FASTA records) / offsets[n+1] / has_qual[n]. */
typedef struct kmhg_reads kmhg_reads;
int kmhg_fastx_read(const char *path, int64_t max_reads, int k, kmhg_reads **out);
int kmhg_reads_info(const kmhg_reads *r, int64_t *n_records, int64_t *n_reads, int64_t *n_bases);
int kmhg_reads_copy(const kmhg_reads *r, uint8_t *seq, uint8_t *qual, int64_t *offsets,
                    uint8_t *has_qual);
int kmhg_reads_free(kmhg_reads *r);
/* Count reads already read (same params as kmhg_sh_count_fastq; max_reads is not applied). */
int kmhg_sh_count_reads(kmhg_index **sh, const kmhg_reads *r, const int32_t params[8]);
/* Device-resident packed reads on `stream`: d_seq / d_qual 16-byte aligned with >= 16 readable
 * bytes past the last read, d_offsets[n_reads + 1] (int64, absolute: d_offsets[0] need not be
 * 0), d_has_qual[n_reads].  Every record is walked as given, down to length 0: the <= k filter
 * belongs to the file reader, so a record of exactly k bases the iterator accepts counts once. */
int kmhg_sh_count_reads_device(kmhg_index **sh, const void *d_seq, const void *d_qual,
                               const int64_t *d_offsets, const uint8_t *d_has_qual,
                               int64_t n_reads, const int32_t params[8], void *stream);

/* Diagnostics of the last batch counted into a suffix hash (no reference counterpart): the HLL
 * estimate of its distinct canonical k-mers, the bucket spread its count-only build chose
 * (stream entries per LDS sub-table / 1024), and the path taken: 1 = built at that spread,
 * 2 = a sub-table overflowed and the batch was rebuilt at spread 1, 3 = global find-or-insert. */
int kmhg_sh_last_batch(const kmhg_index *sh, double *distinct_est, int *spread, int *path);

/* seq.kmer.depth.sh <- .Call("seq_kmer_depth_sh", hash.ptr, seq, k)  src/kmer_hash.c:859-879
 *        (+ seq_kmer_counts src/kmer_reader.c:155-193)
 * counts = counts_n x L int32 (R column-major): the counts of the canonical k-mer the reference's
 * walk writes at each position (its write lands at window start - 1 in normal flow, at the start
 * for an init window; see kmhg_sh.hip), zeros for k-mers absent from the hash, INT_MIN (NA)
 * where nothing is written.  Errors: "unable to obtain suffix_hash_n from external pointer",
 * "Receieved error from seq_kmer_counts" (k differs from the hash's); L < k writes nothing at
 * L - k (the reference writes before its buffer). */
int kmhg_sh_depth(kmhg_index *sh, const char *seq, size_t L, int k, int32_t *counts);
int kmhg_sh_depth_device(kmhg_index *sh, const void *d_seq, size_t L, int k, int32_t *d_counts,
                         void *stream);

/* kmer.spec.sh.n <- .Call("kmer_spectrum_suffix_hash_n", ptr, max.count, comb, comb.inner,
 *                          source.min)          src/kmer_hash.c:1010-1039
 *        (+ sh_count_spectrum_nc src/suffix_hash.c:338-421)
 * counts = (comb_n * counts_n) x (max_count + 1) doubles (R column-major).  *status = 1, or the
 * reference's code -3 (comb_inner not 0/1) / -4 (comb >= 2^counts_n) with all counts zero. */
int kmhg_sh_spectrum(kmhg_index *sh, int max_count, const int32_t *comb,
                     const int32_t *comb_inner, int comb_n, const int32_t *source_min,
                     int n_source_min, double *counts, int *status);

/* ---- single-source read counting: the suffix_hash path -------------------------------------
 * count.kmers.fq.sh <- .Call("count_kmers_fastq_sh", hash.ptr, params, fq.file)
 *                                                       src/kmer_hash.c:715-806
 *        (+ seq_to_counts_sh src/kmer_hash.c:296-332, init_kmer_qual_2 / skip_n_qual
 *         src/kmer_util.c:10-14 and 35-53, sh_add_kmer src/suffix_hash.c:66-97)
 * params = (k, report_n, prefix_bits, max_memory_GiB, min_quality, max_read_n).  The result is a
 * SINGLE suffix hash: one count per canonical k-mer (info.kind = 3, info.sources = 1), the
 * reference's suffix_hash.  It is a different pointer kind from the suffix_hash_n above, as the
 * reference's tags keep them: kmhg_sh_depth*, kmhg_sh_spectrum and kmhg_sh_count_* refuse a
 * kind-3 index ("unable to obtain suffix_hash_n from external pointer"), kmhg_sh1_* refuse a
 * kind-2 one; kmhg_counts_export, kmhg_index_info and kmhg_free take both.
 *
 * The walk is not the .rp iterator.  With mq = (char)(min_quality + '!') and C char comparisons
 * a base is bad when it is N/n or qual < mq, weak when qual == mq, good when qual > mq (FASTA
 * records: only N is bad, nothing is weak; a NUL ends the record).  An init needs k consecutive
 * non-bad bases (weak ones accepted) and restarts after a bad run; a successful init whose window
 * ends exactly at the record's end counts nothing; otherwise its window is counted and every
 * following GOOD base counts the window ending on it; a weak or bad base stops the roll, a weak
 * one becoming the first base of the next init.  The first max_read_n records are taken ((size_t)
 * of the int: negative = all, 0 = none), records of length <= k skipped.  report_n (progress
 * printing, not reproduced), prefix_bits and max_memory do not change the counts.  A file mixing
 * FASTA and FASTQ records is read as the .rp entry reads it: a record without a quality string
 * gets no quality test, wherever it stands (the reference hands such a record the previous
 * record's stale kseq quality buffer).
 *
 * Errors (reference words): "k must be a positive integer less than 1+MAX_K"; *sh not a single
 * suffix hash: "Unable to extract suffix_hash from external pointer".  Deviations, all on paths
 * where the reference's behaviour is undefined:
 *   - suffix bits = 2k - prefix_bits outside 0 .. 32 is refused (the reference truncates the
 *     suffix to 32 bits and mis-sizes its prefix array, src/suffix_hash.c:20-26, 70, 84);
 *   - k = 32 is refused, as for the .rp entry;
 *   - a max_memory too small for the prefix array (8 B << prefix_bits) is refused (the reference
 *     dereferences its NULL prefix array);
 *   - adding to an existing single suffix hash with a different k is refused (the reference keeps
 *     no k and would mask the new k-mers into the old key space).
 * The reference's third reader family, count.kmers.fq / kmer.spec.kt (kmer_tree), is not
 * provided: its result depends on a memory cap that stops counting in mid-file. */
int kmhg_sh1_count_fastq(kmhg_index **sh, const char *path, const int32_t params[6]);
/* Reads already read (max_read_n is not applied) and device-resident packed reads, with the
 * buffer contract of kmhg_sh_count_reads_device.  Records are routed by has_qual: those with
 * qualities to a lane-per-read walk, those without to a position-parallel kernel.  The device
 * entry walks every record as given: the <= k filter belongs to the reader, and this walk counts
 * nothing in a record of length <= k anyway (its only init window ends the record). */
int kmhg_sh1_count_reads(kmhg_index **sh, const kmhg_reads *r, const int32_t params[6]);
int kmhg_sh1_count_reads_device(kmhg_index **sh, const void *d_seq, const void *d_qual,
                                const int64_t *d_offsets, const uint8_t *d_has_qual,
                                int64_t n_reads, const int32_t params[6], void *stream);
/* kmer.spec.sh <- .Call("kmer_spectrum_suffix_hash", ptr, max.count)   src/kmer_hash.c:993-1008
 *        (+ sh_count_spectrum src/suffix_hash.c:112-129)
 * counts = max_count + 1 doubles: counts[min(count, max_count)] += 1 per distinct k-mer (entry 0
 * stays 0).  Errors: "unable to obtain a suffix_hash from external pointer" (not kind 3),
 * "Unsuitable value of max_count" (outside 1 .. 2^30). */
int kmhg_sh1_spectrum(kmhg_index *sh, int max_count, double *counts);

/* reads.kmer.pos / reads.kmer.vote (no reference counterpart): a batch of packed reads queried
 * against a position index on both strands in one call.
 *
 * The reads are packed as kmhg_reads_copy packs them: seq = the n_bases bases of all reads, off =
 * int64[n_reads + 1] with off[0] = 0, non-decreasing, off[n_reads] = n_bases; read r (1-based) is
 * seq[off[r - 1], off[r]).  strands: 1 forward, 2 reverse, 3 both.  1 <= k <= 31; k need not be
 * the index's.
 *
 * The result is H rows of four int32 (read, strand, i, j): the rows with read = r and strand = +1
 * are exactly those of seq.kmer.pos(idx, read_r, k) (kmhg_query_run), the rows with strand = -1
 * exactly those of seq.kmer.pos.rc(idx, read_r, k) (kmhg_query_run_rc: i in rc(read_r)'s
 * coordinates), ordered by read, forward before reverse, then (i, j).  Every rule of the single
 * query -- N, ambiguity codes, lowercase, the dropped end window -- applies to each read as if it
 * were the whole sequence, and the index's occurrence cap (kmhg_set_max_occ) applies.  A read of at
 * most k bases has no row; that is no error.  The bytes are the same on every run.
 *
 * Refused: k outside 1 .. 31 or strands outside 1 .. 3 (KMHG_EINVAL); a counts index; a
 * minimizer-sampled index queried at its own k (per-read minimizer selection is a follow-up);
 * more than 2^31 - 2 bases or 2^31 - 1 reads in one call (KMHG_EOVERFLOW); bases without a read
 * (n_reads = 0, n_bases > 0: KMHG_EINVAL, before any launch); offsets that break the
 * rule above (KMHG_EINVAL: the host entries look before anything is copied, the device entry
 * checks on the device and reads nothing outside d_seq[0, n_bases) and d_off[0 .. n_reads]
 * whatever d_off holds); kmhg_rquery_fill of more than 2^31 - 1 rows (KMHG_EOVERFLOW).
 *
 * kmhg_reads_query_run_device runs on `stream` and waits for it once (the row total sizes the
 * result); the other two copy the reads up and run on the library's stream. */
typedef struct kmhg_rquery kmhg_rquery;
int kmhg_reads_query_run_device(kmhg_index *idx, const void *d_seq, int64_t n_bases,
                                const int64_t *d_off, int64_t n_reads, int k, int strands,
                                void *stream, kmhg_rquery **q, int64_t *n_rows);
int kmhg_reads_query_run_packed(kmhg_index *idx, const uint8_t *seq, int64_t n_bases,
                                const int64_t *off, int64_t n_reads, int k, int strands,
                                kmhg_rquery **q, int64_t *n_rows);
int kmhg_reads_query_run(kmhg_index *idx, const kmhg_reads *r, int k, int strands,
                         kmhg_rquery **q, int64_t *n_rows);
int kmhg_rquery_rows_device(kmhg_rquery *q, const int32_t **d_rows, int64_t *n_rows); /* owned by q */
int kmhg_rquery_copy_device(kmhg_rquery *q, void *d_dst, void *stream);
int kmhg_rquery_fill(kmhg_rquery *q, int32_t *rows);             /* host, 4 * n_rows int32 */
int kmhg_rquery_free(kmhg_rquery *q);

/* reads.kmer.vote: one row of six int32 per read, in read order:
 *   read, strand, pos, hits, second, total
 * A row (read, strand, i, j) of a query at k votes for pos = j - i + k, the index position at
 * which base 1 of the read (strand +1) or of rc(read) (strand -1) lies; it may be <= 0.  Its cell
 * is (strand, bin = floor(pos / band)), floored toward minus infinity, 1 <= band <= 2^30.  The
 * winning cell has the most votes; ties go to the forward strand, then to the smaller bin.
 * strand and pos = bin * band name it, hits is its votes, second the most votes among the read's
 * other cells (0: none), total all of the read's rows.  A read without rows: (r, 0, 0, 0, 0, 0).
 * The rows may come in any order; the bytes are the same on every run; scratch is O(n_rows).
 * kmhg_rrows_votes: d_rows = n_rows x 4 int32 and d_votes = n_reads x 6 int32 on the current
 * device; waits for `stream`.  Refused: band or k out of range, more than 2^31 - 1 rows, a row
 * whose read is outside 1 .. n_reads or whose strand is not +-1 (KMHG_EINVAL). */
int kmhg_rrows_votes(const void *d_rows, int64_t n_rows, int64_t n_reads, int k, int64_t band,
                     void *d_votes, void *stream);
int kmhg_rquery_votes(kmhg_rquery *q, int64_t band, int32_t *votes);   /* host, 6 * n_reads int32 */
int kmhg_rquery_votes_device(kmhg_rquery *q, int64_t band, void *d_votes, void *stream);

/* Rows of a counts index or suffix hash: keys[U] and counts[U * sources] in row order. */
int kmhg_counts_export(kmhg_index *idx, uint64_t *keys, int32_t *counts);

/* Index replication for the multi-GPU query (the index is broadcast once over RCCL/xGMI by the
 * caller): the device image is the hash table (16-B slots {key, count, end}) + the positions +
 * (codes_bytes > 0) the index sequence's 2-bit code words and N flags that the diagonal
 * query path verifies against (0.5 B per window; NULL / 0 = table probes only); export copies
 * it into caller device buffers, import rebuilds an index on the current device. */
typedef struct {
  int64_t table_bytes, positions_bytes, codes_bytes;
} kmhg_image_sizes;
int kmhg_image_sizes_get(const kmhg_index *idx, kmhg_image_sizes *sz, int64_t header[8]);
int kmhg_image_export(const kmhg_index *idx, void *d_table, void *d_positions, void *d_codes,
                      void *stream);
int kmhg_image_import(const int64_t header[8], const void *d_table, const void *d_positions,
                      const void *d_codes, void *stream, kmhg_index **out);

/* Owner-computes multi-GPU build (the reference's own partition pattern, every
 * reader thread inserting only the k-mers it owns, src/kmer_reader.c:28-39): part `part` of
 * `n_parts` walks every window of the (broadcast) sequence but keeps only the k-mers whose hash
 * bucket lies in its contiguous range [b0, b0 + nb) of the whole table's buckets, so each k-mer
 * is built on exactly one device, its positions ascending, with no all-to-all.  The parts,
 * concatenated in bucket order (positions in part order, list ends rebased by each part's first
 * position index), ARE the single-device index: the caller gathers them (RCCL) and imports the
 * result with kmhg_image_import.  A part index refuses the whole-index queries and readout; it
 * is read in place by kmhg_query_run_device_part and the kmhg_part_* kmer.pos entries.
 *   info = {b0, nb, nb_total, slots per bucket, positions N, distinct k-mers U, pairs P, max n,
 *           owns the side slot (key ~0 at k = 32) 0/1, code block bytes}
 *   export: d_table <- its nb x capb slots with count >= 2 list ends + pos_base; d_side_slot <-
 *   its side slot (16 B; meaningful when it owns it); d_positions <- its N int32 positions;
 *   d_codes <- the sequence's code block (every part computes the same one).  Synchronous. */
int kmhg_build_device_part(const void *d_seq, size_t L, int k, int part, int n_parts,
                           void *stream, kmhg_index **out);
int kmhg_part_info(kmhg_index *idx, int64_t info[10]);
int kmhg_part_export(kmhg_index *idx, int64_t pos_base, void *d_table, void *d_side_slot,
                     void *d_positions, void *d_codes, void *stream);

/* Device self-check of the property the radix passes' stable ranks rest on: the lanes of one
 * returning LDS add that hit the same address receive old values in increasing lane order
 * (kmhg_build_v2.hip V_scatter; the bucket kernels also verify every bucket's stream order and
 * fall back).  Writes the same-digit lane pairs found out of order and the pairs checked. */
int kmhg_check_lds_lane_order(uint64_t *out_of_order, uint64_t *checked);

/* Test build only (libkmhgpu_test.so; the product library counts nothing and writes zeros): the
 * bucket kernel's one-batch position buckets since the last reset -- out[0] placed by home-slot
 * counts, out[1] fallen back to the CAS pass for a repeated key, out[2] fallen back for a second
 * wrap.  Waits for the device; reset != 0 zeroes the counters after reading them. */
int kmhg_bucket_place_counters(uint64_t out[3], int reset);

/* Test build only (the product library writes zeros): bucket-id builds started since the last
 * reset -- out[0] with the packed middle stream (one digit-pos word per window between the two
 * radix passes), out[1] every other bucket-id build (bucket id and position arrays).  reset != 0
 * zeroes the counters after reading them. */
int kmhg_bid_pack_counters(uint64_t out[2], int reset);

/* Per-kernel HIP-event timing (KMHG_TIMING=1 also enables it).  The report is JSON:
 * {"kernel": [launches, total_ms], ...}; events are recorded on the kernels' own stream. */
int kmhg_timing_enable(int on);
int kmhg_timing_select(const char *kernel);   /* record only this kernel (NULL = all) */
int kmhg_timing_reset(void);
int kmhg_timing_report(char *buf, size_t cap);

/* Device memory pool (caching allocator). */
int kmhg_pool_trim(void);
int64_t kmhg_pool_cached_bytes(void);

#ifdef __cplusplus
}
#endif
#endif /* KMHGPU_H */
