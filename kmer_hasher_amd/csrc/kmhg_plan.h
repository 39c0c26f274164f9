// kmhg_plan.h -- the partitioned build's decisions (host only: no HIP, any C++17 compiler).
//
// plan_build() turns what is being built (BuildRequest), the switches the plan obeys (BuildKnobs)
// and one round of the bucket kernel on the building device into a BuildPlan: geometry, radix and
// passes, the stream family and every stream's format, which buffer side holds which stream and
// how wide each side is.  build_device_v2 (kmhg_engine.cpp) allocates from the plan and launches;
// tools/asan/host_check `plan` prints one on the CPU.  Each measured threshold sits next to the
// one decision it governs.
#pragma once
#include <stdint.h>

#include <algorithm>
#include <cmath>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "kmhg_common.h"
#include "../../include/kmhgpu.h"

namespace kmhg {

// partitioned build (kmhg_build_v2.hip)
// group buckets: mean windows per bucket and LDS sub-table slots (load 2/3).  Variant builds
// (A/B, `make variant`) may set -DKMHG_BW_WG=2048 -DKMHG_CAPW=3072 -DKMHG_BUCKET_WGS=4.
#ifndef KMHG_BW_WG
#define KMHG_BW_WG 1024
#endif
#ifndef KMHG_CAPW
#define KMHG_CAPW 1536
#endif
#ifndef KMHG_BUCKET_WGS
#define KMHG_BUCKET_WGS 8      // workgroups per CU the compact LDS table allows (1,536 slots)
#endif
constexpr uint32_t V2_BW_WG = KMHG_BW_WG;
constexpr uint32_t V2_CAPW = KMHG_CAPW;  // slots per group bucket (LDS sub-table of one workgroup)
constexpr uint32_t V2_MAXR_IL = 320;   // max radix of one partition pass (the scatter's LDS)

// What one element of a radix stream looks like.  The engine's plan, the launch wrappers and the
// kernels' template parameters all name a stream's layout with this one type (DESIGN.md "Radix
// stream formats" keeps the earlier per-kernel mode numbers findable).
enum class StreamFmt : int {
  Keys,      // u64 key only; the position is implicit (e + 1) or unused: a caller's key stream,
             // the windows of the sequence, the streams of a count-only build
  KeyPos,    // u64 key array + u32 pos array
  Packed12,  // one 12-B element {key lo, key hi, pos}
  Packed8,   // one 8-B element, key << sh | window-in-segment (Pack8, kmhg_kernels.h)
  Bids,      // u32 bucket id only (~0 = not indexed), position implicit: V_hist0's ids
  BidPos,    // u32 bucket-id array + u32 pos array
  DigitPos,  // one u32 digit-pos word, (the reading pass's digit << BID_POS_BITS) | pos
  Pos,       // u32 pos only: what the last bucket-id pass writes
  Digits8,   // the next pass's digit of each element, u8 / u16 (DigitOut, kmhg_kernels.h):
  Digits16,  // read by that pass's histogram only
};
constexpr int BID_POS_BITS = 24;
// the stream belongs to a bucket-id build: u32 words, digits without hashing
constexpr bool fmt_bid(StreamFmt f) {
  return f == StreamFmt::Bids || f == StreamFmt::BidPos || f == StreamFmt::DigitPos ||
         f == StreamFmt::Pos;
}
// the positions travel in an array of their own (pin / pout)
constexpr bool fmt_pos_array(StreamFmt f) {
  return f == StreamFmt::KeyPos || f == StreamFmt::BidPos || f == StreamFmt::Pos;
}
// bytes per element of the stream's first array (kin / kout; 0: there is none)
constexpr uint32_t fmt_key_bytes(StreamFmt f) {
  return f == StreamFmt::Pos ? 0 : f == StreamFmt::Digits8 ? 1 : f == StreamFmt::Digits16 ? 2
         : fmt_bid(f) ? 4 : f == StreamFmt::Packed12 ? 12 : 8;
}
// where an element's position lies, in u32 words of the array that holds it: offset and stride
// (Packed12 keeps it inside the element; only formats that carry a position)
constexpr uint32_t fmt_pos_word(StreamFmt f) { return f == StreamFmt::Packed12 ? 2 : 0; }
constexpr uint32_t fmt_pos_stride(StreamFmt f) { return f == StreamFmt::Packed12 ? 3 : 1; }
inline const char* fmt_name(StreamFmt f) {
  static const char* const names[] = {"Keys", "KeyPos", "Packed12", "Packed8", "Bids",
                                      "BidPos", "DigitPos", "Pos", "Digits8", "Digits16"};
  return names[(int)f];
}

// ---------------------------------------------------------------------------- the request
// What is being built: the windows of a sequence of L chars, or a stream of n_keys distinct
// keys (the counts index's table rebuild): key r is stored with count 1 and aux = r + 1.
// count_only (a key stream whose positions nobody reads: read counting): the group bucket kernel
// skips its position pass and no positions array is kept.
// count_only with co_spread = 0: the spread is chosen from the key stream's own HLL estimate
// (co_spread_for), read back while the radix passes run.
// skip_empty (count-only key streams of k <= 31): EMPTY_KEY entries are padding, not keys --
// the first pass drops them, and the valid count comes from its scan.
// codes: the build keeps the sequence's code words (the diagonal query path; bucket-id streams).
// n_parts >= 1: part `part` of an owner-computes build (n_parts = 0: a whole build).
// w > 1: a minimizer-sampled build (kmhg_minimizer.h) of the n_selected windows the selection
// pass kept, which reach the radix passes as a part's compacted windows do; the result is a whole
// index that holds only those, in a table of the unsampled geometry (plan_geometry).  w = 1
// changes nothing in the plan.
struct BuildRequest {
  bool from_keys = false;
  int64_t L = 0;
  int k = 0;
  int64_t n_keys = 0;
  bool count_only = false;
  int co_spread = 1;
  bool skip_empty = false;
  bool codes = false;
  uint32_t part = 0, n_parts = 0;
  int w = 1;
  int64_t n_selected = 0;

  int64_t windows() const { return from_keys ? n_keys : L - k + 1; }

  static BuildRequest sequence(int64_t L, int k, bool codes) {
    BuildRequest r;
    r.L = L;
    r.k = k;
    r.codes = codes;
    return r;
  }
  static BuildRequest sequence_part(int64_t L, int k, uint32_t part, uint32_t n_parts) {
    BuildRequest r = sequence(L, k, true);
    r.part = part;
    r.n_parts = n_parts;
    return r;
  }
  static BuildRequest sequence_sampled(int64_t L, int k, int w, int64_t n_selected) {
    BuildRequest r = sequence(L, k, false);
    r.w = w;
    r.n_selected = n_selected;
    return r;
  }
  static BuildRequest key_stream(int k, int64_t n_keys) {
    BuildRequest r;
    r.from_keys = true;
    r.k = k;
    r.n_keys = n_keys;
    return r;
  }
  // a padded key stream (EMPTY_KEY entries skipped) whose positions nobody reads
  static BuildRequest count_keys(int k, int64_t n_keys, int co_spread) {
    BuildRequest r = key_stream(k, n_keys);
    r.count_only = true;
    r.co_spread = co_spread;
    r.skip_empty = true;
    return r;
  }
};

// ---------------------------------------------------------------------------- the knobs
// Every switch the build obeys; the defaults are the product's behaviour.  The test build
// (-DKMHG_TEST_BUILD) fills them from the environment, once per build (read_build_knobs,
// kmhg_engine.cpp); they choose between equivalent paths and change no result, except the fault
// injection of test_disorder.  A forced choice is -1 (the plan's own rule), 0 or 1.
struct BuildKnobs {
  uint32_t maxr = V2_MAXR_IL;  // KMHG_MAXR: a lower widest radix (>= 2), to force more passes
  bool nb_round = true;        // KMHG_NB_ROUND=0: keep ceil(windows / 1,024) buckets
  int build_bid = -1;          // KMHG_BUILD_BID=0 / 1: key / bucket-id streams
#ifdef KMHG_NO_AOS
  bool aos = false;            // built with -DKMHG_NO_AOS: SoA streams (A/B)
#else
  bool aos = true;             // packed 12-B (key, pos) elements on key streams
#endif
  bool pack8 = true;           // KMHG_PACK8=0: keep the 12-B first stream
  int digit_stream = -1;       // KMHG_DIGIT_STREAM=0 / 1: digit streams off / on
  bool ds_bid = false;         // KMHG_DS_BID=1: digit streams on bucket-id streams too
  bool ds_u8 = true;           // KMHG_DS_U8=0: u16 digits at any radix
  bool ds_pack = true;         // KMHG_DS_PACK=0: digit streams leave the middle streams KeyPos
  bool bid_pack = true;        // KMHG_BID_PACK=0: the two arrays instead of digit-pos words
  int part_compact = -1;       // KMHG_PART_COMPACT=0 / 1: first pass over every window / compaction
  int build_tags = -1;         // KMHG_BUILD_TAGS=0 / 1: build-time tags on key streams
  int co_spread = 0;           // KMHG_CO_SPREAD: a forced count-only spread (0: none)
  // the launch side's
  bool fuse_bounds = true;     // KMHG_FUSE_BOUNDS=0: every bucket-start level launched on its own
  bool bucket_place = true;    // KMHG_BUCKET_PLACE=0: the CAS pass in every bucket
  int test_disorder = 0;       // KMHG_TEST_DISORDER=1|2|3: a corrupted stream or bound
};

constexpr const char* BUILD_KNOB_NAMES[] = {
    "KMHG_MAXR",       "KMHG_NB_ROUND",     "KMHG_BUILD_BID",   "KMHG_PACK8",
    "KMHG_DIGIT_STREAM", "KMHG_DS_BID",     "KMHG_DS_U8",       "KMHG_DS_PACK",
    "KMHG_BID_PACK",   "KMHG_PART_COMPACT", "KMHG_BUILD_TAGS",  "KMHG_CO_SPREAD",
    "KMHG_FUSE_BOUNDS", "KMHG_BUCKET_PLACE", "KMHG_TEST_DISORDER"};

// One knob from its text (the environment's, or host_check's command line): a switch that is on
// by default goes off on "0", one that is off goes on on "1", a forced choice is "1" or anything
// else.  False: not a build knob.
inline bool set_build_knob(BuildKnobs& kn, const char* name, const char* v) {
  const auto is = [&](const char* n) { return std::strcmp(name, n) == 0; };
  const bool off = v[0] == '0', on = v[0] == '1';
  if (is("KMHG_MAXR")) {
    if (v[0])
      kn.maxr = std::max<uint32_t>(2u, std::min<uint32_t>(V2_MAXR_IL, (uint32_t)std::atoi(v)));
  } else if (is("KMHG_NB_ROUND")) kn.nb_round = !off;
  else if (is("KMHG_BUILD_BID")) kn.build_bid = on;
  else if (is("KMHG_PACK8")) kn.pack8 = !off;
  else if (is("KMHG_DIGIT_STREAM")) kn.digit_stream = v[0] ? (int)on : -1;
  else if (is("KMHG_DS_BID")) kn.ds_bid = on;
  else if (is("KMHG_DS_U8")) kn.ds_u8 = !off;
  else if (is("KMHG_DS_PACK")) kn.ds_pack = !off;
  else if (is("KMHG_BID_PACK")) kn.bid_pack = !off;
  else if (is("KMHG_PART_COMPACT")) kn.part_compact = on;
  else if (is("KMHG_BUILD_TAGS")) kn.build_tags = on;
  else if (is("KMHG_CO_SPREAD")) {   // rounded down to a divisor of 12 (plan_geometry, co_auto)
    int f = std::max(1, std::min(12, std::atoi(v)));
    while (12 % f) --f;
    kn.co_spread = f;
  } else if (is("KMHG_FUSE_BOUNDS")) kn.fuse_bounds = !off;
  else if (is("KMHG_BUCKET_PLACE")) kn.bucket_place = !off;
  else if (is("KMHG_TEST_DISORDER")) kn.test_disorder = v[0] >= '1' && v[0] <= '3' ? v[0] - '0' : 0;
  else return false;
  return true;
}

// ---------------------------------------------------------------------------- thresholds
// Bucket-id radix streams (position builds that keep their code words) up to this many windows;
// KMHG_BUILD_BID=0 / 1 forces key / bucket-id streams.
constexpr int64_t BID_MAX_WINDOWS = 12 << 20;
inline bool bid_streams_for(int64_t Nw, const BuildKnobs& kn) {
  return kn.build_bid >= 0 ? kn.build_bid == 1 : Nw <= BID_MAX_WINDOWS;
}

constexpr double CO_FILL = 0.6;                  // target mean occupancy of a count-only bucket

// Stream entries per group bucket (in units of V2_BW_WG) for a batch of `total` keys with
// ~`distinct` distinct ones: mean distinct keys per bucket ~CO_FILL x V2_CAPW, at most 4x.
// KMHG_CO_SPREAD (tests) forces one, rounded down to a divisor of 12 (BuildKnobs::co_spread).
inline int co_spread_for(double distinct, uint64_t total, int forced) {
  if (forced) return forced;
  const double ratio =
      std::max(std::min(distinct / std::max<double>((double)total, 1.0), 1.0), 1e-3);
  const int f = (int)(CO_FILL * V2_CAPW / (V2_BW_WG * ratio));
  return std::max(1, std::min(4, f));
}

// Radix digits of small builds by 32-bit multiplies.  A digit is floor(b / div) mod R of a bucket
// id b < nb, taken with magic multipliers (Digit, kmhg_kernels.h).  With m = ceil(2^32 / d),
// d m - 2^32 < d, so for x < 2^16 and d <= 2^16 the error term x (d m - 2^32) stays below 2^32 and
// (x m) >> 32 = floor(x / d) exactly: one 32-bit high multiply where the general 64-bit form takes
// four multiplies.  magic32(1) = 0 stands for d = 1 (2^32 does not fit).
constexpr uint32_t DIGIT32_LIMIT = 1u << 16;
inline uint32_t magic32(uint32_t d) {   // ceil(2^32 / d) for d >= 2
  return d <= 1 ? 0u : (uint32_t)(0xFFFFFFFFull / d) + 1u;
}
// every dividend of a build of nb buckets is below nb (and so is its quotient by div)
inline bool digit32_ok(uint32_t nb, uint32_t div, uint32_t R) {
  return nb >= 1 && nb < DIGIT32_LIMIT && div >= 1 && div <= DIGIT32_LIMIT && R >= 1 &&
         R <= DIGIT32_LIMIT;
}
// floor(x / d) by m = magic32(d), x < 2^16.  (m = 0, d = 1: the high product is 0 and the mask
// keeps x -- no branch.)  The kernels' own code (kmhg_build_v2.hip digit_of_b), here so that the
// host can check it (tools/asan/digit_check.cpp).
__host__ __device__ inline uint32_t div_magic32(uint32_t x, uint32_t m) {
  return (uint32_t)(((uint64_t)x * m) >> 32) | (x & (m ? 0u : ~0u));
}
// the digit floor(b / div) mod R and the quotient above it, hi = floor(b / (div R)); hi and R are
// below 2^16, so their product is a 24-bit multiply on the device
__host__ __device__ inline uint32_t digit32(uint32_t b, uint32_t m32div, uint32_t m32R, uint32_t R,
                                            uint32_t& hi) {
  const uint32_t q = div_magic32(b, m32div);
  hi = div_magic32(q, m32R);
#ifdef __HIP_DEVICE_COMPILE__
  return q - __umul24(hi, R);
#else
  return q - hi * R;
#endif
}

// ---------------------------------------------------------------------------- the plan
struct BuildPlan {
  int err = KMHG_OK;           // a refusal: the engine's fail(err, msg)
  const char* msg = nullptr;
  int64_t Nw = 0;              // windows, or keys of the stream
  uint32_t ntiles = 0;         // partition tiles of PTILE windows
  Geom geom{0u, V2_CAPW};      // nb buckets; a part: buckets [b0, b0 + nb) of nbh
  bool is_part = false;
  bool empty_part = false;     // more parts than buckets: nothing to build (only geom is set)
  uint32_t R = 0, passes = 0;  // radix and radix passes: R^passes >= nb
  bool digit32 = false;        // fewer than 2^16 buckets: digits by 32-bit multiplies (digit32_ok)
  bool from_keys = false;
  bool no_pos = false;         // count-only: keys only through the passes
  bool co_auto = false;        // count-only, the spread chosen after the passes
  bool bid = false;            // bucket-id streams
  bool bid_pack = false;       // ... with the digit-pos word between their two passes
  bool aos = false;            // key streams carry packed elements
  bool pack8 = false;          // the first of two streams is Packed8: sh8, seg8 windows per
  int sh8 = 0;                 //   segment, nseg8 segments
  uint64_t seg8 = 0;
  uint32_t nseg8 = 0;
  bool ds_on = false, ds8 = false;   // digit streams, u8 digits
  bool partc = false;          // a part build compacts its own windows first (a sampled build:
  bool sampled = false;        //   its selected windows, by V_min_compact)
  bool fuse_bounds = true;     // BuildKnobs::fuse_bounds
  bool want_tags = false;      // build-time tags
  uint32_t first_pass = 0;     // the first pass of the launch loop (pass 0 has its own launches
                               // over a sequence)
  uint64_t nhist = 0;          // pass 0's histogram, [digit][tile]
  uint32_t scan_tiles = 0;     // tiles of its scan
  std::vector<StreamFmt> fmt;  // F(-1) .. F(passes - 1)
  uint32_t key_bytes[2] = {0, 0};        // per side: bytes per element of the first array,
  bool pos_array[2] = {false, false};    // and whether a position array is needed

  // F(p) = the format of the stream pass p writes, F(-1) = what the first radix pass reads
  StreamFmt F(int p) const { return fmt[(size_t)(p + 1)]; }
  // the side (0 / 1) of the two buffer pairs stream p lives on
  int side(int p) const { return (p & 1) ^ (from_keys || partc ? 1 : 0); }
  // pass p also writes the next pass's digits, which that pass's histogram reads instead of F(p)
  bool ds_out(int p) const { return ds_on && p >= 0 && p + 1 < (int)passes; }
  // each level of the bucket starts rides in its pass (BoundsFuse), except the last one of a
  // count-only build whose spread is chosen after the passes (co_auto); KMHG_FUSE_BOUNDS=0
  // (A/B) launches every level on its own
  bool fused(uint32_t p) const {
    return p >= 1 && fuse_bounds && !(co_auto && p + 1 == passes);
  }
};

namespace plan_detail {

inline void refuse(BuildPlan& P, int code, const char* msg) {
  P.err = code;
  P.msg = msg;
}

// radix plan: fewest passes whose radix fits LDS.  Tiles of PTILE windows keep ~PTILE / R
// elements per digit run: beyond ~300 digits the runs get too short for coalesced writes and
// an extra pass is cheaper.  (5: no plan of up to 4 passes.)
inline uint32_t radix_for(uint32_t nbk, uint32_t maxr, uint32_t& R) {
  for (uint32_t passes = 1; passes <= 4; ++passes) {
    R = (uint32_t)std::ceil(std::pow((double)nbk, 1.0 / passes) - 1e-9);
    while (std::pow((double)R, (double)passes) < (double)nbk) ++R;
    if (R <= maxr) return passes;
  }
  return 5u;
}

// Buckets, the part's range of them, radix and passes.  False: refused, or an empty part.
inline bool plan_geometry(BuildPlan& P, const BuildRequest& rq, const BuildKnobs& kn,
                          uint32_t device_round) {
  // A sampled build keeps the unsampled table's geometry.  The selected windows are those with
  // the smallest mix64(key), and a key's bucket is that value's high bits (bucket_of): every
  // window whose hash is small enough is selected, so the first buckets of a sampled table hold
  // nearly what they hold unsampled, however few windows are selected overall, and the last
  // ones next to nothing.  With the unsampled bucket count every bucket's keys are a subset of
  // the unsampled build's, so a sampled build overflows no bucket that build would not.
  const int64_t Nw = P.Nw;
  // group buckets: 1024 windows, one workgroup each.  (Wave buckets of 256 windows were
  // removed in round 4: group buckets halve the radix -- config 2 26.1 vs 24.8 Gbp/s -- and save
  // a pass from ~26 M windows -- config 3 26.3 vs 24.5.)
  // count-only builds: co_spread x more stream entries per group bucket -- a read batch's
  // distinct keys are a fraction of its key stream, so fewer buckets still fit their LDS
  // sub-tables (co_spread_for); one overflowing bucket fails the whole build (meta->overflow)
  // and sh_count_reads_device rebuilds at spread 1.  With co_spread = 0 the radix passes sort
  // by the bucket b1 among nb1 = 12 * ceil(Nw / (12 * V2_BW_WG)): the bucket among nb1 / s is
  // b1 / s exactly (floor(floor(h nb1 / 2^64) / s) = floor(h (nb1 / s) / 2^64)), so one sorted
  // stream serves every spread s in {1, 2, 3, 4}, and s is picked only before the bucket stage.
  int64_t bw_g = V2_BW_WG;
  if (rq.count_only && !P.co_auto) bw_g *= std::max(1, std::min(8, rq.co_spread));
  uint32_t nb_g =
      P.co_auto ? (uint32_t)(12 * std::max<int64_t>(1, (Nw + 12 * V2_BW_WG - 1) / (12 * V2_BW_WG)))
                : (uint32_t)std::max<int64_t>(1, (Nw + bw_g - 1) / bw_g);
  // Whole rounds of the bucket kernel: its workgroups take about equally long, so 4.77 rounds of
  // the device's resident workgroups (config 2: 9,766 buckets on 256 CUs x 8) cost 5; rounding
  // the bucket count up to whole rounds gives each bucket fewer windows instead (position builds
  // of 2-16 rounds; the parts of an owner-computes build split the same rounded table, so they
  // still assemble into the single-device table).  Only when the extra buckets are few (at most
  // an eighth more: a build just past a round boundary would otherwise nearly double its table
  // and halve its load).  The round is the building device's own (CUs x workgroups per CU).
  // KMHG_NB_ROUND=0 (test build) keeps ceil(windows / 1,024).
  if (!rq.from_keys && !rq.count_only && kn.nb_round) {
    const uint32_t wave_wg = device_round;
    if (wave_wg && nb_g > wave_wg && nb_g <= 16 * wave_wg) {
      const uint32_t rounded = (nb_g + wave_wg - 1) / wave_wg * wave_wg;
      if (rounded - nb_g <= nb_g / 8) nb_g = rounded;
    }
  }
  uint32_t nb = nb_g;
  P.passes = radix_for(nb_g, kn.maxr, P.R);
  // owner-computes part (the reference's reader-pool partition,
  // src/kmer_reader.c:28-39): the whole build's geometry, of which this part keeps the buckets
  // [b0, b1) -- every window is encoded and hashed, only the part's keys are partitioned
  uint32_t b0 = 0, nbh = 0;
  if (rq.n_parts >= 1) {           // n_parts = 0: a whole build
    b0 = (uint32_t)((uint64_t)nb * rq.part / rq.n_parts);
    const uint32_t b1 = (uint32_t)((uint64_t)nb * (rq.part + 1) / rq.n_parts);
    nbh = nb;
    P.is_part = true;
    if (b1 <= b0) {              // more parts than buckets: an empty part (nothing to build)
      P.geom = Geom{0u, V2_CAPW, b0, nbh};
      P.empty_part = true;
      return false;
    }
    nb = b1 - b0;
    P.passes = radix_for(nb, kn.maxr, P.R);
  }
  if (P.passes > 4) {
    refuse(P, KMHG_EOVERFLOW, "sequence too long for the partitioned build");
    return false;
  }
  P.geom = Geom{nb, V2_CAPW, b0, nbh};
  P.digit32 = digit32_ok(nb, 1u, P.R);
  P.nhist = (uint64_t)P.R * P.ntiles;
  P.scan_tiles = (uint32_t)((P.nhist + TILE - 1) / TILE);
  return true;
}

// The stream family: bucket-id or key streams, and on key streams packed elements, Pack8, digit
// streams and a part's compaction.  Returns ds_pack: digit streams take the middle streams packed.
inline bool plan_streams(BuildPlan& P, const BuildRequest& rq, const BuildKnobs& kn) {
  const int64_t Nw = P.Nw;
  const uint32_t passes = P.passes, R = P.R, n_parts = rq.n_parts;
  const bool from_keys = rq.from_keys, count_only = rq.count_only;
  // bucket-id streams (position builds that keep the code words): the radix passes carry
  // (bucket id, pos) -- 8 B per window instead of 12 -- the last pass positions only, and the
  // bucket kernel cuts each key from the code words.  The cut is a random 12-B read per window:
  // cheap while the code words (Nw / 4 bytes) stay in an XCD's 4 MB L2, a 128-B Infinity-Cache
  // line per window beyond.  Measured (A/B in one run): config 2 (10 M windows, 2.5 MB of code)
  // 30.1 -> 31.1 Gbp/s; config 3 (100 M, 25 MB) 28.5 -> 24.0 (bucket kernel 0.84 -> 2.0 ms).
  // So on up to BID_MAX_WINDOWS; KMHG_BUILD_BID=0 / 1 forces key / bucket-id streams.
  const bool bid = P.bid =
      rq.codes && !from_keys && !count_only && !P.sampled && bid_streams_for(Nw, kn);
  // position builds on key streams carry packed 12-B (key, pos) elements: a tile's digit run is
  // one contiguous write instead of a key piece and a position piece in two arrays
  // (tools/scatter_pattern.hip layout, profiles/r5a_scatter_layout.txt: radix 313 1.09 -> 0.87
  // ms per 100 M elements, radix 79 0.72 -> 0.61).  Built with -DKMHG_NO_AOS: SoA streams (A/B).
  const bool aos = P.aos = kn.aos && !from_keys && !count_only && !bid;
  // Pack8 (two-pass builds of small k: 2k <= 52): the first pass writes 8-B elements, key << sh
  // | the window's index inside its segment of 2^sh windows (sh = 64 - 2k), and the second pass
  // restores the position from the element's place in the stream (k_seg_bounds' table).  The
  // first stream's writes and the histogram pass's reads shrink from 12 to 8 B per window.
  // KMHG_PACK8=0 keeps the 12-B first stream (A/B, tests).
  P.sh8 = 64 - 2 * rq.k;
  P.seg8 = P.sh8 >= 12 && P.sh8 < 64 ? (1ull << P.sh8) : 0;
  P.nseg8 = P.seg8 ? (uint32_t)(((uint64_t)Nw + P.seg8 - 1) / P.seg8) : 0;
  const bool pack8 = P.pack8 =
      aos && passes == 2 && n_parts < 2 && !P.sampled && P.seg8 && P.nseg8 <= 256 && kn.pack8;
  // Digit streams (DS): each pass before the last also writes every output element's digit of
  // the next pass (u8 up to radix 256, else u16), and that pass's histogram reads 1-2 B per
  // element instead of the keys -- which also takes away the reason to leave the middle streams
  // unpacked.  The digit writes are short scattered runs (PTILE / R elements per tile and
  // digit); u8 digits pay once the streams outgrow the Infinity Cache, u16 digits (radix
  // 257-320: two-pass builds of ~66-100 M windows) did not.  Measured (A/B in one run,
  // profiles/r5y_ab_ds_*, r5y_ds_sizes_build_only.txt, k = 31 unless noted):
  //   u8: 500 Mbp (3 passes, radix 79) 18.37 -> 16.82 ms (u16 17.75; histograms 1.93 -> 0.48
  //     ms); 200 Mbp (3 passes, radix 59) 6.85 -> 6.23; 60 Mbp 1.773 -> 1.744; 40 Mbp
  //     1.115 -> 1.093; 30 Mbp 0.815 -> 0.804; but 20 Mbp 0.536 -> 0.549 and 16 Mbp
  //     0.433 -> 0.446 (in cache);
  //   u16: 100 Mbp (radix 317) 3.127 -> 3.149 ms; config 3 (k = 21, Pack8 first stream)
  //     2.81 -> 2.93 (histogram -0.11, first scatter +0.22 ms).
  // Sequence builds with positions on key streams without Pack8, radix <= 256, from
  // DS_MIN_WINDOWS windows; KMHG_DIGIT_STREAM=0 / 1 forces off / on, KMHG_DS_U8=0 u16 digits.
  // Bucket-id streams (u32 ids, in-cache sizes) can carry them too, but it is a wash: config 2
  // histogram 10.2 -> 6.7 us, first scatter +3-6 us, build 0.2076-0.2092 ms either way
  // (profiles/r5y_ab_ds_bid_config2.log).  KMHG_DS_BID=1 (or KMHG_DIGIT_STREAM=1) turns them on.
  constexpr int64_t DS_MIN_WINDOWS = 25'000'000;
  // (a part build's later streams hold ~1/n_parts of the windows)
  const int64_t ds_windows = P.sampled ? rq.n_selected : n_parts >= 2 ? Nw / n_parts : Nw;
  const bool ds_keys = !bid && !from_keys && !count_only && passes >= 2 &&
                       (kn.digit_stream >= 0 ? kn.digit_stream == 1
                                             : !pack8 && R <= 256 && ds_windows >= DS_MIN_WINDOWS);
  const bool ds_bids = bid && passes >= 2 &&
                       (kn.digit_stream >= 0 ? kn.digit_stream == 1 : R <= 256 && kn.ds_bid);
  P.ds_on = ds_keys || ds_bids;
  // u8 digits at a radix <= 256 (KMHG_DS_U8=0: u16, A/B)
  P.ds8 = P.ds_on && R <= 256 && kn.ds_u8;
  // Digit-pos words: a two-pass bucket-id build carries ONE u32 per window between its passes,
  // (pass-1 digit << 24) | pos, instead of the (bucket id, pos) pair -- pass 1, its histogram
  // and the bucket-start level need only that digit (the pass-0 digit is implied by where the
  // element lies), the radix of a two-pass plan up to BID_MAX_WINDOWS is far below 256 (nb <=
  // 13,824: R = 118) and the positions fit 24 bits.  Pass 0 writes and pass 1 reads 4 B per
  // window less, and a tile's digit run is one piece instead of two.  Every other bucket-id
  // build (one pass, 3+ passes under KMHG_MAXR, digit streams, KMHG_BUILD_BID=1 beyond 2^24
  // windows) keeps the two arrays.  KMHG_BID_PACK=0 (test build) forces the two arrays.
  static_assert(BID_MAX_WINDOWS < (int64_t(1) << BID_POS_BITS),
                "a default bucket-id build's positions fit the digit-pos word");
  P.bid_pack = bid && passes == 2 && R <= 256 && Nw < (int64_t(1) << BID_POS_BITS) && !ds_bids &&
               kn.bid_pack;
  // a part of 4+ (key streams): V_hist0 also writes the part's windows compacted per tile into
  // side 1's arrays (free until then) with their counts; a scan of the counts and one copy make
  // them a dense (key, position) stream of ~1/n_parts of the windows, and every radix pass runs
  // over that alone -- instead of encoding and hashing every window again in a first pass over
  // all of them.  It costs a copy and one more pass over the part's windows, so it pays from 4
  // parts on (one-GPU rehearsal, tools/part_step.py, per-rank step of 10 Mbp per part: 2 parts
  // 0.397 -> 0.467 ms, 4 parts 0.504 -> 0.495, 8 parts 0.749 -> 0.581).  KMHG_PART_COMPACT=0 / 1
  // forces the first pass over every window / the compaction (tests).
  // (a sampled build always: the selection pass's mask is what compacts)
  P.partc = P.sampled || (!from_keys && n_parts >= 2 && !bid && rq.codes &&
                          (kn.part_compact >= 0 ? kn.part_compact == 1 : n_parts >= 4));
  // Build-time tags (round 6): a position build beyond the cache (key
  // streams, Nw > BID_MAX_WINDOWS) writes the diagonal query path's slot tags and repeated-key
  // bits itself, so the first seq.kmer.pos of a new index does not pay V_diag_prep (2.6 ms at
  // 500 Mbp, +70 % on the query).  In cache (config 2) the build is the headline and the
  // preparation stays with the first query (round-3 A/B: tags in the build +1-1.5 % there).
  // A part of an owner-computes build does the same for its own slots and keys (the owner-
  // routed query runs the diagonal path on it).  KMHG_BUILD_TAGS=0 / 1 (test build) forces
  // either on key streams.
  // A sampled index never takes the diagonal path (it does not hold every valid window): no tags.
  P.want_tags = rq.codes && !bid && !from_keys && !count_only && !P.sampled &&
                (kn.build_tags >= 0 ? kn.build_tags == 1 : Nw > BID_MAX_WINDOWS);
  return ds_keys && kn.ds_pack;
}

// The plan's outcome, once: F(p) = the format of the stream pass p writes, F(-1) = what the
// first radix pass reads (the windows of the sequence and a caller's key stream are Keys,
// positions implicit).  Everything in the launch half -- buffer sizes, which kernel instance a
// pass, its histogram, its bucket-start level and the bucket kernel take -- reads this table.
inline void plan_formats(BuildPlan& P, bool ds_pack) {
  // Which streams are packed (stream p = pass p's output; -1 = a part build's dense stream):
  // the last one, which only the bucket kernel reads, always; an earlier one only at a radix
  // where the scatter's saving beats the 4 more bytes per element its histogram pass then reads.
  // Measured: config 3 (2 passes, radix 313) every stream packed 3.49 -> 3.21 ms per build
  // (scatters 0.94 + 1.03 -> 0.75 + 0.91 ms, histogram 0.27 -> 0.36); the 500 Mbp build (3
  // passes, radix 79) 18.2 -> 18.6 ms (histograms 1.9 -> 2.8 ms, scatters 11.2 -> 10.3), A/B
  // in one run (profiles/r5b_ab_aos_config3.log, r5c_ab_aos_config5.log).
  constexpr uint32_t AOS_MIN_RADIX = 160;
  const int passes = (int)P.passes;
  const auto packed = [&](int p) {
    return P.aos && (p + 1 == passes || P.R >= AOS_MIN_RADIX || ds_pack);
  };
  P.fmt.assign((size_t)passes + 1, StreamFmt::Keys);
  const auto F = [&](int p) -> StreamFmt& { return P.fmt[(size_t)(p + 1)]; };
  F(-1) = P.bid ? StreamFmt::Bids : P.partc && packed(-1) ? StreamFmt::Packed12
          : P.partc ? StreamFmt::KeyPos : StreamFmt::Keys;
  for (int p = 0; p < passes; ++p) {
    const bool last = p + 1 == passes;
    F(p) = P.no_pos ? StreamFmt::Keys
           : P.bid  ? (last ? StreamFmt::Pos : P.bid_pack ? StreamFmt::DigitPos : StreamFmt::BidPos)
           : P.pack8 && p == 0 ? StreamFmt::Packed8
           : packed(p)         ? StreamFmt::Packed12
                               : StreamFmt::KeyPos;
  }
}

// Stream p lives on side p mod 2 of two (first array, position array) buffer pairs -- flipped
// where the radix passes start at pass 0 in the launch loop, so that their first output lands
// on side 1 -- each side sized for the widest stream it holds (+ pad).  F(-1) is stored here
// only where V_hist0 / V_part_dense wrote it (ids, a part's dense stream).
// (Removed in round 4 after measurement, DESIGN.md §5: radix passes writing whole 128-B lines
// through LDS write-combining buffers -- config 3 29.2 -> 25.0-28.7 Gbp/s, the 500 Mbp build
// 18.1 -> 18.9-22.7 ms.)
inline void plan_sides(BuildPlan& P) {
  for (int p = P.bid || P.partc ? -1 : 0; p < (int)P.passes; ++p) {
    P.key_bytes[P.side(p)] = std::max(P.key_bytes[P.side(p)], fmt_key_bytes(P.F(p)));
    P.pos_array[P.side(p)] |= fmt_pos_array(P.F(p));
  }
  if (P.partc) {               // the compacted tiles: u64 keys and positions on side 1
    P.key_bytes[1] = std::max(P.key_bytes[1], 8u);
    P.pos_array[1] = true;
  }
}

}  // namespace plan_detail

// device_round: one round of the bucket kernel on the building device, its CUs x the workgroups
// one CU holds (0: unknown, no rounding).  No allocation apart from the format table, no I/O.
inline BuildPlan plan_build(const BuildRequest& rq, const BuildKnobs& kn, uint32_t device_round) {
  using namespace plan_detail;
  BuildPlan P;
  P.from_keys = rq.from_keys;
  P.Nw = rq.windows();
  P.no_pos = rq.count_only;
  P.co_auto = rq.count_only && rq.co_spread == 0;
  P.fuse_bounds = kn.fuse_bounds;
  if (rq.from_keys && P.Nw < 1) {
    refuse(P, KMHG_EINVAL, "empty key stream (internal error)");
  } else if (rq.skip_empty && !(rq.from_keys && rq.count_only && rq.k < 32)) {
    refuse(P, KMHG_EINVAL, "padded key stream outside a count-only build (internal error)");
  } else if (rq.n_parts >= 1 && (rq.from_keys || rq.count_only)) {
    refuse(P, KMHG_EINVAL, "part builds index sequences only");
  } else if (rq.w > 1 && rq.n_parts >= 1) {
    refuse(P, KMHG_EINVAL, "part builds index every window (w must be 1)");
  } else if (rq.w > 1 && (rq.from_keys || rq.count_only)) {
    refuse(P, KMHG_EINVAL, "sampling selects windows of a sequence (internal error)");
  }
  P.sampled = rq.w > 1;
  if (P.err != KMHG_OK) return P;
  P.ntiles = (uint32_t)((P.Nw + PTILE - 1) / PTILE);
  if (!plan_geometry(P, rq, kn, device_round)) return P;
  const bool ds_pack = plan_streams(P, rq, kn);
  plan_formats(P, ds_pack);
  plan_sides(P);
  // the radix passes of the launch loop start at pass 0 over a caller's keys or a part's dense
  // stream; over a sequence pass 0 has its own launches
  P.first_pass = rq.from_keys || P.partc ? 0 : 1;
  return P;
}

}  // namespace kmhg
