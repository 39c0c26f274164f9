// kmhg_build_v2.hip -- partitioned index build: no per-window global atomics.
//
// Replaces the same reference loops as K_insert/K_scatter/K_sort (src/kmer_pos.c:36-50, 66-98,
// 21-33; kvec growth src/kvec.h:74-80) with an HBM-streaming design for CDNA4:
//
//   V_hist0     LDS-staged 2-bit encode + N mask of every window (as K_insert) and a per-tile
//               histogram of the first radix digit of each window's bucket; keeps the sequence's
//               code words (the diagonal query path) and, for small inputs, every window's
//               bucket id
//   V_scan      exclusive scan of the [digit][tile] histograms (decoupled look-back)
//   V_scatter   stable radix pass: every wave ranks its 512 elements by digit with the
//               returned values of its LDS count atomics (lane-ordered; a device self-check picks
//               ballot ranks where that does not hold), elements land at histogram offsets --
//               LSD over 1-3 digits sorts the windows by bucket while keeping position order
//               inside a bucket
//   V_hist      digit histogram for the next radix pass
//   V_bounds    bucket start offsets in the bucket-sorted stream (from the histograms for <= 2
//               passes)
//   V_bucket_wg ONE WORKGROUP PER BUCKET of ~1,024 windows: the bucket's keys go into a shared
//               LDS hash table (LDS CAS + count atomics), the counts are scanned, repeated keys'
//               windows are ranked in position order, so positions are written ascending per key
//               by construction (no sort).  The LDS table is written out as the bucket's
//               sub-table of the global table.
//
// A bucket's windows are exactly its keys' positions, so the CSR slice of bucket b is
// [start[b], start[b+1]) of `positions` with no global coordination.
#include <hip/hip_runtime.h>
#include <algorithm>
#include <cstdlib>
#include <string>
#include <type_traits>
#include "kmhg_common.h"
#include "kmhg_device.h"
#include "kmhg_kernels.h"

namespace kmhg {

// Diagnostic phase stamps (built only with -DKMHG_STAMPS into a separate library; the real
// kernels execute no stamp).  Lane 0 of each bucket's wave writes s_memtime per phase.
#ifdef KMHG_STAMPS
__device__ uint64_t* g_stamps;
#define STAMP(b, i)                                                                   \
  do {                                                                                \
    __builtin_amdgcn_sched_barrier(0);                                                \
    uint64_t _t = __builtin_amdgcn_s_memtime();                                       \
    if (lane_id() == 0 && g_stamps) g_stamps[(uint64_t)(b) * 8 + (i)] = _t;           \
    __builtin_amdgcn_sched_barrier(0);                                                \
  } while (0)
#define STAMP_WG(b, i) do { if (threadIdx.x < 64) STAMP(b, i); } while (0)
// ... after this wave's outstanding loads have landed (splits load latency from the work after)
#define STAMP_WG_DRAIN(b, i) \
  do { __builtin_amdgcn_s_waitcnt(0); if (threadIdx.x < 64) STAMP(b, i); } while (0)
#else
#define STAMP(b, i) do {} while (0)
#define STAMP_WG(b, i) do {} while (0)
#define STAMP_WG_DRAIN(b, i) do {} while (0)
#endif

__device__ __forceinline__ void wave_sync() {
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

// Radix digit of a key's bucket: floor(b / div) mod R with host-computed magic multipliers,
// floor(x / d) = mulhi64(x, ceil(2^64 / d)) exactly for x, d < 2^32 (m = 0 encodes d = 1) --
// no integer division in the kernels.
__device__ __forceinline__ uint32_t div_magic(uint32_t x, uint64_t m) {
  return m ? (uint32_t)__umul64hi((uint64_t)x, m) : x;
}
// The bucket of hash h inside this build's part (Geom: whole table b0 = 0, nbh = nb); a key of
// another part's range gives a value >= g.nb (unsigned wrap below b0).
__device__ __forceinline__ uint32_t bucket_local(uint64_t h, const Geom& g) {
  return bucket_of(h, g.nbh ? g.nbh : g.nb) - g.b0;
}
__device__ __forceinline__ bool in_part(uint64_t h, const Geom& g) {
  return bucket_local(h, g) < g.nb;
}
// the side slot (key ~0 at k = 32) belongs to the bucket of mix64(~0) of the whole table
__device__ __forceinline__ bool side_bucket(uint32_t b, const Geom& g) {
  return b + g.b0 == bucket_of(mix64(EMPTY_KEY), g.nbh ? g.nbh : g.nb);
}
// A build of fewer than 2^16 buckets (Digit::small; digit32_ok, digit32 in kmhg_plan.h) takes
// the 32-bit form instead: one v_mul_hi_u32 per division where the 64-bit form is four multiplies.
// radix digit of a bucket id (bucket-id streams carry it instead of the key).  SMALL: the caller
// has tested D.small once (V_hist0's window loop), 1 = set, 0 = not set; -1: tested here.
template <int SMALL = -1>
__device__ __forceinline__ uint32_t digit_of_b(uint32_t b, const Digit& D) {
  if (SMALL < 0 ? D.small != 0 : SMALL != 0) {
    uint32_t hi;
    return digit32(b, D.m32div, D.m32R, D.R, hi);
  }
  const uint32_t q = div_magic(b, D.mdiv);
  return q - div_magic(q, D.mR) * D.R;
}
// ... and the quotient above it, floor(b / (div R)): in a two-pass plan (b < R^2) the next pass's
// digit, for free (the digit-pos word of the packed bucket-id stream)
__device__ __forceinline__ uint32_t digit_of_b_hi(uint32_t b, const Digit& D, uint32_t& hi) {
  if (D.small) return digit32(b, D.m32div, D.m32R, D.R, hi);
  const uint32_t q = div_magic(b, D.mdiv);
  hi = div_magic(q, D.mR);
  return q - hi * D.R;
}
__device__ __forceinline__ uint32_t digit_of_h(uint64_t h, const Geom& g, const Digit& D) {
  return digit_of_b(bucket_local(h, g), D);
}
__device__ __forceinline__ uint32_t digit_of(uint64_t key, const Geom& g, const Digit& D) {
  return digit_of_h(mix64(key), g, D);
}
// The radix digit of ONE element of a stream of format F -- the only place that knows how a
// format holds it.  w = the element's word already in registers: the u64 key (Keys, KeyPos,
// Packed12), the packed 8-B element (Packed8: the key is w >> sh, sh = Pack8::sh), the u32 id
// or digit-pos word (bucket-id formats), or the digit itself (Digits8 / Digits16).
// In two steps, for a caller that takes two digits of one element (V_scatter reading Packed8):
// digit_src is what every digit of the element is taken from -- the hash of its key, or the
// word itself -- and digit_of_src one digit of that.
template <StreamFmt F>
__device__ __forceinline__ uint64_t digit_src(uint64_t w, int sh) {
  if constexpr (fmt_bid(F) || F == StreamFmt::Digits8 || F == StreamFmt::Digits16) return w;
  else return mix64(F == StreamFmt::Packed8 ? w >> sh : w);
}
template <StreamFmt F>
__device__ __forceinline__ uint32_t digit_of_src(uint64_t x, const Geom& g, const Digit& D) {
  if constexpr (F == StreamFmt::Digits8 || F == StreamFmt::Digits16) return (uint32_t)x;
  else if constexpr (F == StreamFmt::DigitPos) return (uint32_t)x >> BID_POS_BITS;
  else if constexpr (fmt_bid(F)) return digit_of_b((uint32_t)x, D);
  else return digit_of_h(x, g, D);
}
template <StreamFmt F>
__device__ __forceinline__ uint32_t digit_of_elem(uint64_t w, const Geom& g, const Digit& D,
                                                  int sh) {
  return digit_of_src<F>(digit_src<F>(w, sh), g, D);
}
// ... of element i of the stream's first array `in`
template <StreamFmt F>
__device__ __forceinline__ uint32_t digit_of_elem(const void* __restrict__ in, uint64_t i,
                                                  const Geom& g, const Digit& D, int sh) {
  if constexpr (fmt_bid(F)) {
    return digit_of_elem<F>(reinterpret_cast<const uint32_t*>(in)[i], g, D, sh);
  } else if constexpr (F == StreamFmt::Packed12) {
    const uint32_t* w = reinterpret_cast<const uint32_t*>(in) + 3 * i;
    return digit_of_elem<F>(((uint64_t)w[1] << 32) | w[0], g, D, sh);
  } else {
    return digit_of_elem<F>(reinterpret_cast<const uint64_t*>(in)[i], g, D, sh);
  }
}

// Lanes of the wave holding the same `v` (nbits wide) among active lanes: one ballot per bit.
__device__ __forceinline__ uint64_t match_bits(uint32_t v, int nbits, bool act) {
  uint64_t m = __ballot(act);
  for (int b = 0; b < nbits; ++b) {
    const bool bit = (v >> b) & 1u;
    const uint64_t x = __ballot(act && bit);
    m &= bit ? x : ~x;
  }
  return m;
}

// The diagonal query path's copy of the index sequence (DiagBlock, kmhg_kernels.h), written by
// V_hist0 from its stage: the tile's PTILE / 16 code words and N-flag words (the last tile also
// the words its last windows reach into).  Thread t stores the word it packed itself (stage word
// t), so no barrier is needed first.  ~0.4 B per window against the build's ~17.
constexpr int DIAG_TW = PTILE / 16;             // code words per tile
constexpr int DIAG_EXTRA = 3;                   // ... beyond the last tile's own
static_assert(PSTAGE_W16 <= BLOCK && HALO % 16 == 0 && HALO / 16 + DIAG_TW + DIAG_EXTRA <= PSTAGE_W16,
              "one stage word per thread; the last tile's extra words are staged");
__device__ __forceinline__ void diag_words_out(const PStage& st, uint32_t tile, uint32_t ntiles,
                                               uint32_t* __restrict__ code,
                                               uint16_t* __restrict__ nbit) {
  const int w = (int)threadIdx.x - HALO / 16;
  if (w >= 0 && w < (tile + 1 == ntiles ? DIAG_TW + DIAG_EXTRA : DIAG_TW)) {
    code[(uint64_t)tile * DIAG_TW + w] = st.code[threadIdx.x];
    nbit[(uint64_t)tile * DIAG_TW + w] = (uint16_t)st.nbit[threadIdx.x];
  }
}

// Persistent form for the interleaved schedule (one histogram column per tile): workgroup w
// walks virtual tiles w, w + G, ... (XCD-contiguous like the scatter) and loads the next tile's
// chars into registers while it encodes the current one, so the load latency of all but the
// first tile is hidden behind the encode.
// CODES (position indices): the diagonal query path's code and N-flag words ride along, each
// thread storing the words it packed right after the pack, BEFORE the next tile's loads are
// issued, so the wait for those loads never waits on these stores.  (A/B, config 2: validity
// ballots kept in the window loop and stored per tile cost 24 -> 30-41 us; a kernel of its own
// 18 us; these stores ~1 us.)
// BIDS (bucket-id builds): every window's bucket id (~0 for a window that is not indexed or
// outside this part) is stored in window order, one coalesced 4-B store per window, so the first
// scatter pass reads the ids instead of encoding and hashing every window a second time.
#ifndef KMHG_HIST0_WAVES
#define KMHG_HIST0_WAVES 6   // the bound; the kernels need 42-47 VGPRs (hist0_valu_resources.txt)
#endif
// PARTC (a part build of an owner-computes build, key streams): the windows this part owns are
// written compacted per tile instead of counted -- (key, position) of tile t's owned windows in
// window order at [t * PTILE, t * PTILE + tcnt[t]) -- and V_part_dense packs them into one
// stream, which the radix passes read: ~1/n_parts of the windows instead of encoding and hashing
// every window of the sequence a second time.
template <bool CODES, bool BIDS = false, bool PARTC = false>
__global__ void __launch_bounds__(BLOCK, PARTC ? 5 : KMHG_HIST0_WAVES)   // PARTC: no spills
k_v2_hist0p(const uint8_t* __restrict__ seq, int64_t L, int k, int64_t Nw, Geom g, Digit D,
            uint32_t* __restrict__ hist, uint32_t ntiles, uint64_t* __restrict__ scan_status,
            uint32_t n_status, BuildMeta* __restrict__ meta, uint32_t* __restrict__ code,
            uint16_t* __restrict__ nbit, uint32_t* __restrict__ bids,
            uint64_t* __restrict__ ckeys, uint32_t* __restrict__ cpos,
            uint32_t* __restrict__ tcnt) {
  __shared__ PStage st;
  __shared__ uint32_t lh[V2_MAXR];
  __shared__ uint64_t scs[5];
  __shared__ uint64_t sk[PARTC ? PTILE : 1];     // PARTC: the tile's own windows, compacted
  __shared__ uint32_t sp[PARTC ? PTILE : 1];
  for (uint32_t i = blockIdx.x * BLOCK + threadIdx.x; i < n_status; i += gridDim.x * BLOCK)
    scan_status[i] = 0;
  if (blockIdx.x == 0 && threadIdx.x < sizeof(BuildMeta) / 4)
    reinterpret_cast<uint32_t*>(meta)[threadIdx.x] = 0u;
  const uint32_t G = gridDim.x;
  const uint32_t n_iter = (ntiles - blockIdx.x + G - 1) / G;
  auto tile_at = [&](uint32_t i) -> uint32_t { return xcd_remap(blockIdx.x + i * G, ntiles); };
  for (uint32_t d = threadIdx.x; d < D.R; d += BLOCK) lh[d] = 0;
  StageRegs<PSTAGE_W16> regs;
  stage_load<PSTAGE_W16, true>(regs, seq, L, (int64_t)tile_at(0) * PTILE - HALO, true);
  for (uint32_t it = 0; it < n_iter; ++it) {
    const uint32_t tile = tile_at(it);
    const int64_t tile0 = (int64_t)tile * PTILE;
    stage_pack(regs, st);                      // the previous tile's reads of st are done
    if (CODES) diag_words_out(st, tile, ntiles, code, nbit);
    if (it + 1 < n_iter)
      stage_load<PSTAGE_W16, true>(regs, seq, L, (int64_t)tile_at(it + 1) * PTILE - HALO, true);
    __syncthreads();
    // thread t takes the 8 consecutive windows [8 t, 8 t + 8) of the tile: their code and N
    // flags come from 8 LDS reads (Win8) instead of 6 per window -- this pass was bound
    // by those reads -- and their bucket ids leave as two 16-B stores
    static_assert(PWPT == 8, "Win8 covers 8 windows per thread");
    {
      const int w0 = PWPT * threadIdx.x;
      const int64_t s0 = tile0 + w0;
      const Win8 win(st, HALO + w0, s0, L, k);
      uint32_t bl[8];
      // `all`: the windows are known to be valid (vm unused), else vm says which are; `small`:
      // D.small, tested once per tile instead of once per window
      auto windows = [&](auto all, auto small, uint32_t vm) {
#pragma unroll
        for (int j = 0; j < 8; ++j) {
          bl[j] = ~0u;
          if (decltype(all)::value || (vm >> j & 1u)) {
            const uint32_t b = bucket_local(mix64(win.key(j)), g);
            if (b < g.nb) {
              if (!PARTC) atomicAdd(&lh[digit_of_b<decltype(small)::value ? 1 : 0>(b, D)], 1u);
              bl[j] = b;
            }
          }
        }
      };
      auto windows_of = [&](auto all, uint32_t vm) {
        if (!PARTC && D.small) windows(all, std::true_type{}, vm);
        else windows(all, std::false_type{}, vm);
      };
      // Validity once per thread, and not at all in a wave that sees no N and is nowhere near
      // the sequence's end -- almost every wave of real input
      if (__ballot(!win.all_valid(Nw)) == 0) windows_of(std::true_type{}, 0xFFu);
      else windows_of(std::false_type{}, win.valid_mask(Nw));
      if (PARTC) {                 // this part's windows, compacted in window order
        uint32_t own = 0;
#pragma unroll
        for (int j = 0; j < 8; ++j) own |= (bl[j] != ~0u ? 1u : 0u) << j;
        uint64_t tot;
        uint32_t at = (uint32_t)block_excl_scan((uint64_t)__popc(own), scs, tot);
#pragma unroll
        for (int j = 0; j < 8; ++j) {
          if (own >> j & 1u) {
            sk[at] = win.key(j);
            sp[at] = (uint32_t)(s0 + j + 1);
            ++at;
          }
        }
        __syncthreads();
        // out of LDS in order: consecutive lanes, consecutive entries
        const uint64_t base = (uint64_t)tile * PTILE;
        for (uint32_t i = threadIdx.x; i < (uint32_t)tot; i += BLOCK) {
          ckeys[base + i] = sk[i];
          cpos[base + i] = sp[i];
        }
        if (threadIdx.x == 0) tcnt[tile] = (uint32_t)tot;
      }
      // the id array holds Nw + PTILE entries: a tile's last 16-B stores stay inside it
      if (BIDS && s0 < Nw) {
        uint4* o = reinterpret_cast<uint4*>(bids + s0);
        o[0] = make_uint4(bl[0], bl[1], bl[2], bl[3]);
        o[1] = make_uint4(bl[4], bl[5], bl[6], bl[7]);
      }
    }
    __syncthreads();
    for (uint32_t d = threadIdx.x; !PARTC && d < D.R; d += BLOCK) {
      hist[(size_t)d * ntiles + tile] = lh[d];
      lh[d] = 0;                               // next tile's atomics follow a barrier
    }
  }
}

// ---------------------------------------------------------------- V_scan (u32, exclusive)
// Single pass: tiles in ticket order, decoupled look-back (kmhg_device.h) for the tile base.
// `status` holds one look-back word per tile and the ticket at status[ntiles]; the preceding
// histogram kernel zeroed them.  *total <- sum (the number of valid windows).
// J entries per thread (TILE = BLOCK * J per workgroup): J = 32 for long arrays (a 4x shorter
// look-back chain, 16-B loads).
template <int J>
__global__ void __launch_bounds__(BLOCK)
k_scan_lb_u32(uint32_t* __restrict__ a, uint64_t n, uint64_t* __restrict__ status,
              uint32_t ntiles, uint32_t* __restrict__ total) {
  __shared__ uint64_t sh[8];
  __shared__ uint32_t tk;
  __shared__ uint64_t base_sh;
  const uint32_t tile = take_ticket(reinterpret_cast<uint32_t*>(status + ntiles), &tk);
  const uint64_t base = (uint64_t)tile * (BLOCK * J) + (uint64_t)threadIdx.x * J;
  uint32_t v[J];
  uint64_t sum = 0;
  if (J % 4 == 0 && base + J <= n) {          // whole: 16-B loads (a is 16-B aligned, J % 4 == 0)
#pragma unroll
    for (int j = 0; j < J; j += 4) {
      const uint4 x = *reinterpret_cast<const uint4*>(a + base + j);
      v[j] = x.x; v[j + 1] = x.y; v[j + 2] = x.z; v[j + 3] = x.w;
    }
  } else {
#pragma unroll
    for (int j = 0; j < J; ++j) v[j] = (base + j < n) ? a[base + j] : 0u;
  }
#pragma unroll
  for (int j = 0; j < J; ++j) sum += v[j];
  uint64_t tot;
  const uint64_t ex = block_excl_scan(sum, sh, tot);
  if (threadIdx.x < 64) {
    const uint64_t x = lookback_excl(status, tile, tot);
    if (threadIdx.x == 0) {
      base_sh = x;
      if (tile == ntiles - 1) *total = (uint32_t)(x + tot);
    }
  }
  __syncthreads();
  uint64_t run = ex + base_sh;
#pragma unroll
  for (int j = 0; j < J; ++j) {
    const uint32_t x = v[j];
    v[j] = (uint32_t)run;
    run += x;
  }
  if (J % 4 == 0 && base + J <= n) {
#pragma unroll
    for (int j = 0; j < J; j += 4)
      *reinterpret_cast<uint4*>(a + base + j) = make_uint4(v[j], v[j + 1], v[j + 2], v[j + 3]);
  } else {
#pragma unroll
    for (int j = 0; j < J; ++j)
      if (base + j < n) a[base + j] = v[j];
  }
}

// ---------------------------------------------------------------- V_hist (passes >= 1)
// HLL (count-only builds, first pass): a HyperLogLog sketch of the distinct keys rides on the
// histogram pass, which hashes every key anyway.  A 1/HLL_SAMPLE key-space sample (h mod 64 == 0)
// updates register (h >> 6) mod 256 with rho = leading zeros of h's top 50 bits + 1; each
// workgroup leaves its registers as one 256-B row (bytes), V_hll reduces the rows.
constexpr uint32_t HLL_SAMPLE_BITS = 6;
constexpr uint32_t HLL_PART_ROWS = 256;        // V_hll workgroups (partial rows) at most
static_assert(HLL_PART_WORDS == HLL_PART_ROWS * 64 + 1, "V_hll partial rows + ticket");

// The first pass over a caller's key stream (format Keys: exactly n keys, no pad), one workgroup
// per tile; every later pass takes the persistent k_v2_histp.
template <bool HLL>
__global__ void __launch_bounds__(BLOCK)
k_v2_hist(const uint64_t* __restrict__ keys, const uint32_t* __restrict__ n_ptr, Geom g,
          Digit D, uint32_t* __restrict__ hist, uint32_t ntiles,
          uint64_t* __restrict__ scan_status, uint32_t n_status, uint32_t* __restrict__ hll_rows,
          uint32_t* __restrict__ hll_regs, uint32_t* __restrict__ save_col0, int skip_empty) {
  __shared__ uint32_t lh[V2_MAXR];
  __shared__ uint32_t hreg[HLL ? HLL_REGS : 1];
  for (uint32_t i = blockIdx.x * BLOCK + threadIdx.x; i < n_status; i += gridDim.x * BLOCK)
    scan_status[i] = 0;
  // the previous pass's scanned column 0 (digit starts), kept for V_bounds_lo before this
  // workgroup -- the only writer of column 0 -- overwrites it
  const uint32_t c = xcd_remap(blockIdx.x, ntiles);      // one workgroup per tile
  if (save_col0 && c == 0)
    for (uint32_t d = threadIdx.x; d < D.R; d += BLOCK) save_col0[d] = hist[(size_t)d * ntiles];
  if (HLL) {
    for (uint32_t i = threadIdx.x; i < HLL_REGS; i += BLOCK) hreg[i] = 0;
  }
  const uint64_t n = *n_ptr;
  const uint64_t e0 = (uint64_t)c * PTILE;
  const uint64_t e1 = min(n, e0 + (uint64_t)PTILE);
  const uint32_t R = D.R;
  for (uint32_t d = threadIdx.x; d < R; d += BLOCK) lh[d] = 0;
  __syncthreads();
  constexpr int NL = 4;                           // loads in flight per lane
  for (uint64_t e = e0 + threadIdx.x; e < e1; e += NL * BLOCK) {
    uint32_t dg[NL];
    bool in[NL];
#pragma unroll
    for (int j = 0; j < NL; ++j) {
      in[j] = e + j * BLOCK < e1;
      const uint64_t key = in[j] ? keys[e + j * BLOCK] : 0ull;
      if (skip_empty && key == EMPTY_KEY) in[j] = false;      // a padded read's unused slot
      const uint64_t h = in[j] ? mix64(key) : 1ull;
      dg[j] = in[j] ? digit_of_h(h, g, D) : 0u;
      if (HLL && (h & ((1u << HLL_SAMPLE_BITS) - 1)) == 0)
        atomicMax(&hreg[(uint32_t)(h >> HLL_SAMPLE_BITS) & (HLL_REGS - 1)],
                  (uint32_t)__clzll(h | ((1ull << (HLL_SAMPLE_BITS + 8)) - 1)) + 1u);
    }
#pragma unroll
    for (int j = 0; j < NL; ++j)
      if (in[j]) atomicAdd(&lh[dg[j]], 1u);
  }
  __syncthreads();
  for (uint32_t d = threadIdx.x; d < R; d += BLOCK) hist[(size_t)d * ntiles + c] = lh[d];
  if (HLL && threadIdx.x < HLL_REGS / 4) {
    const uint32_t* h4 = hreg + 4 * threadIdx.x;
    hll_rows[(size_t)blockIdx.x * (HLL_REGS / 4) + threadIdx.x] =
        h4[0] | (h4[1] << 8) | (h4[2] << 16) | (h4[3] << 24);
  }
}

// Persistent form for the interleaved schedule (position builds' later passes): workgroup w walks
// virtual tiles w, w + G, ... (XCD-contiguous like the scatter), thread t taking the 8
// consecutive elements [8 t, 8 t + 8) of a tile with 16-B loads, the next tile's loads in flight
// while this one is counted -- the one-tile-per-workgroup form exposed every workgroup's load
// latency (config 2: 14.5 us for 40 MB).  `in` holds n + PTILE elements (the passes' padded
// streams), so whole-tile loads stay inside it.
// IN = the format of `in`.  KeyPos reads the u64 key array (a Keys stream takes the same
// instance); BidPos the u32 bucket ids; Packed12 the position builds' packed key streams;
// Packed8 the 8-B elements whose key is e >> sh; Digits16 / Digits8 the previous pass's digit
// stream (DS in V_scatter) instead of its elements; DigitPos the packed bucket-id stream, whose
// digit is w >> 24.  What differs per format here is the load shape only (16-B loads; one
// dwordx3 element per lane for Packed12; one 8-B load for Digits8) -- the digit of an element is
// digit_of_elem's.
template <StreamFmt IN>
__global__ void __launch_bounds__(BLOCK)
k_v2_histp(const uint64_t* __restrict__ in, const uint32_t* __restrict__ n_ptr, Geom g, Digit D,
           uint32_t* __restrict__ hist, uint32_t ntiles, uint64_t* __restrict__ scan_status,
           uint32_t n_status, uint32_t* __restrict__ save_col0, int sh) {
  static_assert(IN != StreamFmt::Keys && IN != StreamFmt::Bids && IN != StreamFmt::Pos,
                "Keys streams take the KeyPos instance; Bids and Pos streams are never counted");
  __shared__ uint32_t lh[V2_MAXR];
  for (uint32_t i = blockIdx.x * BLOCK + threadIdx.x; i < n_status; i += gridDim.x * BLOCK)
    scan_status[i] = 0;
  const uint64_t n = *n_ptr;
  const uint32_t G = gridDim.x, R = D.R;
  const uint32_t n_iter = (ntiles - blockIdx.x + G - 1) / G;
  auto tile_at = [&](uint32_t i) -> uint32_t { return xcd_remap(blockIdx.x + i * G, ntiles); };
  // the previous pass's scanned column 0, saved by the workgroup that writes column 0 (tile 0)
  // before it does
  if (save_col0 && tile_at(0) == 0)
    for (uint32_t d = threadIdx.x; d < R; d += BLOCK) save_col0[d] = hist[(size_t)d * ntiles];
  for (uint32_t d = threadIdx.x; d < R; d += BLOCK) lh[d] = 0;
  if constexpr (IN == StreamFmt::Packed12) {
    // packed 12-B elements: thread t takes elements t + 256 j of the tile (j < 8), so every
    // load instruction reads 768 contiguous bytes per wave (one element per lane, dwordx3); a
    // thread's 96 consecutive bytes would spread each instruction over 48 lines
    uint3 nx[8];
    auto prefetch = [&](uint32_t tile) {
      const uint3* src = reinterpret_cast<const uint3*>(in) + (uint64_t)tile * PTILE + threadIdx.x;
#pragma unroll
      for (int j = 0; j < 8; ++j) nx[j] = src[j * BLOCK];
    };
    prefetch(tile_at(0));
    for (uint32_t it = 0; it < n_iter; ++it) {
      const uint32_t tile = tile_at(it);
      uint3 cur[8];
#pragma unroll
      for (int j = 0; j < 8; ++j) cur[j] = nx[j];
      if (it + 1 < n_iter) prefetch(tile_at(it + 1));
      __syncthreads();                                 // lh zeroed (previous tile written out)
      const uint64_t e0 = (uint64_t)tile * PTILE + threadIdx.x;
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        if (e0 + (uint64_t)j * BLOCK < n)
          atomicAdd(&lh[digit_of_elem<IN>(((uint64_t)cur[j].y << 32) | cur[j].x, g, D, sh)], 1u);
      }
      __syncthreads();
      for (uint32_t d = threadIdx.x; d < R; d += BLOCK) {
        hist[(size_t)d * ntiles + tile] = lh[d];
        lh[d] = 0;
      }
    }
    return;
  }
  // thread t's 8 consecutive elements of a tile, EB bytes each, as NV 16-B words
  constexpr int EB = (int)fmt_key_bytes(IN);
  constexpr int NV = EB == 1 ? 1 : EB / 2;
  uint4 nx[NV];
  auto prefetch = [&](uint32_t tile) {
    if constexpr (EB == 1) {                           // 8 u8 digits: one 8-B load
      const uint2 v = reinterpret_cast<const uint2*>(in)[(uint64_t)tile * (PTILE / 8) + threadIdx.x];
      nx[0] = make_uint4(v.x, v.y, 0u, 0u);
      return;
    }
    const uint4* src = reinterpret_cast<const uint4*>(in) +
                       ((uint64_t)tile * PTILE + 8u * threadIdx.x) / (16 / EB);
#pragma unroll
    for (int v = 0; v < NV; ++v) nx[v] = src[v];
  };
  prefetch(tile_at(0));
  for (uint32_t it = 0; it < n_iter; ++it) {
    const uint32_t tile = tile_at(it);
    uint4 cur[NV];
#pragma unroll
    for (int v = 0; v < NV; ++v) cur[v] = nx[v];
    if (it + 1 < n_iter) prefetch(tile_at(it + 1));
    __syncthreads();                                   // lh zeroed (previous tile written out)
    const uint64_t e0 = (uint64_t)tile * PTILE + 8u * threadIdx.x;
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      if (e0 + j < n) {
        // element j out of the loaded words: u32 word jw of them, or the u64 at words jw, jw + 1
        constexpr int PW = 4 / (EB < 4 ? EB : 4);      // elements per u32 word
        const int jw = EB == 8 ? 2 * j : j / PW;
        const uint4 w = cur[jw >> 2];
        auto word = [&](int i) { return i == 0 ? w.x : i == 1 ? w.y : i == 2 ? w.z : w.w; };
        uint64_t e = word(jw & 3);
        if constexpr (EB == 8) e |= (uint64_t)word((jw & 3) + 1) << 32;
        if constexpr (EB < 4) e = (e >> (8 * EB * (j % PW))) & ((1u << (8 * EB)) - 1u);
        atomicAdd(&lh[digit_of_elem<IN>(e, g, D, sh)], 1u);
      }
    }
    __syncthreads();
    for (uint32_t d = threadIdx.x; d < R; d += BLOCK) {
      hist[(size_t)d * ntiles + tile] = lh[d];
      lh[d] = 0;
    }
  }
}

// V_hll: register-wise max of the histogram workgroups' HLL rows.  V_hll_part: workgroup g
// reduces rows [g * rpw, (g + 1) * rpw) into partial row g (thread t takes packed word t mod 64
// of every 16th row: each row one coalesced 256-B read, eight rows in flight per thread);
// V_hll_final (one workgroup) reduces the partial rows and turns the registers into the estimate
// of distinct keys (Flajolet et al. 2007, linear counting in the small range, x 64 for the
// sample), published to pinned host memory.  Two launches instead of a last-workgroup ticket:
// the ticket's release fence per workgroup (an XCD L2 write-back) cost ~35 us.
__device__ __forceinline__ uint32_t max_u8x4(uint32_t a, uint32_t b) {
  uint32_t r = 0;
#pragma unroll
  for (int j = 0; j < 4; ++j) r |= max((a >> (8 * j)) & 0xFFu, (b >> (8 * j)) & 0xFFu) << (8 * j);
  return r;
}

// rows r0 + q, r0 + q + HLL_RG, ... below r1, word w: eight independent loads per trip
constexpr uint32_t HLL_T = 1024;               // V_hll threads: 16 row groups x 64 words
constexpr uint32_t HLL_RG = HLL_T / 64;
__device__ __forceinline__ uint32_t hll_rows_max(const uint32_t* rows, uint32_t r0, uint32_t r1,
                                                 uint32_t w, uint32_t q) {
  uint32_t m = 0;
  uint32_t r = r0 + q;
  for (; r + 7 * HLL_RG < r1; r += 8 * HLL_RG) {
    uint32_t x[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) x[j] = rows[(size_t)(r + j * HLL_RG) * 64 + w];
#pragma unroll
    for (int j = 0; j < 8; ++j) m = max_u8x4(m, x[j]);
  }
  for (; r < r1; r += HLL_RG) m = max_u8x4(m, rows[(size_t)r * 64 + w]);
  return m;
}

__global__ void __launch_bounds__(HLL_T)
k_v2_hll_part(const uint32_t* __restrict__ rows, uint32_t n_rows, uint32_t* __restrict__ part) {
  __shared__ uint32_t pw[HLL_RG][64];
  const uint32_t w = threadIdx.x & 63, q = threadIdx.x >> 6;
  const uint32_t rpw = (n_rows + gridDim.x - 1) / gridDim.x;
  const uint32_t r0 = blockIdx.x * rpw, r1 = min(n_rows, r0 + rpw);
  pw[q][w] = hll_rows_max(rows, r0, r1, w, q);
  __syncthreads();
  if (q == 0) {
    uint32_t m = 0;
#pragma unroll
    for (uint32_t j = 0; j < HLL_RG; ++j) m = max_u8x4(m, pw[j][w]);
    part[(size_t)blockIdx.x * 64 + w] = m;
  }
}

__global__ void __launch_bounds__(HLL_T)
k_v2_hll_final(const uint32_t* __restrict__ part, uint32_t n_part, double* __restrict__ host_est,
               const uint32_t* __restrict__ n_valid, uint64_t* __restrict__ host_n) {
  __shared__ uint32_t pw[HLL_RG][64];
  __shared__ double zs[HLL_REGS / 64];
  __shared__ uint32_t zc[HLL_REGS / 64];
  const uint32_t w = threadIdx.x & 63, q = threadIdx.x >> 6;
  pw[q][w] = hll_rows_max(part, 0, n_part, w, q);
  __syncthreads();
  if (threadIdx.x < HLL_REGS) {                // one thread per register
    const uint32_t reg = threadIdx.x, wr = reg >> 2, sh = 8 * (reg & 3);
    uint32_t v = 0;
#pragma unroll
    for (uint32_t j = 0; j < HLL_RG; ++j) v = max(v, (pw[j][wr] >> sh) & 0xFFu);
    double z = ldexp(1.0, -(int)v);
    uint32_t zero = v == 0;
    for (int d = 32; d >= 1; d >>= 1) {
      z += __shfl_xor(z, d);
      zero += __shfl_xor(zero, d);
    }
    if (lane_id() == 0) { zs[threadIdx.x >> 6] = z; zc[threadIdx.x >> 6] = zero; }
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    const double mm = HLL_REGS;
    const double zt = zs[0] + zs[1] + zs[2] + zs[3];
    const uint32_t zeros = zc[0] + zc[1] + zc[2] + zc[3];
    double e = 0.7213 / (1.0 + 1.079 / mm) * mm * mm / zt;
    if (e <= 2.5 * mm && zeros) e = mm * log(mm / (double)zeros);
    *host_est = e * (double)(1u << HLL_SAMPLE_BITS);
    if (host_n) *host_n = *n_valid;            // the keys the estimate is set against
  }
}

// ---------------------------------------------------------------- V_bounds_lo
// Bucket starts from the radix histograms instead of a pass over the sorted keys.  With LSD
// passes, pass p's input is sorted by lo = c mod div (c = the element's digits 0 .. p combined,
// div = R^p) and the pass places elements by its own digit hi, stably, so
//   S_p[hi * div + lo] = #(digit < hi) + #(digit == hi and lo' < lo)
//                      = hist_p[hi][t] + #(digit hi among the pass's input [t * PTILE, P_lo))
// where P_lo = S_(p-1)[lo] = #(lo' < lo) is the start of lo in that input (for p = 1 pass 0's
// scanned column 0, saved by V_hist) and t = P_lo / PTILE: one workgroup per lo value counts at
// most one partial tile.  S_p of the last pass are the bucket starts; the earlier levels (3+
// passes) keep S_p (R^(p+1) entries, `nlim`) for the next.  Each level rides in its pass's
// scatter (BoundsFuse) -- it needs that pass's scanned histogram and its input, both live
// there -- so no key pass and no launch of its own.  Interleaved schedule only (one histogram
// column per tile).  `spread` (count-only builds): start[b / spread] for the buckets b that are
// multiples of spread.
// IN = the format of the pass's input `in` (sh: Pack8::sh of a Packed8 stream).
template <StreamFmt IN>
__device__ __forceinline__ void bounds_lo_body(uint32_t lo, uint32_t* cnt,
                                               const void* __restrict__ in, int sh, uint32_t n,
                                               Geom g, Digit Dlast, uint32_t div,
                                               const uint32_t* __restrict__ hist, uint32_t C,
                                               const uint32_t* __restrict__ lo_start,
                                               uint32_t spread, uint32_t* __restrict__ start,
                                               int tb, uint32_t nlim) {
  const uint32_t R = Dlast.R;
  const uint32_t P = lo_start ? lo_start[lo] : 0u;
  for (uint32_t d = threadIdx.x; d < R; d += tb) cnt[d] = 0;
  __syncthreads();
  const uint32_t tile = P / PTILE;
  for (uint32_t i = tile * PTILE + threadIdx.x; i < P; i += tb)
    atomicAdd(&cnt[digit_of_elem<IN>(in, i, g, Dlast, sh)], 1u);
  __syncthreads();
  for (uint32_t hi = threadIdx.x; hi < R; hi += tb) {
    const uint64_t b = (uint64_t)hi * div + lo;
    if (b >= nlim || b % spread) continue;
    // P == n on a tile boundary past the last column: the end of digit hi
    const uint32_t base = tile < C ? hist[(size_t)hi * C + tile]
                                   : (hi + 1 < R ? hist[(size_t)(hi + 1) * C] : n);
    start[b / spread] = base + cnt[hi];
  }
  if (lo == 0 && threadIdx.x == 0) start[nlim / spread] = n;
  __syncthreads();                         // cnt is the caller's LDS: free again
}

// The unfused level (KMHG_FUSE_BOUNDS=0, the last level of a count-only build that picks its
// spread after the passes, one-pass builds): the cold path, so one kernel that switches over the
// format at run time.
__global__ void __launch_bounds__(BLOCK)
k_v2_bounds_lo(StreamFmt fmt, const void* __restrict__ in, int sh,
               const uint32_t* __restrict__ n_ptr, Geom g, Digit Dlast, uint32_t div,
               const uint32_t* __restrict__ hist, uint32_t C,
               const uint32_t* __restrict__ lo_start, uint32_t spread,
               uint32_t* __restrict__ start, uint32_t nlim) {
  __shared__ uint32_t cnt[V2_MAXR];
#define KMHG_LEVEL(F)                                                                          \
  case StreamFmt::F:                                                                           \
    bounds_lo_body<StreamFmt::F>(blockIdx.x, cnt, in, sh, *n_ptr, g, Dlast, div, hist, C,       \
                                 lo_start, spread, start, BLOCK, nlim);                         \
    break
  switch (fmt) {
    KMHG_LEVEL(KeyPos);
    KMHG_LEVEL(Packed12);
    KMHG_LEVEL(Packed8);
    KMHG_LEVEL(BidPos);
    KMHG_LEVEL(DigitPos);
    default: break;            // (Keys arrives as KeyPos; nothing else is a pass's input)
  }
#undef KMHG_LEVEL
}

// ---------------------------------------------------------------- V_scatter (stable)
// Tile t = elements [t*PTILE, (t+1)*PTILE); wave w of the NWV waves owns the contiguous
// PTILE/NWV elements [t*PTILE + w*PTILE/NWV, ...), lane l holds element 64c + l of them.
// Element order inside the tile = (wave, c, lane) = input order, so ranks assigned in that
// order keep the pass stable.  FROM_SEQ (pass 0) encodes the windows from LDS-staged chars and
// drops invalid ones; later passes read the (key, pos) stream.  The tile is re-ordered by digit
// in LDS first and written out run by run, so each wave store covers a few contiguous runs
// instead of 64 scattered addresses.
// Persistent workgroup b walks virtual tiles b, b + G, ...: every XCD owns one contiguous tile
// range (xcd_remap), so the tiles running at the same time on an XCD are neighbours and their
// partial output lines merge in that XCD's L2.  Histograms are per tile; each tile's digit bases
// are prefetched with its inputs.
// (Removed in round 4 after measurement: 8-wave workgroups, +10 % at config 3, and a chunked
// schedule with per-chunk histograms, -10 %: each workgroup's open digit-run heads overflow the
// L2.)
constexpr int SC_NWV = 4;                       // waves per scatter workgroup
// KEY / POS / STG: the pass stages keys / positions / the tile's chars (the two DigitPos passes,
// Bids -> DigitPos and DigitPos -> Pos, drop what they never touch: 33.4 -> 24.1 KB per
// workgroup)
template <class KT, bool KEY = true, bool POS = true, bool STG = true>
struct ScatterLDS {
  static constexpr uint32_t MAXR = V2_MAXR_IL;
  uint32_t wc[SC_NWV][MAXR];   // per-wave digit counts -> per-wave tile-local cursors
  uint32_t tstart[MAXR];       // tile-local start of each digit
  uint32_t gbase[MAXR];        // global start of each digit for this tile (scanned histogram)
  KT skey[KEY ? PTILE : 1];
  uint32_t spos[POS ? PTILE : 1];
  uint32_t sdst[PTILE];
  typename std::conditional<STG, PStage, uint32_t>::type st;
};

// Exclusive scan over the NWV * 64 threads of a block (one value per thread), lds >= NWV u64.
template <int NWV>
__device__ __forceinline__ uint64_t block_excl_scan_n(uint64_t v, uint64_t* lds, uint64_t& total) {
  const int wid = threadIdx.x >> 6;
  const uint64_t inc = wave_incl_scan(v);
  if (lane_id() == 63) lds[wid] = inc;
  __syncthreads();
  uint64_t off = 0, tot = 0;
#pragma unroll
  for (int w = 0; w < NWV; ++w) {
    const uint64_t x = lds[w];
    if (w < wid) off += x;
    tot += x;
  }
  __syncthreads();
  total = tot;
  return off + inc - v;
}

// The same for u32 values whose block total fits 32 bits, the wave scans by DPP (no LDS permutes).
template <int NWV>
__device__ __forceinline__ uint32_t block_excl_scan_n32(uint32_t v, uint64_t* lds, uint64_t& total) {
  const int wid = threadIdx.x >> 6;
  const uint32_t inc = wave_incl_scan_u32(v);
  if (lane_id() == 63) lds[wid] = inc;
  __syncthreads();
  uint64_t off = 0, tot = 0;
#pragma unroll
  for (int w = 0; w < NWV; ++w) {
    const uint64_t x = lds[w];
    if (w < wid) off += x;
    tot += x;
  }
  __syncthreads();
  total = tot;
  return (uint32_t)off + inc - v;
}

// KEYS0: the first pass over a caller's key stream (a table rebuilt from keys): `kin` holds
// exactly n keys (loads clamped, no pad) and positions are implicit (e + 1), so the stream is
// neither copied nor paired with an iota array first.
// IN / OUT: the formats of the pass's input and output (StreamFmt; the sequence and a first
// pass over keys are Keys in: positions implicit).
// Keys out (count-only builds: nobody reads the positions): 8 B per element in and out instead
// of 12.  KeyPos: (key u64, pos) in two arrays.
// BidPos (bucket-id streams, position builds that keep code words): (bucket id u32, pos) -- the
// digit needs no hash, and the key is cut from the code words by the bucket kernel; the last
// pass writes Pos, positions only.  kin / kout then point at u32 arrays.  8 B per element
// instead of 12 through the middle passes, 4 B out of the last.
// DigitPos: the two passes of a two-pass bucket-id build at a radix <= 256 and < 2^24 windows
// carry ONE u32 per window between them, the digit-pos word (pass-1 digit << 24) | pos: Bids ->
// DigitPos (pass 0: V_hist0's ids in, positions implicit) writes the words to kout, nothing to
// pout; DigitPos -> Pos, the last pass, reads them (digit = w >> 24, no division) and writes
// w & 0xFFFFFF to pout.  The pass-0 digit is implied by where the word lies, and the fused
// bucket-start level reads only this pass's digit too.  4 B per window through the middle
// instead of 8, one run per tile and digit instead of two.
// Packed12: (key, pos) elements, 12 B each in kin / kout ({key lo, key hi, pos}; pin / pout
// unused): a tile's digit run leaves as ONE contiguous piece instead of an 8 c-byte piece of
// keys and a 4 c-byte piece of positions in two arrays; KeyPos -> Packed12 is the last pass of a
// build whose earlier streams stay unpacked for their histogram passes.
// Packed8 (Pack8, small k): the first pass from the sequence writes packed 8-B elements, and
// Packed8 -> Packed12, the second pass, reads them (each element's position restored from its
// segment, found in pk.segb by its place in the stream).  Write-pattern probe
// (tools/scatter_pattern.hip layout, profiles/r5a_scatter_layout.txt, 100 M elements): radix 313
// 1.09 -> 0.87 ms, radix 79 0.72 -> 0.61 ms.
// BALLOT: stable ranks from one ballot per digit bit instead of the count atomics' lane-ordered
// returns -- chosen at run time where the device self-check finds that order violated.
// DS (digit stream): the pass also writes every element's digit of the NEXT pass (u16, at the
// element's place in the output), which that pass's histogram reads instead of the keys.
// the (IN, OUT) pairs a pass may be built for (launch_v2_scatter lists the same ones)
constexpr bool scatter_pair_ok(bool from_seq, bool keys0, StreamFmt in, StreamFmt out) {
  using F = StreamFmt;
  if (from_seq)                // the windows: keys with implicit positions
    return !keys0 && in == F::Keys && (out == F::KeyPos || out == F::Packed12 || out == F::Packed8);
  if (keys0)                   // a caller's keys, or V_hist0's ids
    return in == F::Keys ? out == F::Keys || out == F::KeyPos
                         : in == F::Bids &&
                               (out == F::BidPos || out == F::DigitPos || out == F::Pos);
  return (in == F::Keys && out == F::Keys) ||
         (in == F::KeyPos && (out == F::KeyPos || out == F::Packed12)) ||
         ((in == F::Packed12 || in == F::Packed8) && out == F::Packed12) ||
         (in == F::BidPos && (out == F::BidPos || out == F::Pos)) ||
         (in == F::DigitPos && out == F::Pos);
}
template <bool FROM_SEQ, bool KEYS0, StreamFmt IN, StreamFmt OUT, bool BALLOT, bool DS>
__global__ void __launch_bounds__(SC_NWV * 64)
k_v2_scatter(const uint8_t* __restrict__ seq, int64_t L, int k, int64_t Nw,
             const uint64_t* __restrict__ kin, const uint32_t* __restrict__ pin,
             const uint32_t* __restrict__ n_ptr, Geom g, Digit D,
             const uint32_t* __restrict__ hist, uint32_t ntiles,
             uint64_t* __restrict__ kout, uint32_t* __restrict__ pout, uint32_t pad,
             int skip_empty, BoundsFuse bf, Pack8 pk, DigitOut dso) {
  static_assert(scatter_pair_ok(FROM_SEQ, KEYS0, IN, OUT), "not a pair of formats a pass converts");
  static_assert(!DS || (OUT != StreamFmt::Pos && OUT != StreamFmt::DigitPos &&
                        OUT != StreamFmt::Keys), "no digit stream out of these passes");
  constexpr bool DPW0 = OUT == StreamFmt::DigitPos, DPW1 = IN == StreamFmt::DigitPos;
  constexpr bool BIDS = fmt_bid(IN);              // bucket-id streams: u32 words in and out
  constexpr bool KEYOUT = fmt_key_bytes(OUT) != 0;   // the pass writes kout
  constexpr bool POSOUT = fmt_pos_array(OUT);     // ... pout
  constexpr bool POSIN = fmt_pos_array(IN);       // ... reads pin
  constexpr bool AOS = OUT == StreamFmt::Packed12, AIN = IN == StreamFmt::Packed12;
  constexpr bool P8OUT = OUT == StreamFmt::Packed8, P8IN = IN == StreamFmt::Packed8;
  using KT = typename std::conditional<BIDS, uint32_t, uint64_t>::type;
  // staged in LDS: the key unless the pass reads digit-pos words, the position unless it writes
  // them, the chars in neither of the two
  using SL = ScatterLDS<KT, !DPW1, !DPW0, !(DPW0 || DPW1)>;
  const KT* __restrict__ kinT = reinterpret_cast<const KT*>(kin);
  KT* __restrict__ koutT = reinterpret_cast<KT*>(kout);
  constexpr int NWV = SC_NWV;
  constexpr int TB = NWV * 64;                  // threads per workgroup
  constexpr int PER = PTILE / NWV / 64;         // elements per lane
  constexpr int DPT = (int)((SL::MAXR + TB - 1) / TB);   // digits owned per thread
  __shared__ SL S;
  __shared__ uint64_t sh[8];
  const uint32_t R = D.R;
  const int wave = threadIdx.x >> 6, lane = lane_id();
  const uint32_t wbase = (uint32_t)wave * (PTILE / NWV);
  // elements to read: every window (FROM_SEQ) or the caller's whole key stream (KEYS0, passed
  // as Nw: with skip_empty it is longer than the valid count the scan left in *n_ptr)
  const uint64_t n = (FROM_SEQ || KEYS0) ? (uint64_t)Nw : (uint64_t)*n_ptr;
  // thread t owns digits [DPT t, DPT t + DPT)
  const uint32_t G = gridDim.x;
  const uint32_t n_iter = (ntiles - blockIdx.x + G - 1) / G;
  // Each XCD walks its tile range from the END: the histogram pass before this one read the
  // same input ascending, so the tail it read last is still in the Infinity Cache when this
  // pass starts (-DKMHG_NO_REVERSE: ascending, A/B)
#ifndef KMHG_NO_REVERSE
  auto tile_at = [&](uint32_t i) -> uint32_t {
    return xcd_remap(blockIdx.x + (n_iter - 1 - i) * G, ntiles);
  };
#else
  auto tile_at = [&](uint32_t i) -> uint32_t { return xcd_remap(blockIdx.x + i * G, ntiles); };
#endif
  uint32_t ngb[DPT];
  auto load_bases = [&](uint32_t tv) {     // unconditional (clamped) loads: static count
#pragma unroll
    for (int q = 0; q < DPT; ++q) {
      const uint32_t d = min(threadIdx.x * DPT + q, R - 1);
      ngb[q] = hist[(size_t)d * ntiles + tv];
    }
  };
  // the folded bucket-start level, over this pass's own input, before any tile's loads are
  // issued
  if (bf.start)
    for (uint32_t lo = blockIdx.x; lo < bf.div; lo += gridDim.x)
      bounds_lo_body<IN>(lo, &S.wc[0][0], kin, pk.sh, *n_ptr, g, bf.Dlast, bf.div, hist, ntiles,
                         bf.lo_start, bf.spread, bf.start, TB, bf.nlim);
  // the next tile's inputs are in flight while this one is processed
  KT nkey[PER];
  uint32_t npos[PER];
  StageRegs<PSTAGE_W16> nchars;
  auto prefetch = [&](uint32_t tv) {
    const uint64_t t0 = (uint64_t)tv * PTILE;
    load_bases(tv);
    if constexpr (FROM_SEQ) {
      stage_load<PSTAGE_W16, true>(nchars, seq, L, (int64_t)t0 - HALO, true);
    } else {
#pragma unroll
      for (int cc = 0; cc < PER; ++cc) {   // e < ntiles * PTILE <= n_max + pad: in bounds
        const uint64_t e = t0 + wbase + (uint32_t)cc * 64 + lane;
        if (KEYS0) {
          nkey[cc] = kinT[e < n ? e : n - 1];    // positions implicit: e + 1 (below)
        } else if (AIN) {
          const uint3 v = reinterpret_cast<const uint3*>(kin)[e];
          nkey[cc] = ((uint64_t)v.y << 32) | v.x;
          npos[cc] = v.z;
        } else {                               // (Packed8: the position is restored from the
          nkey[cc] = kinT[e];                  // segment table, DigitPos: cut from the word)
          npos[cc] = POSIN ? pin[e] : 0u;
        }
      }
    }
  };
  // Every path into the loop top has [prefetch loads][PTILE/TB x 2 stores] in flight, so the
  // compiler waits for the prefetch with a counted vmcnt: the pad stores below stand in for the
  // previous tile's write-out on the first iteration.
  prefetch(tile_at(0));
#pragma unroll
  for (int j = 0; j < PTILE / TB; ++j) {
    if (AOS) {
      reinterpret_cast<uint3*>(kout)[pad + threadIdx.x] = make_uint3(0u, 0u, 0u);
    } else {
      if (KEYOUT) koutT[pad + threadIdx.x] = 0;
      if (POSOUT) pout[pad + threadIdx.x] = 0;
    }
    if constexpr (DS) {
      if (dso.out8) dso.out8[pad + threadIdx.x] = 0;
      else dso.out[pad + threadIdx.x] = 0;
    }
  }
  for (uint32_t it = 0; it < n_iter; ++it) {
    const uint32_t tile = tile_at(it);
    const uint64_t tile0 = (uint64_t)tile * PTILE;
    KT key[PER];
    uint32_t ps[PER], dg[PER];
    bool act[PER];
    uint32_t cursor[DPT];
#pragma unroll
    for (int q = 0; q < DPT; ++q) cursor[q] = ngb[q];
    if constexpr (FROM_SEQ) {
      stage_pack(nchars, S.st);
    } else {
#pragma unroll
      for (int cc = 0; cc < PER; ++cc) {
        key[cc] = nkey[cc];
        ps[cc] = KEYS0 ? (uint32_t)(tile0 + wbase + (uint32_t)cc * 64 + lane + 1) : npos[cc];
      }
    }
    prefetch(tile_at(min(it + 1, n_iter - 1)));   // unconditional: static vmcnt
    for (uint32_t d = lane; d < R; d += 64) S.wc[wave][d] = 0;
    __syncthreads();                       // stage packed; previous tile's write-out done
#pragma unroll
    for (int c = 0; c < PER; ++c) {
      const uint32_t w = wbase + (uint32_t)c * 64 + lane;     // element index inside the tile
      const uint64_t e = tile0 + w;
      if constexpr (FROM_SEQ) {
        uint64_t kk = 0;
        act[c] = e < n && window_key(S.st, HALO + (int)w, (int64_t)e, L, k, kk);
        ps[c] = (uint32_t)(e + 1);
        const uint64_t h = mix64(kk);
        const uint32_t bl = bucket_local(h, g);
        act[c] = act[c] && bl < g.nb;                        // a part build keeps its buckets
        key[c] = P8OUT ? (KT)((kk << pk.sh) | (e & ((1ull << pk.sh) - 1ull))) : (KT)kk;
        dg[c] = act[c] ? digit_of_b(bl, D) : 0;
      } else {
        // a first pass drops what is no element: V_hist0's ~0 ids, a padded stream's empty keys
        act[c] = e < n && !(KEYS0 && (BIDS ? (uint32_t)key[c] == ~0u
                                           : skip_empty && (uint64_t)key[c] == EMPTY_KEY));
        [[maybe_unused]] const uint64_t src = digit_src<IN>(key[c], pk.sh);
        if constexpr (DPW0) {
          // both digits from one division: this pass's, and the quotient (< R <= 256: two
          // passes) that is the next pass's, packed over the position (< 2^24)
          uint32_t hi;
          const uint32_t lo = digit_of_b_hi((uint32_t)key[c], D, hi);
          dg[c] = act[c] ? lo : 0;
          key[c] = (KT)((hi << BID_POS_BITS) | ps[c]);
        } else {
          dg[c] = act[c] ? digit_of_src<IN>(src, g, D) : 0;
        }
        if constexpr (P8IN) {
          // key and window index from the packed element; the segment from the element's place
          // in its pass-0 digit run (segb row of that digit: the largest s with segb[s] <= e)
          const uint64_t kk = (uint64_t)key[c] >> pk.sh;
          const uint32_t d0 = digit_of_src<IN>(src, g, pk.d0);   // the same hash's pass-0 digit
          const uint32_t* row = pk.segb + (uint64_t)d0 * (pk.nseg + 1);
          uint32_t lo = 0, hi = pk.nseg;                     // row[0] <= e < row[nseg]
          while (hi - lo > 1) {
            const uint32_t mid = (lo + hi) >> 1;
            if ((uint64_t)row[mid] <= e) lo = mid; else hi = mid;
          }
          ps[c] = (uint32_t)((((uint64_t)lo << pk.sh) |
                              ((uint64_t)key[c] & ((1ull << pk.sh) - 1ull))) + 1);
          key[c] = (KT)kk;
        }
        if constexpr (DPW1) ps[c] = (uint32_t)key[c] & ((1u << BID_POS_BITS) - 1u);
      }
    }
    if (!BALLOT) {
      // Stable ranks from the count atomics themselves: the lanes of one LDS instruction that
      // hit the same counter are served in lane order (CDNA4; kmhg_check_lds_lane_order checks
      // it on the device before the first build), and a wave's instructions run in program
      // order, so the returned running count is the element's rank among the wave's elements
      // of its digit in (c, lane) = input order.
      // (the rank rides in the digit's register, bits 16+: digit < 2^16, rank < PTILE)
#pragma unroll
      for (int c = 0; c < PER; ++c)
        if (act[c]) dg[c] |= atomicAdd(&S.wc[wave][dg[c]], 1u) << 16;
    } else {
#pragma unroll
      for (int c = 0; c < PER; ++c)          // counts only: order-free LDS atomics
        if (act[c]) atomicAdd(&S.wc[wave][dg[c]], 1u);
    }
    __syncthreads();
    // tile-local digit starts: thread t owns digits [DPT t, DPT t + DPT)
    uint32_t dsum[DPT];
    uint64_t own = 0;
#pragma unroll
    for (int q = 0; q < DPT; ++q) {
      const uint32_t d = threadIdx.x * DPT + q;
      uint32_t sum = 0;
      if (d < R) {
#pragma unroll
        for (int w = 0; w < NWV; ++w) sum += S.wc[w][d];
      }
      dsum[q] = sum;
      own += sum;
    }
    uint64_t tile_n;
#ifndef KMHG_NO_DPP_SCAN
    uint32_t run = block_excl_scan_n32<NWV>((uint32_t)own, sh, tile_n);   // own <= PTILE
#else
    uint32_t run = (uint32_t)block_excl_scan_n<NWV>(own, sh, tile_n);
#endif
#pragma unroll
    for (int q = 0; q < DPT; ++q) {
      const uint32_t d = threadIdx.x * DPT + q;
      if (d < R) {
        S.tstart[d] = run;
        S.gbase[d] = cursor[q];
        uint32_t cur = run;
#pragma unroll
        for (int w = 0; w < NWV; ++w) {
          const uint32_t t = S.wc[w][d];
          S.wc[w][d] = cur;
          cur += t;
        }
        run += dsum[q];
      }
    }
    __syncthreads();
    if (!BALLOT) {
#pragma unroll
      for (int c = 0; c < PER; ++c) {
        if (act[c]) {
          const uint32_t d = dg[c] & 0xFFFFu;
          const uint32_t ld = S.wc[wave][d] + (dg[c] >> 16);
          if (KEYOUT) S.skey[ld] = key[c];       // the last bucket-id pass writes positions only
          if (!DPW0) S.spos[ld] = ps[c];         // (the digit-pos word holds it)
          S.sdst[ld] = S.gbase[d] + (ld - S.tstart[d]);
        }
      }
    } else {
#pragma unroll
      for (int c = 0; c < PER; ++c) {        // stable ranks: ballots over the digit bits
        const uint64_t grp = match_bits(dg[c], D.nbits, act[c]);
        const int leader = act[c] ? __ffsll((unsigned long long)grp) - 1 : lane;
        uint32_t cur = 0;
        if (act[c] && leader == lane) {
          cur = S.wc[wave][dg[c]];
          S.wc[wave][dg[c]] = cur + (uint32_t)__popcll(grp);
        }
        cur = __shfl(cur, leader);
        wave_sync();
        if (act[c]) {
          const uint32_t ld = cur + (uint32_t)__popcll(grp & lanemask_lt());
          if (KEYOUT) S.skey[ld] = key[c];
          if (!DPW0) S.spos[ld] = ps[c];
          S.sdst[ld] = S.gbase[dg[c]] + (ld - S.tstart[dg[c]]);
        }
      }
    }
    __syncthreads();
    // a static count of store instructions per lane (masked, fully unrolled), so the wait for
    // the next tile's prefetched loads at the loop top is vmcnt(#stores), not vmcnt(0): the
    // prefetch was issued before these stores and must not queue behind their completion
#pragma unroll
    for (int j = 0; j < PTILE / TB; ++j) {
      const uint32_t i = (uint32_t)(j * TB) + threadIdx.x;
      // lanes past the tile's end store into the PTILE-element pad behind the outputs
      const uint32_t dst = i < (uint32_t)tile_n ? S.sdst[i] : pad + threadIdx.x;
      if (AOS) {
        const uint64_t kk = S.skey[i];
        reinterpret_cast<uint3*>(kout)[dst] = make_uint3((uint32_t)kk, (uint32_t)(kk >> 32), S.spos[i]);
      } else {
        if (KEYOUT) koutT[dst] = S.skey[i];
        if (POSOUT) pout[dst] = S.spos[i];
      }
      if constexpr (DS) {       // the next pass's digit, from the staged key (no more LDS)
        const uint32_t dnx = digit_of_elem<OUT>(S.skey[i], g, dso.Dn, pk.sh);
        // (plain stores: the partial lines merge in the XCD's L2; nontemporal digit stores cost
        // the 500 Mbp build 16.86 -> 19.04 ms, profiles/r5y_variants_large_build_only.txt)
        if (dso.out8) dso.out8[dst] = (uint8_t)dnx;
        else dso.out[dst] = (uint16_t)dnx;
      }
    }
  }
}

// Pack8's segment table: segb[d * (nseg + 1) + s] = where segment s (tiles [s tps, (s + 1) tps))
// of pass-0 digit d starts in pass 0's output -- the scanned histogram entry (d, s tps), or the
// end of digit d's run past the last tile.
__global__ void __launch_bounds__(BLOCK)
k_seg_bounds(const uint32_t* __restrict__ hist, uint32_t ntiles, uint32_t R, uint32_t nseg,
             uint32_t tps, const uint32_t* __restrict__ n_valid, uint32_t* __restrict__ segb) {
  const uint32_t i = blockIdx.x * BLOCK + threadIdx.x;
  if (i >= R * (nseg + 1)) return;
  const uint32_t d = i / (nseg + 1), sg = i % (nseg + 1);
  const uint64_t t = (uint64_t)sg * tps;
  segb[i] = t < ntiles ? hist[(size_t)d * ntiles + t]
                       : (d + 1 < R ? hist[(size_t)(d + 1) * ntiles] : *n_valid);
}

// The radix passes are stable by the lane order of the LDS count atomics (V_scatter), so a
// bucket's stream lists its windows in ascending position -- the order the position lists keep.
// The bucket kernels check it with one neighbour load per element and report a violation like
// an LDS table overflow, which rebuilds the index with the global-atomic build (finish_build).
// (pos: the stream's positions, every `stride`-th word: 3 in a packed (key, pos) stream)
template <int STRIDE = 1>
__device__ __forceinline__ bool stream_out_of_order(const uint32_t* __restrict__ pos, uint32_t i,
                                                    uint32_t s0, uint32_t s1, uint32_t p) {
  return i > s0 && i < s1 && pos[(uint64_t)(i - 1) * STRIDE] >= p;
}

// ---------------------------------------------------------------- V_bucket_wg (group per bucket)
// ONE WORKGROUP per bucket (V2_BW_WG windows on average) with one shared LDS sub-table of
// V2_CAPW slots, 12 B per slot (8-B key + one u32 `val`: 18.4 KB, so 8 workgroups fit a CU's
// LDS).  `val` is the count during pass A; the counts pass moves every slot's count into the
// registers of the thread that owns the slot for the write-out (slot q * TB + t), and `val`
// becomes the inline position of a key seen once or the list cursor of a repeated key, tagged
// VAL_MULTI so that pass B can tell them apart.
// Pass A of a one-batch bucket of code-word keys is first tried by placement (home-slot counts,
// one block scan, plain stores: no CAS, no counts pass; see "pass A by placement" below); a
// bucket with a repeated key falls back to the CAS pass.  Measured at config 2, interleaved with
// the parent on one device: headline 44.3 -> 48.2 Gbp/s.  The key-stream and
// packed variants keep the CAS pass (the placement spills VGPRs there).
// (Removed in round 4 after measurement, see DESIGN.md §5: one wave per 256-window bucket, a
// 16-B-per-slot table, 8-wave workgroups, a one-atomic fingerprint insert, a sort-based bucket
// build, and slot tags written by the build.)
struct GroupTableC {
  uint64_t key[V2_CAPW + 1];
  uint32_t val[V2_CAPW + 1];
};
constexpr uint32_t VAL_MULTI = 0x80000000u;    // positions and list offsets are < 2^31

// Find-or-insert by CAS only.  (Measured, 10 Mbp: a plain read before the CAS 0.098 -> 0.186 ms;
// the claiming occurrence skipping its count atomic 0.098 -> 0.136 ms; a per-lane state machine
// over a lane's elements, one CAS per trip, 0.098 -> 0.204 ms.)
__device__ __forceinline__ int lds_insert_g(GroupTableC& W, uint64_t key, uint64_t h) {
  if (key == EMPTY_KEY) return (int)V2_CAPW;
  uint32_t j = local_home(h, V2_CAPW);
  for (uint32_t n = 0; n < V2_CAPW; ++n) {
    const uint64_t prev = atomicCAS((unsigned long long*)&W.key[j],
                                    (unsigned long long)EMPTY_KEY, (unsigned long long)key);
    if (prev == EMPTY_KEY || prev == key) return (int)j;
    if (++j == V2_CAPW) j = 0;
  }
  return -1;
}

__device__ __forceinline__ int lds_find_g(const GroupTableC& W, uint64_t key) {
  if (key == EMPTY_KEY) return (int)V2_CAPW;
  uint32_t j = local_home(mix64(key), V2_CAPW);
  for (uint32_t n = 0; n < V2_CAPW; ++n) {
    if (W.key[j] == key) return (int)j;
    if (++j == V2_CAPW) j = 0;
  }
  return -1;
}

// COUNT_ONLY (occurrence counts of a key stream, kmhg_sh.hip's read counting): pass B -- the
// positions -- is skipped; slots get {key, count, unspecified aux}.
// CK (bucket-id streams): the stream holds positions only; each window's key is cut from the
// sequence's code words (`code`, 16 chars per u32) at its position -- three loads per window
// from a 0.25 B/window array, against 8 B of key per window carried through every radix pass.
// BALLOT: repeated keys' windows ranked by ballots instead of the cursor atomic's lane order.
// Every key must hash to this bucket: a stream entry that does not (an unstable pass moving
// another bucket's window in) is reported like an LDS overflow.
struct Words3 {                                // three consecutive code words, 4-B aligned
  uint32_t a, b, c;
};
// AOS: the stream is packed 12-B (key, pos) elements in `keys` (`pos` unused).
// TAGS (position builds beyond the cache, round 6): the diagonal query path's preparation comes
// with the build -- each slot's tag byte TG[slot] (0 empty, else slot_tag of its key's hash: the
// same bytes V_diag_prep would write), and for every window of a repeated key its bit in `rep`
// (u32 word (pos - 1) / 32, zeroed before the launch), so the first query runs V_diag_valid
// alone (uniq = indexed windows AND NOT rep).
// "Report the bucket as overflowed and leave" (`return bucket_fail(meta);`): a bucket range
// outside the stream, a full table, a key of another bucket or a stream out of position order
// are all reported alike, and the index is rebuilt by the global-atomic build.
__device__ __forceinline__ void bucket_fail(BuildMeta* __restrict__ meta) {
  if (threadIdx.x == 0) atomicOr(&meta->overflow, 1u);
}

// The kernel's phases, in the order k_v2_bucket_wg (below) runs them.  Barriers that separate
// two phases stand in the kernel body; a phase's inner barriers are named in Lds.  Pass A by
// placement alone stays in the kernel body: as a function it spills two VGPRs in the headline
// instance (profiles/bucket_phases_resources.txt).  The LDS objects are static members, used by
// name: through a reference they stay generic pointers until late in the compile.
template <bool COUNT_ONLY, bool CK, bool BALLOT, bool AOS, bool TAGS>
struct BucketPhases {
#define PHASE static __device__ __forceinline__
  static constexpr int TB = BLOCK;
  static constexpr int NW = TB / 64;                  // waves of the workgroup
  // elements per thread per batch: 2x the mean (code words: 1.5x, for the VGPR budget of
  // 8 waves / SIMD); a larger bucket takes more batches
  static constexpr int PER = (CK ? 3 : 4) * V2_BW_WG / 2 / TB;
  static constexpr int EW = (PER + 1) & ~1;           // edge row: PER positions, written as pairs
  static constexpr uint32_t BATCH = TB * PER;
  static constexpr uint32_t SPT = (V2_CAPW + 1 + TB - 1) / TB;   // slots per owner thread

  // The workgroup's LDS: who writes each field, who reads it, and the barrier in between.
  struct Lds {
    // W: table_clear | barrier | pass A (placement or CAS: keys, val = counts) | pass A's
    // verdict barrier | counts pass (val -> owner registers) | its __syncthreads_or | list
    // offsets (val = offset, VAL_MULTI if repeated) | barrier | pass B (val = inline position or
    // cursor) | barrier | write-out.  A placed bucket skips the counts and the offsets; its val
    // holds group starts where no key landed.
    static inline __shared__ GroupTableC W;
    // sh[0, NW): the placement scan's per-wave record, then the list offsets' block scan (which
    // ends in a barrier of its own).  sh[NW, 2 NW): the counts pass's per-wave pair sums, read
    // with the bucket statistics after the offsets -- the upper half, so the scan in between
    // leaves them be.
    static inline __shared__ uint64_t sh[2 * NW];
    // red[0]: the counts pass's keys per wave; red[1]: its maximum count per wave, both read
    // with the bucket statistics behind the counts pass's barriers.  red[1] first carries the
    // placement's per-wave verdict bits, read behind its last barrier; the counts pass of a
    // fallen-back bucket writes it only after the CAS pass's verdict barrier.
    static inline __shared__ uint32_t red[2][NW];
    // edge (stream-order check; none in a count-only build): row `wave` holds that wave's
    // lane-63 positions, EW per row, written and read as pairs -- a handful of LDS instructions
    // per wave: single-lane LDS instructions cost nearly a full one each in this LDS-bound
    // kernel.  order_write fills the rows and zeroes the verdict word edge[EW * NW]; pass A's
    // verdict barrier; order_read sets the verdict.  It is consumed once per bucket, behind the
    // first barrier after order_read: the counts pass's (CAS buckets) or pass B's (placed ones).
    static inline __shared__ __attribute__((aligned(16))) uint32_t edge[EW * NW + 1];
  };
  struct Bucket {                                     // block-uniform, but wave and lane
    uint32_t b, s0, s1;
    int wave, lane;
    __device__ bool one_batch() const { return s1 - s0 <= BATCH; }
    __device__ bool chk() const { return !COUNT_ONLY && one_batch(); }
  };
  // A thread's elements of the current batch, in registers: each phase takes the arrays it
  // reads and writes by reference (every index is a constant once the loops are unrolled).
  using Keys = uint64_t[PER];                         // key[c]
  using Words = uint32_t[PER];                        // ps[c]: positions; wa/wb/wc: code words (CK)
  using Slots = int[PER];                             // slot[c]: the key's LDS slot, -1 if none
  // element c of thread t in a batch: i0 + c * TB + t, so position order = (c, wave, lane)
  PHASE uint32_t elem(uint32_t i0, int c) {
    return i0 + (uint32_t)c * TB + threadIdx.x;
  }

  PHASE void range(const uint32_t* __restrict__ start, Bucket& x) {
    x.b = blockIdx.x;
    x.wave = threadIdx.x >> 6;
    x.lane = lane_id();
    x.s0 = start[x.b];
    x.s1 = start[x.b + 1];
  }

  // CK: load() issues the positions, then the code words, all in flight at once; cut() turns
  // them into keys -- after the table clear for the first batch, so the clear hides the loads.
  // A multi-batch bucket checks its stream order here, with a neighbour load per element.
  PHASE void load(const uint64_t* __restrict__ keys, const uint32_t* __restrict__ pos,
                  const uint32_t* __restrict__ code, uint32_t nw, const Bucket& x, uint32_t i0,
                  Keys& key, Words& ps, Words& wa, Words& wb, Words& wc, bool& disorder) {
    if (CK) {
#pragma unroll
      for (int c = 0; c < PER; ++c) {
        const uint32_t i = elem(i0, c);
        ps[c] = i < x.s1 ? pos[i] : 1u;             // 1-based window start
        if (!x.one_batch()) disorder |= stream_out_of_order(pos, i, x.s0, x.s1, ps[c]);
      }
#pragma unroll
      for (int c = 0; c < PER; ++c) {       // one 12-B load per window (global_load_dwordx3)
        // clamped: a position outside [1, nw] (a stream error, flagged in pass A) never
        // turns into a code-word address outside the array
        const Words3 w3 = *reinterpret_cast<const Words3*>(code + (min(ps[c] - 1u, nw - 1u) >> 4));
        wa[c] = w3.a;
        wb[c] = w3.b;
        wc[c] = w3.c;
      }
      return;
    }
#pragma unroll
    for (int c = 0; c < PER; ++c) {
      const uint32_t i = elem(i0, c);
      if (AOS) {
        const uint3 v = i < x.s1 ? reinterpret_cast<const uint3*>(keys)[i] : make_uint3(0u, 0u, 0u);
        key[c] = ((uint64_t)v.y << 32) | v.x;
        ps[c] = v.z;
      } else {
        key[c] = i < x.s1 ? keys[i] : 0;
        ps[c] = (!COUNT_ONLY && i < x.s1) ? pos[i] : 0;
      }
      if (!COUNT_ONLY && i < x.s1 && ps[c] - 1u >= nw) disorder = true;   // outside [1, nw]
      if (!COUNT_ONLY && !x.one_batch())
        disorder |= AOS ? stream_out_of_order<3>(reinterpret_cast<const uint32_t*>(keys) + 2, i,
                                                    x.s0, x.s1, ps[c])
                          : stream_out_of_order(pos, i, x.s0, x.s1, ps[c]);
    }
  }
  PHASE void cut(const Bucket& x, uint32_t i0, int k, Keys& key, const Words& ps, const Words& wa,
                 const Words& wb, const Words& wc) {
    if (CK) {
#pragma unroll
      for (int c = 0; c < PER; ++c)
        key[c] = elem(i0, c) < x.s1
                       ? code_key(wa[c], wb[c], wc[c], (int64_t)ps[c] - 1, k) : 0;
    }
  }
  // CK: positions in [1, nw] (checked after the cut: fewer live VGPRs)
  PHASE void check_positions(const Bucket& x, uint32_t i0, uint32_t nw, const Words& ps,
                             bool& disorder) {
    if (CK) {
#pragma unroll
      for (int c = 0; c < PER; ++c)
        if (elem(i0, c) < x.s1 && ps[c] - 1u >= nw) disorder = true;
    }
  }

  PHASE void table_clear() {
    for (uint32_t j = threadIdx.x; j <= V2_CAPW; j += TB) {
      Lds::W.key[j] = EMPTY_KEY;
      Lds::W.val[j] = 0u;
    }
  }

  // Stream order of a one-batch bucket: element (c, wave, lane) follows (c, wave, lane - 1) -- a
  // DPP shift -- and lane 0 follows lane 63 of the wave before (of row c - 1 for wave 0),
  // exchanged through `edge` (order_write) and read after a barrier (order_read).  Both run
  // after pass A, when the positions have long arrived, so the check makes no load wait earlier
  // than it did.
  PHASE void order_write(const Bucket& x, const Words& ps, bool& disorder) {
    if (!x.chk()) return;
    if (threadIdx.x == 0) Lds::edge[EW * NW] = 0u;
#pragma unroll
    for (int c = 0; c < PER; ++c) {
      // lane - 1's position by a DPP wave shift (a VALU move; __shfl_up is an LDS permute)
      const uint32_t up = (uint32_t)__builtin_amdgcn_update_dpp(0, (int)ps[c], 0x138 /* wave_shr:1 */,
                                                                0xF, 0xF, false);
      if (x.lane > 0 && elem(x.s0, c) < x.s1 && up >= ps[c]) disorder = true;
    }
    if (x.lane == 63) {
#pragma unroll
      for (int q = 0; q < PER; q += 2)
        *reinterpret_cast<uint2*>(&Lds::edge[EW * x.wave + q]) =
            make_uint2(ps[q], q + 1 < PER ? ps[q + 1] : 0u);
    }
  }
  PHASE void order_read(const Bucket& x, const Words& ps) {
    if (!(x.chk() && x.lane == 0)) return;
    // lane 0 of wave w follows lane 63 of wave w - 1 (same row); wave 0 follows wave NW - 1
    const uint32_t* row = Lds::edge + EW * (x.wave ? x.wave - 1 : NW - 1);
    uint32_t pv[PER + 1];
#pragma unroll
    for (int q = 0; q < PER; q += 2) {
      const uint2 v = *reinterpret_cast<const uint2*>(&row[q]);
      pv[q] = v.x;
      pv[q + 1] = v.y;
    }
    bool bad = false;
#pragma unroll
    for (int c = 0; c < PER; ++c) {
      const uint32_t e = elem(x.s0, c);
      const uint32_t prev = x.wave ? pv[c] : (c ? pv[c - 1] : 0u);   // wave 0: row c - 1
      bad |= e > x.s0 && e < x.s1 && prev >= ps[c];
    }
    if (bad) Lds::edge[EW * NW] = 1u;           // read after the next barrier
  }
  PHASE bool order_verdict(const Bucket& x) {
    return x.chk() && Lds::edge[EW * NW];
  }
  // pass A by CAS, one batch: distinct keys + counts (CAS on a table shared by the four waves).
  // (Measured round 3, A/B in one run: letting the claiming occurrence skip the count add --
  // counts pass adds 1 per occupied slot -- made the kernel 100 -> 142 us, as in round 2; and
  // issuing the first CAS of all 8 elements of a lane back to back before resolving any,
  // 98 -> 112 us.)
  PHASE void pass_a_cas(const Bucket& x, Geom g, uint32_t nw, uint32_t i0, const Keys& key,
                        const Words& ps, Slots& slot, bool& ovf, bool& disorder) {
#pragma unroll
    for (int c = 0; c < PER; ++c) {
      slot[c] = -1;
      if (elem(i0, c) < x.s1) {
        // bucket membership (one multiply-high: CK keys are cut from the code words at the
        // stream's positions, so this checks the positions too)
        const uint64_t h = mix64(key[c]);
        if (bucket_local(h, g) != x.b) disorder = true;
        slot[c] = lds_insert_g(Lds::W, key[c], h);
        if (slot[c] < 0) ovf = true;
        else atomicAdd(&Lds::W.val[slot[c]], 1u);
      }
    }
    check_positions(x, i0, nw, ps, disorder);
  }

  // counts: thread t owns slots t, t + TB, ... (lane-contiguous: conflict-free LDS; thread-
  // contiguous runs of 6 slots ran 0.104 ms against 0.096 for the kernel).  Returns whether some
  // key is repeated (block-uniform).
  // The bucket's distinct keys by ballots (no cross-lane shuffles: each __shfl_xor is an LDS
  // permute, in a kernel bound by its LDS instructions); the count maximum and the pairs only
  // when some key is repeated, which the i.i.d. buckets of a large build almost never have.
  PHASE bool counts(const Bucket& x, uint32_t (&cnt)[SPT], uint32_t& cs) {
    uint32_t occ_w = 0;                      // wave-uniform
    bool multi = false;
#pragma unroll
    for (uint32_t q = 0; q < SPT; ++q) {
      const uint32_t j = q * TB + threadIdx.x;
      const uint32_t c = j <= V2_CAPW ? Lds::W.val[j] : 0u;
      cnt[q] = c;
      cs += c;
      multi |= c > 1;
      occ_w += (uint32_t)__popcll(__ballot(c != 0));
    }
    if (x.lane == 0) Lds::red[0][x.wave] = occ_w;
    const bool has_multi = __syncthreads_or(multi);
    if (has_multi) {                         // block-uniform
      uint32_t mx = 0;
      uint64_t pairs = 0;
#pragma unroll
      for (uint32_t q = 0; q < SPT; ++q) {
        mx = max(mx, cnt[q]);
        pairs += (uint64_t)cnt[q] * (cnt[q] - (cnt[q] ? 1u : 0u)) / 2;
      }
      for (int d = 32; d >= 1; d >>= 1) {
        pairs += __shfl_xor(pairs, d);
        mx = max(mx, (uint32_t)__shfl_xor(mx, d));
      }
      if (x.lane == 0) {
        Lds::red[1][x.wave] = mx;
        Lds::sh[NW + x.wave] = pairs;
      }
      __syncthreads();
    }
    return has_multi;
  }
  // list offsets (only repeated keys have lists): any slot order gives each key a contiguous
  // range of [s0, s1), here slot q * TB + t in (t, q) order
  PHASE void list_offsets(const Bucket& x, const uint32_t (&cnt)[SPT], uint32_t cs) {
    uint64_t tot;
    uint32_t off_run = x.s0 + (uint32_t)block_excl_scan_n<NW>(cs, Lds::sh, tot);
#pragma unroll
    for (uint32_t q = 0; q < SPT; ++q) {
      const uint32_t j = q * TB + threadIdx.x;
      if (j <= V2_CAPW) Lds::W.val[j] = cnt[q] > 1 ? (VAL_MULTI | off_run) : off_run;
      off_run += cnt[q];
    }
  }
  // the bucket's statistics, from the counts pass's per-wave partials
  PHASE void write_stats(const Bucket& x, bool placed, bool has_multi,
                         BucketStats* __restrict__ bstats) {
    if (threadIdx.x != 0) return;
    BucketStats st;
    st.n_kmers = 0;
    st.max_count = 0;
    st.n_pairs = 0;
    if (placed) {                            // no repeated key: every window is a key
      st.n_kmers = x.s1 - x.s0;
      st.max_count = x.s1 > x.s0 ? 1u : 0u;
      bstats[x.b] = st;
      return;
    }
#pragma unroll
    for (int w = 0; w < NW; ++w) st.n_kmers += Lds::red[0][w];
    if (!has_multi) {
      st.max_count = st.n_kmers ? 1u : 0u;
    } else {
#pragma unroll
      for (int w = 0; w < NW; ++w) {
        st.max_count = max(st.max_count, Lds::red[1][w]);
        st.n_pairs += Lds::sh[NW + w];
      }
    }
    bstats[x.b] = st;
  }

  // pass B, one batch whose slots are known.  Keys seen once keep their position inline (val) ...
  PHASE void pass_b_inline(const Bucket& x, uint32_t i0, const Slots& slot, const Words& ps) {
#pragma unroll
    for (int c = 0; c < PER; ++c)
      if (elem(i0, c) < x.s1) Lds::W.val[slot[c]] = ps[c];
  }
  // ... repeated keys are ranked in position order, the waves taking turns so that wave w
  // follows waves < w (a barrier per turn)
  PHASE void pass_b_rank(const Bucket& x, uint32_t i0, const Slots& slot, const Words& ps,
                         int32_t* __restrict__ positions, uint32_t* __restrict__ rep) {
    for (int c = 0; c < PER; ++c) {
      const bool act = elem(i0, c) < x.s1;
      // waves take turns on this c: wave w ranks after waves < w have advanced the cursors
      for (int turn = 0; turn < NW; ++turn) {
        if (x.wave == turn) {
          const uint32_t v = act ? Lds::W.val[slot[c]] : 0u;
          const bool multi = act && (v & VAL_MULTI);
          if (act && !multi) Lds::W.val[slot[c]] = ps[c];
          if (!BALLOT) {
            // the cursor atomic's lane-ordered returns rank the wave's windows of one key
            if (multi) {
              const uint32_t at = atomicAdd(&Lds::W.val[slot[c]], 1u) & ~VAL_MULTI;
              positions[at] = (int32_t)ps[c];
              if (TAGS) atomicOr(&rep[(ps[c] - 1u) >> 5], 1u << ((ps[c] - 1u) & 31u));
            }
          } else if (__ballot(multi)) {
            const uint64_t m = match_bits((uint32_t)slot[c], V2_SLOT_BITS_WG, multi);
            const int leader = multi ? __ffsll((unsigned long long)m) - 1 : x.lane;
            if (multi && leader == x.lane) Lds::W.val[slot[c]] = v + (uint32_t)__popcll(m);
            const uint32_t cur = (uint32_t)__shfl((int)v, leader) & ~VAL_MULTI;
            if (multi) positions[cur + (uint32_t)__popcll(m & lanemask_lt())] = (int32_t)ps[c];
            if (TAGS && multi) atomicOr(&rep[(ps[c] - 1u) >> 5], 1u << ((ps[c] - 1u) & 31u));
          }
        }
        __syncthreads();
      }
    }
  }

  // the bucket's sub-table, coalesced 16-B slots, counts from the registers of the slot's owner
  // (a placed bucket had no counts pass: every occupied slot counts 1, taken from the key)
  PHASE void write_table(const Bucket& x, bool placed, const uint32_t (&cnt)[SPT],
                         Slot* __restrict__ T, uint8_t* __restrict__ TG) {
    Slot* Tb = T + (uint64_t)x.b * V2_CAPW;
#pragma unroll
    for (uint32_t q = 0; q < SPT; ++q) {
      const uint32_t j = q * TB + threadIdx.x;
      if (j < V2_CAPW) {
        const uint64_t kk = Lds::W.key[j];
        // placed: val holds the group starts where no key landed
        const uint32_t cq = placed ? (kk != EMPTY_KEY ? 1u : 0u) : cnt[q];
        const uint32_t aux = COUNT_ONLY ? 0u : (placed && kk == EMPTY_KEY) ? 0u : (Lds::W.val[j] & ~VAL_MULTI);
        if (CK) {
          // code-word keys: the table streams past the L2 (nontemporal), which keeps the code
          // words every bucket gathers from resident there
          typedef unsigned int u32x4 __attribute__((ext_vector_type(4)));
          const u32x4 sv = {(uint32_t)kk, (uint32_t)(kk >> 32), cq, aux};
          __builtin_nontemporal_store(sv, reinterpret_cast<u32x4*>(&Tb[j]));
        } else {
          *reinterpret_cast<uint4*>(&Tb[j]) = make_uint4((uint32_t)kk, (uint32_t)(kk >> 32), cq, aux);
        }
        if (TAGS)      // one byte per slot: 64 consecutive bytes per wave and row q
          TG[(uint64_t)x.b * V2_CAPW + j] = kk == EMPTY_KEY ? (uint8_t)0 : slot_tag(mix64(kk));
      }
    }
  }
  PHASE void write_side(const Bucket& x, Geom g, bool placed, uint32_t n_real,
                        const uint32_t (&cnt)[SPT], Slot* __restrict__ T) {
    if (threadIdx.x == 0 && side_bucket(x.b, g)) {
      // (placed: the windows that are not among the table's keys hold the sentinel key)
      const uint2 c = make_uint2(placed ? x.s1 - x.s0 - n_real : cnt[V2_CAPW / TB],
                                 COUNT_ONLY ? 0u : (Lds::W.val[V2_CAPW] & ~VAL_MULTI));
      *reinterpret_cast<uint4*>(&T[side_slot(g)]) = make_uint4(0xFFFFFFFFu, 0xFFFFFFFFu, c.x, c.y);
    }
  }
#undef PHASE
};

template <bool COUNT_ONLY, bool CK, bool BALLOT, bool AOS = false, bool TAGS = false>
__global__ void __launch_bounds__(BLOCK, BALLOT ? 4 : KMHG_BUCKET_WGS)
k_v2_bucket_wg(const uint64_t* __restrict__ keys, const uint32_t* __restrict__ pos,
               const uint32_t* __restrict__ start, Geom g, Slot* __restrict__ T,
               int32_t* __restrict__ positions, BucketStats* __restrict__ bstats,
               BuildMeta* __restrict__ meta, const uint32_t* __restrict__ code, int k,
               const uint32_t* __restrict__ n_ptr, uint32_t nw, uint8_t* __restrict__ TG,
               uint32_t* __restrict__ rep, uint32_t place, uint32_t* __restrict__ place_ctr) {
  static_assert(!(CK && COUNT_ONLY), "code-word keys belong to position builds");
  static_assert(!(TAGS && (CK || COUNT_ONLY)), "build-time tags: key-stream position builds");
  static_assert(!(AOS && (CK || COUNT_ONLY)), "packed streams carry keys and positions");
  static_assert(V2_CAPW % BLOCK == 0, "the side slot V2_CAPW is slot q = V2_CAPW / TB of thread 0");
  using P = BucketPhases<COUNT_ONLY, CK, BALLOT, AOS, TAGS>;
  constexpr int TB = P::TB, NW = P::NW, PER = P::PER;
  constexpr uint32_t BATCH = P::BATCH;
  using S = typename P::Lds;
  typename P::Bucket x;
  P::range(start, x);
  const uint32_t b = x.b, s0 = x.s0, s1 = x.s1;
  const int wave = x.wave, lane = x.lane;
  // a bucket range outside the stream (a bounds error) is never dereferenced
  if (s0 > s1 || s1 > *n_ptr) return bucket_fail(meta);
  const bool one_batch = x.one_batch();
  uint64_t key[PER];
  uint32_t ps[PER];
  int slot[PER];
  uint32_t wa[PER], wb[PER], wc[PER];                 // CK: each window's three code words
  bool ovf = false;                                   // LDS table full
  bool disorder = false;                              // the bucket's stream out of position order
  STAMP_WG(b, 0);
  // the first batch: its loads are in flight while the table is cleared
  P::load(keys, pos, code, nw, x, s0, key, ps, wa, wb, wc, disorder);
  P::table_clear();
  __syncthreads();
  P::cut(x, s0, k, key, ps, wa, wb, wc);
  STAMP_WG(b, 1);
  STAMP_WG_DRAIN(b, 6);
  // pass A by placement (one-batch position buckets): a linear-probing layout is fixed by how
  // many keys have each home slot, so a bucket WITHOUT a repeated key -- every bucket of an
  // i.i.d. sequence -- needs no find-or-insert: one u32 LDS add per element counts the keys of
  // its home and ranks the element among them (r), a block scan over the homes turns the counts
  // c(h) into the start of each home's group in the table that inserting the keys in home order
  // would give, and each element stores its key at start + r.  With S the exclusive prefix sum
  // of c and M(h) = max(0, max_{j <= h}(j - S(j))), home h's group starts at p(h) = S(h) + M(h)
  // (p(h) = max(h, p(h-1) + c(h-1))).  The last cluster may run past the end by
  // over = max(0, n + M(last) - CAPW) slots, which wrap into [0, over) and push the first
  // cluster: p'(h) = S(h) + max(M(h), over).  The pushed layout reaches the end again only if
  // over > M(last), that is n > CAPW -- a bucket the CAS pass reports as full.  A repeated key
  // shows as two equal keys in one home's group (each element reads the group members of lower
  // rank); such a bucket, or one with a crowded home (so no element reads more than CROWD - 1
  // keys), clears the table and takes the CAS pass below, which stays the one place that
  // handles repeats.  Homes are scanned thread-contiguous (V2_CAPW / TB per thread).
  bool placed = false;                                // block-uniform
  uint32_t n_real = 0;                                // placed: the bucket's keys but the sentinel
  // (code-word keys only: the key-stream and packed variants, 8 elements per thread, spill 9-10
  // VGPRs to scratch at 8 workgroups per CU with this path compiled in, so they keep the CAS pass)
  if (CK && one_batch && place) {
    constexpr uint32_t HB = V2_SLOT_BITS_WG, HM = (1u << HB) - 1u;
    constexpr uint32_t HPT = V2_CAPW / TB;            // homes per thread
    static_assert(HPT % 2 == 0 && (sizeof(S::W.key) % 8) == 0, "the scan reads counts as pairs");
    static_assert(BATCH < (1u << (32 - HB - 1)), "(home, rank) packs into slot[c]");
    constexpr uint32_t CROWD = 8, OFF = 2048;         // OFF >= BATCH keeps j + OFF - S(j) >= 0
    static_assert(BATCH <= OFF && V2_CAPW + OFF < 0x10000u, "the scan's per-wave record: 16-bit fields");
    bool rpt = false;
#pragma unroll
    for (int c = 0; c < PER; ++c) {
      slot[c] = -1;
      if (P::elem(s0, c) < s1) {
        const uint64_t h = mix64(key[c]);
        if (bucket_local(h, g) != b) disorder = true;
        if (key[c] == EMPTY_KEY) {                    // the side slot holds one key
          rpt |= atomicAdd(&S::W.val[V2_CAPW], 1u) != 0u;
          slot[c] = (int)V2_CAPW;
        } else {
          const uint32_t home = local_home(h, V2_CAPW);
          slot[c] = (int)(home | (atomicAdd(&S::W.val[home], 1u) << HB));
        }
      }
    }
    P::check_positions(x, s0, nw, ps, disorder);
    __syncthreads();
    uint32_t cn[HPT];
    uint2* vp = reinterpret_cast<uint2*>(&S::W.val[HPT * threadIdx.x]);
#pragma unroll
    for (uint32_t i = 0; i < HPT; i += 2) {
      const uint2 v = vp[i / 2];
      cn[i] = v.x;
      cn[i + 1] = v.y;
    }
    uint32_t ls = 0, tmax = 0;
    bool crowded = false;
#pragma unroll
    for (uint32_t i = 0; i < HPT; ++i) {              // j + OFF - (S(j) inside the thread)
      tmax = max(tmax, HPT * threadIdx.x + i + OFF - ls);
      ls += cn[i];
      crowded |= cn[i] > CROWD;
    }
    const uint32_t inc = wave_incl_scan_u32(ls);      // S inside the wave
    const uint32_t wex = inc - ls;
    const uint32_t minc = wave_incl_max(tmax - wex);  // j + OFF - (S(j) inside the wave)
    const uint32_t mex = (uint32_t)__builtin_amdgcn_update_dpp(0, (int)minc, 0x138 /* wave_shr:1 */,
                                                               0xF, 0xF, false);
    const bool wcrowd = __ballot(crowded) != 0;
    if (lane == 63) S::sh[wave] = (uint64_t)inc | ((uint64_t)minc << 16) | ((uint64_t)wcrowd << 32);
    __syncthreads();
    int wbase = 0, Mw = 0, Mall = 0, ntot = 0;
    bool crowd = false;
#pragma unroll
    for (int w = 0; w < NW; ++w) {
      const uint64_t x = S::sh[w];
      const int G = (int)((uint32_t)(x >> 16) & 0xFFFFu) - (int)OFF - ntot;
      if (w < wave) {
        Mw = max(Mw, G);
        wbase = ntot + (int)((uint32_t)x & 0xFFFFu);
      }
      Mall = max(Mall, G);
      ntot += (int)((uint32_t)x & 0xFFFFu);
      crowd |= (x >> 32) != 0;
    }
    n_real = (uint32_t)__builtin_amdgcn_readfirstlane(ntot);
    int which = crowd ? 1 : 2;                        // fallback: a repeat / a second wrap
    if (!crowd && n_real <= V2_CAPW) {                // block-uniform
      which = 1;
      const int over = max(0, ntot + Mall - (int)V2_CAPW);
      int m = max(Mw, (int)mex - (int)OFF - wbase);   // (lane 0: mex = 0, below every term)
      int sx = wbase + (int)wex;
#pragma unroll
      for (uint32_t i = 0; i < HPT; ++i) {
        m = max(m, (int)(HPT * threadIdx.x + i) - sx);
        const uint32_t c = cn[i];
        cn[i] = (uint32_t)(sx + max(m, over));        // p'(h) in [0, 2 CAPW)
        sx += (int)c;
      }
#pragma unroll
      for (uint32_t i = 0; i < HPT; i += 2) vp[i / 2] = make_uint2(cn[i], cn[i + 1]);
      __syncthreads();
#pragma unroll
      for (int c = 0; c < PER; ++c) {
        if (P::elem(s0, c) < s1 && slot[c] != (int)V2_CAPW) {
          const uint32_t r = (uint32_t)slot[c] >> HB;
          uint32_t j = S::W.val[(uint32_t)slot[c] & HM] + r;
          if (j >= V2_CAPW) j -= V2_CAPW;
          S::W.key[j] = key[c];
          slot[c] = (int)(j | (r << HB));
        }
      }
      P::order_write(x, ps, disorder);
      __syncthreads();
#pragma unroll
      for (int c = 0; c < PER; ++c) {
        if (P::elem(s0, c) < s1) {
          const uint32_t r = (uint32_t)slot[c] >> HB, j = (uint32_t)slot[c] & HM;
          uint32_t q = j >= r ? j - r : j + V2_CAPW - r;   // the group's first slot
          for (uint32_t i = 0; i < r; ++i) {          // r < CROWD; addresses known up front
            rpt |= S::W.key[q] == key[c];
            if (++q == V2_CAPW) q = 0;
          }
          slot[c] = (int)j;
        }
      }
      // one reduction for both verdicts: bit 0 a repeated key, bit 1 a stream error
      const uint32_t wf = (__ballot(rpt) ? 1u : 0u) | (__ballot(ovf || disorder) ? 2u : 0u);
      if (lane == 0) S::red[1][wave] = wf;
      __syncthreads();
      uint32_t bf = 0;
#pragma unroll
      for (int w = 0; w < NW; ++w) bf |= S::red[1][w];
      if (bf & 2u) return bucket_fail(meta);
      if (!(bf & 1u)) {
        placed = true;
        which = 0;
        P::order_read(x, ps);
      }
    }
    if (!placed) {                                    // nobody reads the table past the barriers above
      P::table_clear();
      __syncthreads();
    }
    // test build only: buckets placed / fallen back for a repeat / for a second wrap
    if (place_ctr && threadIdx.x == 0) atomicAdd(&place_ctr[which], 1u);
  }
  // pass A by CAS, batch by batch (none if the bucket was placed)
  for (uint32_t i0 = s0; i0 < (placed ? s0 : s1); i0 += BATCH) {
    if (i0 != s0) {
      P::load(keys, pos, code, nw, x, i0, key, ps, wa, wb, wc, disorder);
      P::cut(x, i0, k, key, ps, wa, wb, wc);
    }
    P::pass_a_cas(x, g, nw, i0, key, ps, slot, ovf, disorder);
  }
  if (!placed) {
    P::order_write(x, ps, disorder);
    if (__syncthreads_or(ovf || disorder)) return bucket_fail(meta);
    P::order_read(x, ps);              // its verdict: read after the counts pass's barrier
  }
  STAMP_WG(b, 2);
  constexpr uint32_t SPT = P::SPT;
  uint32_t cnt[SPT];
  uint32_t cs = 0;
  bool has_multi = false;
  if (!placed) {
    has_multi = P::counts(x, cnt, cs);
    // stream out of order at a wave / row boundary
    if (P::order_verdict(x)) return bucket_fail(meta);
  }
  if (!COUNT_ONLY && has_multi) {
    P::list_offsets(x, cnt, cs);
    __syncthreads();
  }
  STAMP_WG(b, 3);
  P::write_stats(x, placed, has_multi, bstats);
  // pass B, batch by batch
  for (uint32_t i0 = s0; i0 < (COUNT_ONLY ? s0 : s1); i0 += BATCH) {
    if (!one_batch) {
      P::load(keys, pos, code, nw, x, i0, key, ps, wa, wb, wc, disorder);
      P::cut(x, i0, k, key, ps, wa, wb, wc);
#pragma unroll
      for (int c = 0; c < PER; ++c) slot[c] = P::elem(i0, c) < s1 ? lds_find_g(S::W, key[c]) : -1;
    }
    if (!has_multi) P::pass_b_inline(x, i0, slot, ps);   // every key seen once
    else P::pass_b_rank(x, i0, slot, ps, positions, rep);
  }
  __syncthreads();
  // (placed: order_read's verdict, behind pass B's barrier)
  if (placed && P::order_verdict(x)) return bucket_fail(meta);
  STAMP_WG(b, 4);
  P::write_table(x, placed, cnt, T, TG);
  P::write_side(x, g, placed, n_real, cnt, T);
  STAMP_WG(b, 5);
}

// V_stats: reduce the per-bucket partials (grid-stride, one atomic per workgroup; meta was
// zeroed by V_hist0).  The last workgroup to finish copies the totals into `host_meta`, a
// pinned host record, so the host reads them without a copy launch.
constexpr int STATS_PER = 8;
__global__ void __launch_bounds__(BLOCK)
k_v2_stats(const BucketStats* __restrict__ bs, uint32_t nb, const uint32_t* __restrict__ n_valid,
           BuildMeta* __restrict__ meta, BuildMeta* __restrict__ host_meta) {
  __shared__ uint64_t su[4], sp[4];
  __shared__ uint32_t sm[4];
  uint64_t u = 0, p = 0;
  uint32_t m = 0;
  // STATS_PER buckets per thread and trip, their loads all in flight before any is summed (a
  // plain grid-stride loop waits out one load latency per bucket)
  const uint32_t stride = gridDim.x * BLOCK;
  for (uint32_t b0 = blockIdx.x * BLOCK + threadIdx.x; b0 < nb; b0 += stride * STATS_PER) {
    BucketStats x[STATS_PER];
#pragma unroll
    for (int q = 0; q < STATS_PER; ++q) {
      const uint32_t b = b0 + q * stride;
      x[q] = b < nb ? bs[b] : BucketStats{0u, 0u, 0ull};
    }
#pragma unroll
    for (int q = 0; q < STATS_PER; ++q) {
      u += x[q].n_kmers;
      p += x[q].n_pairs;
      m = max(m, x[q].max_count);
    }
  }
  u = wave_sum(u);
  p = wave_sum(p);
  m = (uint32_t)lane63(wave_incl_max(m));
  const int w = threadIdx.x >> 6;
  if (lane_id() == 0) { su[w] = u; sp[w] = p; sm[w] = m; }
  __syncthreads();
  if (threadIdx.x == 0) {
    u = su[0] + su[1] + su[2] + su[3];
    p = sp[0] + sp[1] + sp[2] + sp[3];
    m = max(max(sm[0], sm[1]), max(sm[2], sm[3]));
    if (u) atomicAdd((unsigned long long*)&meta->n_kmers, (unsigned long long)u);
    if (p) atomicAdd((unsigned long long*)&meta->n_pairs, (unsigned long long)p);
    if (m) atomicMax(&meta->max_count, m);
    __threadfence();
    const uint32_t done = atomicAdd(&meta->blocks_done, 1u);
    if (done == gridDim.x - 1) {           // every other block's atomics are visible
      __threadfence();
      BuildMeta r;
      r.n_kmers = __hip_atomic_load(&meta->n_kmers, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      r.n_pairs = __hip_atomic_load(&meta->n_pairs, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      r.max_count = __hip_atomic_load(&meta->max_count, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      r.overflow = __hip_atomic_load(&meta->overflow, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      r.n_positions = *n_valid;
      r.n_small = 0;
      r.n_large = 0;
      r.blocks_done = done + 1;
      r.distinct_est = 0;
      *host_meta = r;
      __threadfence_system();
    }
  }
}

#ifdef KMHG_STAMPS
void set_stamp_buffer(uint64_t* p) { (void)hipMemcpyToSymbol(HIP_SYMBOL(g_stamps), &p, sizeof(p)); }
#endif

// ---------------------------------------------------------------- V_part_dense
// A part build's compacted tiles (V_hist0 PARTC) into one dense stream: tile t's off[t+1] -
// off[t] elements (off = the scanned tile counts, off[ntiles] = *n_total) move from
// [t * PTILE, ...) to [off[t], ...), keys and positions, order kept.
// AOS: the dense stream is packed 12-B (key, pos) elements in dk (dp unused).
template <bool AOS>
__global__ void __launch_bounds__(BLOCK)
k_part_dense(const uint64_t* __restrict__ ck, const uint32_t* __restrict__ cp,
             const uint32_t* __restrict__ off, uint32_t ntiles,
             const uint32_t* __restrict__ n_total, uint64_t* __restrict__ dk,
             uint32_t* __restrict__ dp) {
  for (uint32_t t = blockIdx.x; t < ntiles; t += gridDim.x) {
    const uint32_t o0 = off[t], o1 = t + 1 < ntiles ? off[t + 1] : *n_total;
    const uint64_t src = (uint64_t)t * PTILE;
    for (uint32_t i = threadIdx.x; i < o1 - o0; i += BLOCK) {
      if (AOS) {
        const uint64_t kk = ck[src + i];
        reinterpret_cast<uint3*>(dk)[o0 + i] = make_uint3((uint32_t)kk, (uint32_t)(kk >> 32), cp[src + i]);
      } else {
        dk[o0 + i] = ck[src + i];
        dp[o0 + i] = cp[src + i];
      }
    }
  }
}

// ---------------------------------------------------------------- launchers
// Persistent grids: as many workgroups as are resident at once (CUs x the occupancy the
// kernel's VGPR/LDS budget allows), so no workgroup waits for another to finish.
static unsigned resident_blocks(const void* kernel, int threads = BLOCK) {
  int dev = 0, cus = 256, per = 1;
  if (hipGetDevice(&dev) == hipSuccess)
    (void)hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev);
  if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&per, kernel, threads, 0) != hipSuccess ||
      per < 1)
    per = 1;
  return (unsigned)(cus > 0 ? cus : 256) * (unsigned)per;
}

static inline unsigned grid_of(uint64_t n, unsigned per) {
  uint64_t g = (n + per - 1) / per;
  return (unsigned)(g ? g : 1);
}

// The lane order of same-address LDS atomics, checked once per device (kmhg_check_lds_lane_order
// runs the same kernel for the tests): where it does not hold, every build takes the ballot-rank
// kernels.  KMHG_TEST_BALLOT=1 (tests) forces them.
bool ballot_ranks();

void launch_v2_hist0(const uint8_t* seq, int64_t L, int k, int64_t Nw, Geom g, Digit D,
                     uint32_t* hist, uint32_t ntiles, uint64_t* scan_status, uint32_t n_status,
                     BuildMeta* meta, hipStream_t s, uint32_t* code, uint16_t* nbit,
                     uint32_t* bids, uint64_t* ckeys, uint32_t* cpos, uint32_t* tcnt) {
  if (ckeys) {                 // a part build's compacted windows (keep the code words)
    static const unsigned cap_p = resident_blocks((const void*)k_v2_hist0p<true, false, true>);
    hipLaunchKernelGGL((k_v2_hist0p<true, false, true>), dim3(std::min<unsigned>(ntiles, cap_p)),
                       dim3(BLOCK), 0, s, seq, L, k, Nw, g, D, hist, ntiles, scan_status,
                       n_status, meta, code, nbit, nullptr, ckeys, cpos, tcnt);
  } else if (bids) {           // bucket-id builds (keep the code words)
    static const unsigned cap_b = resident_blocks((const void*)k_v2_hist0p<true, true>);
    hipLaunchKernelGGL((k_v2_hist0p<true, true>), dim3(std::min<unsigned>(ntiles, cap_b)),
                       dim3(BLOCK), 0, s, seq, L, k, Nw, g, D, hist, ntiles, scan_status,
                       n_status, meta, code, nbit, bids, nullptr, nullptr, nullptr);
  } else if (code && nbit) {
    static const unsigned cap_c = resident_blocks((const void*)k_v2_hist0p<true, false>);
    hipLaunchKernelGGL((k_v2_hist0p<true, false>), dim3(std::min<unsigned>(ntiles, cap_c)),
                       dim3(BLOCK), 0, s, seq, L, k, Nw, g, D, hist, ntiles, scan_status,
                       n_status, meta, code, nbit, nullptr, nullptr, nullptr, nullptr);
  } else {
    static const unsigned cap_n = resident_blocks((const void*)k_v2_hist0p<false, false>);
    hipLaunchKernelGGL((k_v2_hist0p<false, false>), dim3(std::min<unsigned>(ntiles, cap_n)),
                       dim3(BLOCK), 0, s, seq, L, k, Nw, g, D, hist, ntiles, scan_status,
                       n_status, meta, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr);
  }
}
// Beyond 64 tiles of 2048 entries: the 32-per-thread look-back scan at any length.  Measured
// (A/B in one run, `profiles/rd3n_ab_scan_*`): config 3's 15 M-entry histograms 89 -> 60 us per
// scan (three launches of reduce-then-scan before), config 2's 0.5 M 7.7 -> 7.0 us.
void launch_scan_u32(uint32_t* a, uint64_t n, uint64_t* status, uint32_t* total, hipStream_t s) {
  const uint32_t nt = grid_of(n, TILE);
  // entries per thread by length (round 5, `profiles/r5n_scan_width_build_only.txt`): config 2's
  // 0.5 M entries 16 per thread (7.3 -> 6.1 us per scan against 32), config 3's 15 M 64 per
  // thread (59 -> 51 us): a short array wants more workgroups, a long one a shorter look-back
  if (nt > 64) {
    if (n < (1ull << 21)) {
      const uint32_t t16 = grid_of(n, BLOCK * 16);
      hipLaunchKernelGGL(k_scan_lb_u32<16>, dim3(t16), dim3(BLOCK), 0, s, a, n, status, t16, total);
    } else if (n < (1ull << 23)) {
      const uint32_t t32 = grid_of(n, BLOCK * 32);
      hipLaunchKernelGGL(k_scan_lb_u32<32>, dim3(t32), dim3(BLOCK), 0, s, a, n, status, t32, total);
    } else {
      const uint32_t t64 = grid_of(n, BLOCK * 64);
      hipLaunchKernelGGL(k_scan_lb_u32<64>, dim3(t64), dim3(BLOCK), 0, s, a, n, status, t64, total);
    }
  } else {
    hipLaunchKernelGGL(k_scan_lb_u32<WPT>, dim3(nt), dim3(BLOCK), 0, s, a, n, status, nt, total);
  }
}
template <StreamFmt IN>
static void histp_launch(const void* in, const uint32_t* n_ptr, Geom g, Digit D, uint32_t* hist,
                         uint32_t ntiles, uint64_t* scan_status, uint32_t n_status, hipStream_t s,
                         uint32_t* save_col0, int sh) {
  static const unsigned cap = resident_blocks((const void*)k_v2_histp<IN>);
  hipLaunchKernelGGL(k_v2_histp<IN>, dim3(std::min<unsigned>(ntiles, cap)), dim3(BLOCK), 0, s,
                     reinterpret_cast<const uint64_t*>(in), n_ptr, g, D, hist, ntiles,
                     scan_status, n_status, save_col0, sh);
}
void launch_v2_hist(StreamFmt fmt, const void* in, const uint32_t* n_ptr, Geom g, Digit D,
                    uint32_t* hist, uint32_t ntiles, uint64_t* scan_status, uint32_t n_status,
                    hipStream_t s, uint32_t* save_col0, int sh) {
#define KMHG_HISTP(F)                                                                          \
  case StreamFmt::F:                                                                           \
    return histp_launch<StreamFmt::F>(in, n_ptr, g, D, hist, ntiles, scan_status, n_status, s,  \
                                      save_col0, sh)
  switch (fmt == StreamFmt::Keys ? StreamFmt::KeyPos : fmt) {   // the key array alone is read
    KMHG_HISTP(KeyPos);
    KMHG_HISTP(Packed12);
    KMHG_HISTP(Packed8);
    KMHG_HISTP(BidPos);
    KMHG_HISTP(DigitPos);
    KMHG_HISTP(Digits8);
    KMHG_HISTP(Digits16);
    default: std::abort();     // Bids and Pos streams are no pass's histogram input
  }
#undef KMHG_HISTP
}
void launch_v2_hist_keys0(const uint64_t* keys, const uint32_t* n_ptr, Geom g, Digit D,
                          uint32_t* hist, uint32_t ntiles, uint64_t* scan_status,
                          uint32_t n_status, hipStream_t s, uint32_t* hll_rows,
                          uint32_t* hll_regs, bool skip_empty) {
  if (hll_rows)
    hipLaunchKernelGGL(k_v2_hist<true>, dim3(ntiles), dim3(BLOCK), 0, s, keys, n_ptr, g, D, hist,
                       ntiles, scan_status, n_status, hll_rows, hll_regs, nullptr,
                       skip_empty ? 1 : 0);
  else
    hipLaunchKernelGGL(k_v2_hist<false>, dim3(ntiles), dim3(BLOCK), 0, s, keys, n_ptr, g, D, hist,
                       ntiles, scan_status, n_status, nullptr, nullptr, nullptr,
                       skip_empty ? 1 : 0);
}
void launch_v2_bounds_lo(StreamFmt fmt, const void* in, const uint32_t* n_ptr, Geom g,
                         Digit Dlast, uint32_t div, const uint32_t* hist, uint32_t C,
                         const uint32_t* lo_start, uint32_t spread, uint32_t* start,
                         uint32_t nlim, hipStream_t s, int sh) {
  hipLaunchKernelGGL(k_v2_bounds_lo, dim3(div), dim3(BLOCK), 0, s,
                     fmt == StreamFmt::Keys ? StreamFmt::KeyPos : fmt, in, sh, n_ptr, g, Dlast,
                     div, hist, C, lo_start, spread, start, nlim);
}
void launch_seg_bounds(const uint32_t* hist, uint32_t ntiles, uint32_t R, uint32_t nseg,
                       uint32_t tps, const uint32_t* n_valid, uint32_t* segb, hipStream_t s) {
  hipLaunchKernelGGL(k_seg_bounds, dim3(grid_of((uint64_t)R * (nseg + 1), BLOCK)), dim3(BLOCK),
                     0, s, hist, ntiles, R, nseg, tps, n_valid, segb);
}
void launch_v2_hll(const uint32_t* hll_rows, uint32_t n_rows, uint32_t* hll_regs, double* host_est,
                   const uint32_t* n_valid, uint64_t* host_n, hipStream_t s) {
  const uint32_t g = std::max(1u, std::min(HLL_PART_ROWS, (n_rows + 127) / 128));
  hipLaunchKernelGGL(k_v2_hll_part, dim3(g), dim3(HLL_T), 0, s, hll_rows, n_rows, hll_regs);
  hipLaunchKernelGGL(k_v2_hll_final, dim3(1), dim3(HLL_T), 0, s, hll_regs, g, host_est, n_valid,
                     host_n);
}
void launch_part_dense(const uint64_t* ck, const uint32_t* cp, const uint32_t* off,
                       uint32_t ntiles, const uint32_t* n_total, void* dk, uint32_t* dp,
                       StreamFmt out, hipStream_t s) {
  const dim3 gr(std::min<uint32_t>(ntiles, 8192u)), bl(BLOCK);
  uint64_t* dk64 = reinterpret_cast<uint64_t*>(dk);
  if (out == StreamFmt::Packed12)
    hipLaunchKernelGGL(k_part_dense<true>, gr, bl, 0, s, ck, cp, off, ntiles, n_total, dk64, dp);
  else
    hipLaunchKernelGGL(k_part_dense<false>, gr, bl, 0, s, ck, cp, off, ntiles, n_total, dk64, dp);
}

// One (FROM_SEQ, KEYS0, IN, OUT) pass: the lane-order or the ballot-rank instance, each on its
// own persistent grid; scatter_launch_ds: the pass may also write the next pass's digits.
struct ScatterArgs {
  ScatterIn in;
  uint64_t* kout;
  uint32_t* pout;
  uint32_t pad;
  const uint32_t* n_ptr;
  Geom g;
  Digit D;
  const uint32_t* hist;
  uint32_t ntiles;
  hipStream_t s;
  BoundsFuse bf;
  Pack8 pk;
  DigitOut dso;
};
template <bool FS, bool K0, StreamFmt IN, StreamFmt OUT, bool BAL, bool DS>
static void scatter_launch1(const ScatterArgs& a) {
  static const unsigned cap =
      resident_blocks((const void*)k_v2_scatter<FS, K0, IN, OUT, BAL, DS>, SC_NWV * 64);
  hipLaunchKernelGGL((k_v2_scatter<FS, K0, IN, OUT, BAL, DS>), dim3(std::min(a.ntiles, cap)),
                     dim3(SC_NWV * 64), 0, a.s, a.in.seq, a.in.L, a.in.k, a.in.n0,
                     reinterpret_cast<const uint64_t*>(a.in.kin), a.in.pin, a.n_ptr, a.g, a.D,
                     a.hist, a.ntiles, a.kout, a.pout, a.pad, a.in.skip_empty ? 1 : 0, a.bf, a.pk,
                     a.dso);
}
template <bool FS, bool K0, StreamFmt IN, StreamFmt OUT, bool DS = false>
static void scatter_launch(const ScatterArgs& a) {
  if (ballot_ranks()) scatter_launch1<FS, K0, IN, OUT, true, DS>(a);
  else scatter_launch1<FS, K0, IN, OUT, false, DS>(a);
}
template <bool FS, bool K0, StreamFmt IN, StreamFmt OUT>
static void scatter_launch_ds(const ScatterArgs& a) {
  if (a.dso.out || a.dso.out8) scatter_launch<FS, K0, IN, OUT, true>(a);
  else scatter_launch<FS, K0, IN, OUT, false>(a);
}
constexpr int pass_id(int src, StreamFmt i, StreamFmt o) {
  return (src * 16 + (int)i) * 16 + (int)o;
}
void launch_v2_scatter(const ScatterIn& in, StreamFmt fin, StreamFmt fout, void* kout,
                       uint32_t* pout, uint32_t pad, const uint32_t* n_ptr, Geom g, Digit D,
                       const uint32_t* hist, uint32_t ntiles, hipStream_t s, const BoundsFuse* bf,
                       const Pack8* pk, const DigitOut* ds) {
  using F = StreamFmt;
  const ScatterArgs a{in, reinterpret_cast<uint64_t*>(kout), pout, pad, n_ptr, g, D, hist, ntiles,
                      s, bf ? *bf : BoundsFuse{nullptr, nullptr, Digit{}, 0u, 1u, 0u},
                      pk ? *pk : Pack8{0, nullptr, 0u, Digit{}}, ds ? *ds : kNoDigits};
  // every pass there is: its source (SEQ the sequence, FIRST a first pass with implicit
  // positions, 0 a stream), IN -> OUT, and whether it may also write digits (_ds)
  enum { SEQ = 2, FIRST = 1 };
#define KMHG_PASS(SRC, I, O, LAUNCH)                                                           \
  case pass_id(SRC, F::I, F::O):                                                               \
    return LAUNCH<SRC == SEQ, SRC == FIRST, F::I, F::O>(a)
  switch (pass_id(in.seq ? SEQ : in.first ? FIRST : 0, fin, fout)) {
    KMHG_PASS(SEQ, Keys, KeyPos, scatter_launch_ds);
    KMHG_PASS(SEQ, Keys, Packed12, scatter_launch_ds);
    KMHG_PASS(SEQ, Keys, Packed8, scatter_launch_ds);
    KMHG_PASS(FIRST, Keys, Keys, scatter_launch);
    KMHG_PASS(FIRST, Keys, KeyPos, scatter_launch);
    KMHG_PASS(FIRST, Bids, BidPos, scatter_launch_ds);
    KMHG_PASS(FIRST, Bids, DigitPos, scatter_launch);
    KMHG_PASS(FIRST, Bids, Pos, scatter_launch);
    KMHG_PASS(0, Keys, Keys, scatter_launch);
    KMHG_PASS(0, KeyPos, KeyPos, scatter_launch_ds);
    KMHG_PASS(0, KeyPos, Packed12, scatter_launch_ds);
    KMHG_PASS(0, Packed12, Packed12, scatter_launch_ds);
    KMHG_PASS(0, Packed8, Packed12, scatter_launch);
    KMHG_PASS(0, BidPos, BidPos, scatter_launch_ds);
    KMHG_PASS(0, BidPos, Pos, scatter_launch);
    KMHG_PASS(0, DigitPos, Pos, scatter_launch);
    default: std::abort();     // not a pair of formats a pass converts (scatter_pair_ok)
  }
#undef KMHG_PASS
}
// a bucket kernel instance's switches <COUNT_ONLY, CK, BALLOT, AOS, TAGS> as one number
static constexpr int bucket_inst(bool co, bool ck, bool bal, bool aos, bool tags) {
  return co * 16 + ck * 8 + bal * 4 + aos * 2 + tags;
}
void launch_v2_bucket_wg(StreamFmt fmt, const void* keys_, const uint32_t* pos,
                         const uint32_t* start, Geom g, Slot* T, int32_t* positions,
                         BucketStats* bstats, BuildMeta* meta, hipStream_t s,
                         const uint32_t* n_ptr, uint32_t nw, const uint32_t* code, int k,
                         uint8_t* TG, uint32_t* rep, bool place, uint32_t* place_ctr) {
  const uint64_t* keys = reinterpret_cast<const uint64_t*>(keys_);
  const bool count_only = fmt == StreamFmt::Keys, aos = fmt == StreamFmt::Packed12;
  if (fmt != StreamFmt::Pos) code = nullptr;     // only bucket-id builds cut keys from the code
  const bool ballot = ballot_ranks();
  const bool tags = TG != nullptr && !count_only && !code;
  const dim3 gr(g.nb), bl(BLOCK);
  // (count-only: no positions, so nothing is ranked, packed or tagged)
  const int inst = count_only ? bucket_inst(true, false, false, false, false)
                              : bucket_inst(false, code != nullptr, ballot, aos, tags);
#define KMHG_BUCKET(CO, CKK, BAL, AO, TG_)                                                       \
  case bucket_inst(CO, CKK, BAL, AO, TG_):                                                       \
    hipLaunchKernelGGL((k_v2_bucket_wg<CO, CKK, BAL, AO, TG_>), gr, bl, 0, s, keys, pos, start,  \
                       g, T, positions, bstats, meta, CKK ? code : nullptr, CKK ? k : 0, n_ptr,  \
                       nw, TG, rep, place ? 1u : 0u, place_ctr);                                 \
    break
  switch (inst) {
    KMHG_BUCKET(true, false, false, false, false);
    KMHG_BUCKET(false, true, false, false, false);
    KMHG_BUCKET(false, true, true, false, false);
    KMHG_BUCKET(false, false, false, false, false);
    KMHG_BUCKET(false, false, true, false, false);
    KMHG_BUCKET(false, false, false, false, true);
    KMHG_BUCKET(false, false, true, false, true);
    KMHG_BUCKET(false, false, false, true, false);
    KMHG_BUCKET(false, false, true, true, false);
    KMHG_BUCKET(false, false, false, true, true);
    KMHG_BUCKET(false, false, true, true, true);
    default: std::abort();     // code words with a packed stream or tags: no such build
  }
#undef KMHG_BUCKET
}
// The hardware property the radix passes' ranks rest on, checked on the device itself
// (tools/lds_order.hip is the stand-alone probe): the lanes of one returning LDS add that hit
// the same address get old values in increasing lane order.  Every wave draws skewed random
// digits, adds, and compares each lane with every lower lane of the same digit.
__global__ void __launch_bounds__(BLOCK)
k_lane_order_check(unsigned long long* __restrict__ res, uint32_t seed, int iters) {
  __shared__ uint32_t cnt[BLOCK / 64][128];
  __shared__ uint32_t got[BLOCK / 64][64], dig[BLOCK / 64][64];
  const int w = threadIdx.x >> 6, lane = lane_id();
  uint32_t r = (seed ^ (blockIdx.x * BLOCK + threadIdx.x) * 2654435761u) | 1u;
  unsigned long long bad = 0, chk = 0;
  for (int it = 0; it < iters; ++it) {
    for (int d = lane; d < 128; d += 64) cnt[w][d] = 0;
    wave_sync();
    r ^= r << 13; r ^= r >> 17; r ^= r << 5;
    const uint32_t d = (r & 1) ? (r >> 8) % 4 : (r >> 8) % 99;
    const bool act = ((r >> 20) & 7) != 0;
    const uint32_t v = act ? atomicAdd(&cnt[w][d], 1u) : 0u;
    got[w][lane] = act ? v : 0xFFFFFFFFu;
    dig[w][lane] = d;
    wave_sync();
    if (act)
      for (int m = 0; m < lane; ++m)
        if (got[w][m] != 0xFFFFFFFFu && dig[w][m] == d) {
          ++chk;
          bad += got[w][m] > v ? 1u : 0u;
        }
    wave_sync();
  }
  atomicAdd(&res[0], bad);
  atomicAdd(&res[1], chk);
}
void launch_lane_order_check(unsigned long long* res, hipStream_t s, int blocks) {
  hipLaunchKernelGGL(k_lane_order_check, dim3(blocks), dim3(BLOCK), 0, s, res, 12345u, 64);
}

// Test knob (KMHG_TEST_DISORDER=<mode>, tests only), each of which the bucket kernel must report
// (the build then falls back) instead of faulting: 1 swaps the first two positions of bucket 0's
// stream; 2 zeroes its first position (an entry no pass wrote: the pad's value); 3 moves bucket
// 1's start past the end of the stream.
// (pos: the stream's positions, every `stride`-th word)
__global__ void k_v2_test_disorder(uint32_t* __restrict__ pos, uint32_t* __restrict__ start,
                                   const uint32_t* __restrict__ n_ptr, int mode, uint32_t stride) {
  if (threadIdx.x == 0 && blockIdx.x == 0) {
    const uint64_t a = start[0], b = start[1];
    if (mode == 1 && b - a >= 2) {
      const uint32_t t = pos[a * stride];
      pos[a * stride] = pos[(a + 1) * stride];
      pos[(a + 1) * stride] = t;
    } else if (mode == 2 && b > a) {
      pos[a * stride] = 0u;
    } else if (mode == 3) {
      start[1] = *n_ptr + 4096u;
    }
  }
}
void launch_v2_test_disorder(StreamFmt fmt, void* keys, uint32_t* pos, uint32_t* start,
                             const uint32_t* n_ptr, int mode, hipStream_t s) {
  uint32_t* words = fmt_pos_array(fmt) ? pos : reinterpret_cast<uint32_t*>(keys);
  hipLaunchKernelGGL(k_v2_test_disorder, dim3(1), dim3(64), 0, s, words + fmt_pos_word(fmt), start,
                     n_ptr, mode, fmt_pos_stride(fmt));
}
void launch_v2_stats(const BucketStats* bstats, uint32_t nb, const uint32_t* n_valid,
                     BuildMeta* meta, BuildMeta* host_meta, hipStream_t s) {
  // one bucket per thread up to 64 workgroups (config 2: 40), then STATS_PER per trip
  // (measured: 5 workgroups of 8 buckets per thread 6.1 us at config 2, 40 of one 4.8; 256
  // workgroups at config 3 16 us against 9 -- their device atomics and arrival tickets)
  unsigned gr = grid_of(nb, BLOCK);
  if (gr > 64) gr = 64;
  hipLaunchKernelGGL(k_v2_stats, dim3(gr), dim3(BLOCK), 0, s, bstats, nb, n_valid, meta, host_meta);
}

}  // namespace kmhg
