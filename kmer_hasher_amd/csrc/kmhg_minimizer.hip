// kmhg_minimizer.hip -- (w,k)-minimizer sampling on the device (gfx950): the selection mask of a
// sequence, the sampled build's compaction of the selected windows, and the query side's mask of
// the probe's window records.  The rule itself is minimizer_selected of kmhg_minimizer.h.
#include "kmhg_device.h"
#include "kmhg_kernels.h"
#include "kmhg_minimizer.h"
#include "kmhg_querycall.h"

namespace kmhg {

// The selection stage: a tile's TILE windows with MIN_HALO more window starts on both sides (w - 1
// <= 255 of them are used; 256 keeps the stage base a multiple of 16), and the chars those reach.
constexpr int MIN_HALO = MINIMIZER_W_MAX;
constexpr int MSTAGE = TILE + 2 * MIN_HALO + 2 * HALO + 16;
constexpr int MSTAGE_W16 = MSTAGE / 16;
using MStage = StageN<MSTAGE_W16>;
constexpr int MIN_NH = TILE + 2 * (MINIMIZER_W_MAX - 1);       // hashes of one tile and its halo
static_assert(MSTAGE % 16 == 0 && MIN_HALO % 16 == 0 && MSTAGE_W16 <= BLOCK, "one word per thread");
// the last halo window starts at stage offset (HALO + 15) + MIN_HALO + TILE - 1 + (MIN_HALO - 1);
// window_key reads the three 16-char words from the one holding the char before it
static_assert((HALO + 15 + MIN_HALO + TILE - 1 + MIN_HALO - 1) / 16 + 2 < MSTAGE_W16,
              "window_key's reads stay inside the stage");

// V_min_mask: bit (u & 31) of mask[u >> 5] = window u (0-based) of the strand is selected at
// (k, w); bits from Nw on, up to the last word, are 0.  One tile per workgroup: the chars are
// staged as the probe stages them (RC: the reverse strand, from the forward sequence), every
// window of the tile and of a halo of w - 1 windows on both sides is hashed ONCE into LDS with
// its validity, and each window decides from LDS by the shared rule -- a lane walks at most
// 2 (w - 1) neighbours, and stops at the first smaller hash: about two steps on random input.
// The tile's 64 mask words leave LDS as 16-B stores (4-B stores in a last, partial tile or for an
// unaligned mask).  *total += the tile's count (one atomic per tile).
template <bool RC>
__global__ void __launch_bounds__(BLOCK)
k_minimizer_mask(const uint8_t* __restrict__ seq, int64_t L, int k, int w, int aligned,
                 uint32_t* __restrict__ mask, int64_t n_words, int mask_al16,
                 unsigned long long* __restrict__ total) {
  __shared__ MStage st;
  __shared__ uint64_t hh[MIN_NH];
  __shared__ uint8_t okb[(MIN_NH + 15) & ~15];
  __shared__ uint32_t mw[TILE / 32];
  __shared__ uint64_t sh[8];
  const uint32_t tile = blockIdx.x;
  const int64_t Nw = L - k + 1;
  const int64_t t_start = (int64_t)tile * TILE;
  const int64_t base = RC ? rc_stage_base(t_start - MIN_HALO, L) : t_start - HALO - MIN_HALO;
  const int o0 = (int)(t_start - base);                  // HALO + MIN_HALO .. + 15
  if (RC) stage_tile_rc(seq, L, base, st, aligned != 0);
  else stage_tile(seq, L, base, st, aligned != 0);
  __syncthreads();
  const int hal = w - 1;
  const int n_h = TILE + 2 * hal;
  for (int i = threadIdx.x; i < n_h; i += BLOCK) {
    const int64_t u = t_start - hal + i;
    uint64_t key = 0;
    const bool v = u >= 0 && u < Nw && window_key(st, o0 - hal + i, u, L, k, key);
    hh[i] = mix64(key);
    okb[i] = v ? 1 : 0;
  }
  __syncthreads();
  const int64_t h0 = t_start - hal;                      // the window of hh[0]
  const auto at = [&](int64_t v, uint64_t& hv) {
    const int64_t i = v - h0;
    if (i < 0 || i >= n_h || !okb[i]) return false;
    hv = hh[i];
    return true;
  };
  const int wave = threadIdx.x >> 6;
  uint64_t cnt = 0;
#pragma unroll 2
  for (int j = 0; j < WPT; ++j) {
    const int64_t u = t_start + j * BLOCK + (int)threadIdx.x;
    const bool sel = u < Nw && minimizer_selected(at, u, w);
    const uint64_t b = __ballot(sel);
    if (lane_id() == 0) {
      mw[j * (BLOCK / 32) + 2 * wave] = (uint32_t)b;
      mw[j * (BLOCK / 32) + 2 * wave + 1] = (uint32_t)(b >> 32);
    }
    cnt += sel ? 1u : 0u;
  }
  uint64_t tot;
  block_excl_scan(cnt, sh, tot);                         // (its barriers publish mw too)
  const int64_t word0 = (int64_t)tile * (TILE / 32);
  const int64_t left = n_words - word0;                  // >= 1: the grid covers ceil(Nw / TILE)
  if (mask_al16 && left >= TILE / 32) {
    if (threadIdx.x < TILE / 128)
      reinterpret_cast<uint4*>(mask + word0)[threadIdx.x] =
          make_uint4(mw[4 * threadIdx.x], mw[4 * threadIdx.x + 1], mw[4 * threadIdx.x + 2],
                     mw[4 * threadIdx.x + 3]);
  } else if ((int64_t)threadIdx.x < min(left, (int64_t)(TILE / 32))) {
    mask[word0 + threadIdx.x] = mw[threadIdx.x];
  }
  if (threadIdx.x == 0 && tot) atomicAdd(total, (unsigned long long)tot);
}

// V_min_compact (sampled builds, w > 1): the selected windows of the sequence in the layout the
// part builds' dense pack reads (V_hist0 PARTC, kmhg_build_v2.hip): (key, position) of tile t's
// selected windows in window order at [t * PTILE, t * PTILE + tcnt[t]).  Like V_hist0 it also
// zeroes the scan's status words and the build's meta record.  A selected window is valid by
// the rule; the window rule is applied all the same, so no mask can put a window into an index
// that the unsampled build would leave out.  `seq` is 16-B aligned (the build copies otherwise).
__global__ void __launch_bounds__(BLOCK)
k_minimizer_compact(const uint8_t* __restrict__ seq, int64_t L, int k, int64_t Nw,
                    const uint32_t* __restrict__ mask, uint64_t* __restrict__ ckeys,
                    uint32_t* __restrict__ cpos, uint32_t* __restrict__ tcnt,
                    uint64_t* __restrict__ scan_status, uint32_t n_status,
                    BuildMeta* __restrict__ meta) {
  __shared__ PStage st;
  __shared__ uint64_t scs[5];
  __shared__ uint64_t sk[PTILE];
  __shared__ uint32_t sp[PTILE];
  for (uint32_t i = blockIdx.x * BLOCK + threadIdx.x; i < n_status; i += gridDim.x * BLOCK)
    scan_status[i] = 0;
  if (blockIdx.x == 0 && threadIdx.x < sizeof(BuildMeta) / 4)
    reinterpret_cast<uint32_t*>(meta)[threadIdx.x] = 0u;
  const uint32_t tile = blockIdx.x;
  const int64_t tile0 = (int64_t)tile * PTILE;
  stage_tile<true>(seq, L, tile0 - HALO, st, true);
  __syncthreads();
  static_assert(PWPT == 8 && PTILE % 32 == 0, "a thread's 8 windows are one byte of a mask word");
  const int w0 = PWPT * threadIdx.x;
  const int64_t s0 = tile0 + w0;
  const Win8 win(st, HALO + w0, s0, L, k);
  uint32_t own = 0;
  if (s0 < Nw) own = (mask[s0 >> 5] >> (s0 & 31)) & 0xFFu & win.valid_mask(Nw);
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
  const uint64_t base = (uint64_t)tile * PTILE;
  for (uint32_t i = threadIdx.x; i < (uint32_t)tot; i += BLOCK) {
    ckeys[base + i] = sk[i];
    cpos[base + i] = sp[i];
  }
  if (threadIdx.x == 0) tcnt[tile] = (uint32_t)tot;
}

// Q_min_mask (queries on a sampled index): between the probe and the scan of its tile totals,
// the records of the query windows the rule does not select become 0, as if the probe had
// missed, and the tile's total becomes what its windows keep.  Record e is window w0 + e of the
// strand; `mask` covers the whole strand.  Windows as Q_mask takes them; a kept record is not
// rewritten.
__global__ void __launch_bounds__(BLOCK)
k_qrec_minmask(uint32_t* __restrict__ qrec, const uint2* __restrict__ qmulti, int64_t Nw,
               int64_t w0, const uint32_t* __restrict__ mask, uint64_t* __restrict__ tile_rows) {
  __shared__ uint64_t sh[8];
  const uint32_t tile = blockIdx.x;
  const int64_t tile0 = (int64_t)tile * TILE;
  uint64_t rows = 0;
#pragma unroll
  for (int j = 0; j < WPT; ++j) {
    const int64_t e = tile0 + j * BLOCK + threadIdx.x;
    if (e >= Nw) continue;
    uint32_t rec = qrec[e];
    if (rec == 0u) continue;
    const int64_t u = w0 + e;
    if (!((mask[u >> 5] >> (u & 31)) & 1u)) {
      qrec[e] = 0u;
      continue;
    }
    rows += qrec_rows(rec, rec == QREC_MAXOCC_MULTI ? qmulti[e].x : 1u, 0xFFFFFFFFu);
  }
  uint64_t tot;
  block_excl_scan(rows, sh, tot);
  if (threadIdx.x == 0) tile_rows[tile] = tot;
}

// ---------------------------------------------------------------- launchers
void launch_minimizer_mask(const uint8_t* seq, int64_t L, int k, int w, bool rc, bool aligned,
                           uint32_t* mask, unsigned long long* total, hipStream_t s) {
  const int64_t Nw = L - k + 1;
  const unsigned grid = (unsigned)((Nw + TILE - 1) / TILE);
  const int al16 = (reinterpret_cast<uintptr_t>(mask) & 15) == 0;
  if (rc)
    hipLaunchKernelGGL(k_minimizer_mask<true>, dim3(grid), dim3(BLOCK), 0, s, seq, L, k, w,
                       aligned ? 1 : 0, mask, minimizer_mask_words(Nw), al16, total);
  else
    hipLaunchKernelGGL(k_minimizer_mask<false>, dim3(grid), dim3(BLOCK), 0, s, seq, L, k, w,
                       aligned ? 1 : 0, mask, minimizer_mask_words(Nw), al16, total);
}

void launch_minimizer_compact(const uint8_t* seq, int64_t L, int k, int64_t Nw,
                              const uint32_t* mask, uint64_t* ckeys, uint32_t* cpos,
                              uint32_t* tcnt, uint32_t ntiles, uint64_t* scan_status,
                              uint32_t n_status, BuildMeta* meta, hipStream_t s) {
  hipLaunchKernelGGL(k_minimizer_compact, dim3(ntiles), dim3(BLOCK), 0, s, seq, L, k, Nw, mask,
                     ckeys, cpos, tcnt, scan_status, n_status, meta);
}

void launch_qrec_minmask(uint32_t* qrec, const uint2* qmulti, int64_t Nw, int64_t w0,
                         const uint32_t* mask, uint64_t* tile_rows, hipStream_t s) {
  hipLaunchKernelGGL(k_qrec_minmask, dim3((unsigned)((Nw + TILE - 1) / TILE)), dim3(BLOCK), 0, s,
                     qrec, qmulti, Nw, w0, mask, tile_rows);
}

}  // namespace kmhg
