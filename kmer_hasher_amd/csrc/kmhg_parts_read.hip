// kmhg_parts_read.hip -- kmer.pos over the parts of an owner-computes build, no assembly
// (kmhg_parts_read.h).  The reference's kmer_positions (src/kmer_hash.c:1054-1147) walks one
// table; here the table stays split over the ranks as the reader pool splits its k-mers
// (src/kmer_reader.c:28-39), and only an L-bit mask and each part's finished rows move.
#include <hip/hip_runtime.h>

#include <algorithm>

#include "kmhg_device.h"
#include "kmhg_parts_read.h"

namespace kmhg {

static inline unsigned grid_cap(uint64_t n, unsigned per, unsigned cap = 16384) {
  const uint64_t g = (n + per - 1) / per;
  return (unsigned)std::min<uint64_t>(std::max<uint64_t>(g, 1), cap);
}

// P_mask: the first position of every occupied slot, as k_read_first finds it, into the bitmap.
// Distinct keys have distinct first positions, so no bit is set twice; bits of one word come
// from unrelated slots, hence the atomic OR.
__global__ void __launch_bounds__(BLOCK)
k_part_mask(const Slot* __restrict__ T, uint64_t nslots, const int32_t* __restrict__ positions,
            int64_t L, uint32_t* __restrict__ mask) {
  for (uint64_t i = (uint64_t)blockIdx.x * BLOCK + threadIdx.x; i < nslots;
       i += (uint64_t)gridDim.x * BLOCK) {
    const uint4 v = *reinterpret_cast<const uint4*>(&T[i]);
    if (!v.z) continue;
    const uint32_t b = (uint32_t)(v.z == 1 ? (int32_t)v.w : positions[v.w - v.z]) - 1u;
    if ((int64_t)b < L) atomicOr(&mask[b >> 5], 1u << (b & 31u));
  }
}

// P_prefix: exclusive scan of the mask words' popcounts.  A tile is TILE words, WPT consecutive
// words per thread; tiles come from a ticket so every tile a workgroup waits on is running.
__global__ void __launch_bounds__(BLOCK)
k_mask_prefix(const uint32_t* __restrict__ mask, uint64_t W, uint64_t* __restrict__ status,
              uint32_t* __restrict__ ticket, uint32_t* __restrict__ wprefix) {
  __shared__ uint64_t lds[5];
  __shared__ uint64_t base_s;
  __shared__ uint32_t tk;
  const uint32_t tile = take_ticket(ticket, &tk);
  const uint64_t w0 = (uint64_t)tile * TILE + (uint64_t)threadIdx.x * WPT;
  uint32_t pc[WPT];
  uint64_t sum = 0;
#pragma unroll
  for (int j = 0; j < WPT; ++j) {
    pc[j] = w0 + j < W ? (uint32_t)__popc(mask[w0 + j]) : 0u;
    sum += pc[j];
  }
  uint64_t total;
  const uint64_t ex = block_excl_scan(sum, lds, total);
  if (threadIdx.x < 64) {                          // wave 0, all 64 lanes
    const uint64_t x = lookback_excl(status, tile, total);
    if (threadIdx.x == 0) base_s = x;
  }
  __syncthreads();
  uint64_t run = base_s + ex;
#pragma unroll
  for (int j = 0; j < WPT; ++j) {
    if (w0 + j < W) wprefix[w0 + j] = (uint32_t)run;
    run += pc[j];
  }
}

// P_labels: a row's first position -> its rank among all parts' first positions, 1-based.
__global__ void __launch_bounds__(BLOCK)
k_part_labels(const uint2* __restrict__ rinfo, uint32_t U, const int32_t* __restrict__ positions,
              const uint32_t* __restrict__ mask, const uint32_t* __restrict__ wprefix, uint64_t W,
              int32_t* __restrict__ labels) {
  for (uint32_t c = blockIdx.x * BLOCK + threadIdx.x; c < U; c += gridDim.x * BLOCK) {
    const uint2 v = rinfo[c];
    const uint32_t b = (uint32_t)(v.x == 1 ? (int32_t)v.y : positions[v.y - v.x]) - 1u;
    const uint32_t w = b >> 5;
    int32_t lab = 0;                               // a position outside the mask: no such row
    if (w < W) lab = (int32_t)(wprefix[w] + (uint32_t)__popc(mask[w] & (0xFFFFFFFFu >> (31u - (b & 31u)))));
    labels[c] = lab;
  }
}

// M_keys: counts and strings by label.  The strings move char by char: thread e reads char e of
// the part's strings (coalesced) and writes it k + 1 chars into a row that is its own.
__global__ void __launch_bounds__(BLOCK)
k_merge_keys(const int32_t* __restrict__ labels, const int32_t* __restrict__ counts,
             const char* __restrict__ kmers, uint32_t Up, uint32_t k1, uint32_t U,
             int32_t* __restrict__ gcount, char* __restrict__ gkmers) {
  const uint64_t stride = (uint64_t)gridDim.x * BLOCK;
  const uint64_t t = (uint64_t)blockIdx.x * BLOCK + threadIdx.x;
  if (gcount)
    for (uint64_t i = t; i < Up; i += stride) {
      const uint32_t l = (uint32_t)labels[i] - 1u;
      if (l < U) gcount[l] = counts[i];
    }
  if (gkmers) {
    const uint64_t n = (uint64_t)Up * k1;
    for (uint64_t e = t; e < n; e += stride) {
      const uint32_t i = (uint32_t)(e / k1);
      const uint32_t l = (uint32_t)labels[i] - 1u;
      if (l < U) gkmers[(uint64_t)l * k1 + (e - (uint64_t)i * k1)] = kmers[e];
    }
  }
}

__global__ void __launch_bounds__(BLOCK)
k_rows_per_key(const int32_t* __restrict__ counts, uint32_t n, int pairs,
               uint64_t* __restrict__ a) {
  for (uint32_t i = blockIdx.x * BLOCK + threadIdx.x; i < n; i += gridDim.x * BLOCK) {
    const uint64_t c = (uint64_t)(uint32_t)counts[i];
    a[i] = pairs ? c * (c - (c ? 1 : 0)) / 2 : c;
  }
}

__global__ void __launch_bounds__(BLOCK)
k_merge_delta(const int32_t* __restrict__ labels, const uint64_t* __restrict__ loff,
              const uint64_t* __restrict__ goff, uint32_t Up, uint32_t U,
              int64_t* __restrict__ delta) {
  for (uint32_t i = blockIdx.x * BLOCK + threadIdx.x; i < Up; i += gridDim.x * BLOCK) {
    const uint32_t l = (uint32_t)labels[i] - 1u;
    if (l < U) delta[l] = (int64_t)goff[l] - (int64_t)loff[i];
  }
}

// M_rows: a part's rows to their global place, one int32 per thread: the reads are coalesced and
// so are the writes inside a key's run (the part's rows ascend by label, so runs follow each
// other in the output too, with the other parts' runs between them).
template <int W>
__global__ void __launch_bounds__(BLOCK)
k_merge_rows(const int32_t* __restrict__ rows, uint64_t n_rows, const int64_t* __restrict__ delta,
             uint32_t U, uint64_t n_out, int32_t* __restrict__ out) {
  const uint64_t n = n_rows * W;
  for (uint64_t e = (uint64_t)blockIdx.x * BLOCK + threadIdx.x; e < n;
       e += (uint64_t)gridDim.x * BLOCK) {
    const uint64_t j = e / W;
    const uint32_t l = (uint32_t)rows[j * W] - 1u;
    if (l >= U) continue;
    const uint64_t d = (uint64_t)((int64_t)j + delta[l]);
    if (d < n_out) out[d * W + (e - j * W)] = rows[e];
  }
}

// ================================================================== launchers
void launch_part_mask(const Slot* T, uint64_t nslots, const int32_t* positions, int64_t L,
                      uint32_t* mask, hipStream_t s) {
  hipLaunchKernelGGL(k_part_mask, dim3(grid_cap(nslots, BLOCK)), dim3(BLOCK), 0, s, T, nslots,
                     positions, L, mask);
}
void launch_mask_prefix(const uint32_t* mask, uint64_t W, uint64_t* status, uint32_t* ticket,
                        uint32_t* wprefix, hipStream_t s) {
  if (!W) return;
  const unsigned nt = (unsigned)((W + TILE - 1) / TILE);
  hipLaunchKernelGGL(k_mask_prefix, dim3(nt), dim3(BLOCK), 0, s, mask, W, status, ticket, wprefix);
}
void launch_part_labels(const uint2* rinfo, uint32_t U, const int32_t* positions,
                        const uint32_t* mask, const uint32_t* wprefix, uint64_t W,
                        int32_t* labels, hipStream_t s) {
  if (!U) return;
  hipLaunchKernelGGL(k_part_labels, dim3(grid_cap(U, BLOCK)), dim3(BLOCK), 0, s, rinfo, U,
                     positions, mask, wprefix, W, labels);
}
void launch_merge_keys(const int32_t* labels, const int32_t* counts, const char* kmers,
                       uint32_t Up, int k, uint32_t U, int32_t* gcount, char* gkmers,
                       hipStream_t s) {
  if (!Up || (!gcount && !gkmers)) return;
  const uint64_t n = gkmers ? (uint64_t)Up * (k + 1) : Up;
  hipLaunchKernelGGL(k_merge_keys, dim3(grid_cap(n, BLOCK)), dim3(BLOCK), 0, s, labels, counts,
                     kmers, Up, (uint32_t)(k + 1), U, gcount, gkmers);
}
void launch_rows_per_key(const int32_t* counts, uint32_t n, bool pairs, uint64_t* a,
                         hipStream_t s) {
  if (!n) return;
  hipLaunchKernelGGL(k_rows_per_key, dim3(grid_cap(n, BLOCK)), dim3(BLOCK), 0, s, counts, n,
                     pairs ? 1 : 0, a);
}
void launch_merge_delta(const int32_t* labels, const uint64_t* loff, const uint64_t* goff,
                        uint32_t Up, uint32_t U, int64_t* delta, hipStream_t s) {
  if (!Up) return;
  hipLaunchKernelGGL(k_merge_delta, dim3(grid_cap(Up, BLOCK)), dim3(BLOCK), 0, s, labels, loff,
                     goff, Up, U, delta);
}
void launch_merge_rows(const int32_t* rows, uint64_t n_rows, int W, const int64_t* delta,
                       uint32_t U, uint64_t n_out, int32_t* out, hipStream_t s) {
  if (!n_rows) return;
  const unsigned g = grid_cap(n_rows * (uint64_t)W, BLOCK * 4, 65536);
  if (W == 2)
    hipLaunchKernelGGL(k_merge_rows<2>, dim3(g), dim3(BLOCK), 0, s, rows, n_rows, delta, U, n_out,
                       out);
  else
    hipLaunchKernelGGL(k_merge_rows<3>, dim3(g), dim3(BLOCK), 0, s, rows, n_rows, delta, U, n_out,
                       out);
}

}  // namespace kmhg
