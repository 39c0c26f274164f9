// kmhg_segrec.hip -- the front half of seq.kmer.segs / seq.kmer.blocks without rows: the pairing
// keys of a probed query's segment starts and ends straight from its per-window records (qrec /
// qmulti / positions, launch_query_probe).  Definition and the search arithmetic: kmhg_segrec.h.
//
// Both kernels run one workgroup per tile of TILE query windows and walk it as R_records does
// (kmhg_raster.hip): a window with at most SEGREC_DIRECT hits is classified by its own lane, hit q
// of every such window of the wave in one step; a window with more is listed in LDS and then dealt
// to the whole workgroup, BLOCK consecutive hits per step, SR_STEPS steps per round so that a
// round's loads are in flight together.  Windows s - 1 and s + 1 are read from the global records:
// tile edges need no halo.  No lane walks a diagonal, none a list beyond SEGREC_DIRECT.
//
//   SR_count   per tile the starts and the ends as two full u64 (a tile can hold more than 2^32
//              hits, and the totals must be exact before anything is refused), per window its
//              starts as a u32 (a window has fewer than 2^31 hits)
//   scans      launch_scan_u64 over either tile array
//   SR_emit    the same walk again (nothing of size H is kept): every start writes seg_key(i, j)
//              and its rank among all starts in (s, q) order -- the tile's offset, the window's
//              prefix inside the tile (a scan of SR_count's per-window counts), its rank inside
//              the window (a dealt window: the ballot prefix of its step over a running base, the
//              steps' wave counts exchanged through LDS, one barrier per round) -- and every end
//              its key at a slot drawn from the tile's LDS counter: the ends' order is the sort's
// The ranks are those S_emit gives the same starts (kmhg_segs.hip), so everything behind the sort
// is byte for byte what the rows route produces.  Ranks and slots are below S <= 2^31 - 1 (the
// host refused anything else before SR_emit is launched) and are checked against S before a store.
#include <hip/hip_runtime.h>
#include "kmhg_common.h"
#include "kmhg_device.h"
#include "kmhg_kernels.h"
#include "kmhg_segrec.h"

namespace kmhg {

namespace {

constexpr int NW = BLOCK / 64;
constexpr int SR_STEPS = 4;            // steps of BLOCK hits per round of a dealt window
static_assert(TILE <= 65536, "heavy[] holds tile-local window indices");

// A distinct slot from *ctr (LDS) for every lane with f set: one atomic per wave.  Called by all
// 64 lanes of a wave together.
__device__ __forceinline__ uint32_t wave_slot(bool f, uint32_t* ctr) {
  const uint64_t m = __ballot(f);
  if (!m) return 0u;                                // uniform
  const int lead = __ffsll((unsigned long long)m) - 1;
  uint32_t b = 0;
  if (lane_id() == lead) b = atomicAdd(ctr, (uint32_t)__popcll(m));
  b = __shfl(b, lead);
  return b + (uint32_t)__popcll(m & lanemask_lt());
}

__global__ void __launch_bounds__(BLOCK)
k_segrec_count(const uint32_t* __restrict__ qrec, const uint2* __restrict__ qmulti, int64_t Nw,
               const int32_t* __restrict__ positions, uint64_t* __restrict__ tile_starts,
               uint64_t* __restrict__ tile_ends, uint32_t* __restrict__ win_starts) {
  __shared__ uint16_t heavy[TILE];
  __shared__ uint32_t hcnt[TILE];                   // starts of listed window h
  __shared__ uint32_t n_heavy;
  __shared__ uint64_t wtot[2 * NW];
  const int64_t tile0 = (int64_t)blockIdx.x * TILE;
  const int wave = threadIdx.x >> 6, lane = lane_id();
  if (threadIdx.x == 0) n_heavy = 0;
  uint32_t rec[WPT];
#pragma unroll
  for (int j = 0; j < WPT; ++j) {
    const int64_t s = tile0 + j * BLOCK + threadIdx.x;
    rec[j] = s < Nw ? qrec[s] : 0u;
  }
  __syncthreads();
  uint64_t ls = 0, le = 0;                          // this lane's light windows
#pragma unroll
  for (int j = 0; j < WPT; ++j) {
    const int w = j * BLOCK + threadIdx.x;
    const int64_t s = tile0 + w;
    uint32_t ns = 0, ne = 0;
    bool listed = false;
    if (rec[j] == 0u) {
    } else if (rec[j] != SEGREC_MULTI) {
      const uint32_t c = segrec_classify(qrec, qmulti, positions, Nw, s, 0u, (int32_t)rec[j]);
      ns = c & SEG_START;
      ne = (c >> 1) & 1u;
    } else {
      const uint2 v = qmulti[s];
      if (v.x > SEGREC_DIRECT) {
        heavy[atomicAdd(&n_heavy, 1u)] = (uint16_t)w;
        listed = true;
      } else {
        for (uint32_t q = 0; q < v.x; ++q) {
          const uint32_t c = segrec_classify(qrec, qmulti, positions, Nw, s, q, positions[v.y + q]);
          ns += c & SEG_START;
          ne += (c >> 1) & 1u;
        }
      }
    }
    if (s < Nw && !listed) win_starts[s] = ns;
    ls += ns;
    le += ne;
  }
  __syncthreads();
  const uint32_t nh = n_heavy;
  for (uint32_t h = threadIdx.x; h < nh; h += BLOCK) hcnt[h] = 0u;
  __syncthreads();
  uint64_t hs = 0, he = 0;                          // this wave's share of the listed windows
  for (uint32_t h = 0; h < nh; ++h) {               // uniform loops
    const uint32_t w = heavy[h];
    const int64_t s = tile0 + w;
    const uint2 v = qmulti[s];
    uint32_t cs = 0, ce = 0;
    for (uint32_t base = 0; base < v.x; base += SR_STEPS * BLOCK) {
      uint32_t c[SR_STEPS];
#pragma unroll
      for (int u = 0; u < SR_STEPS; ++u) {
        const uint32_t q = base + u * BLOCK + threadIdx.x;
        c[u] = q < v.x ? segrec_classify(qrec, qmulti, positions, Nw, s, q, positions[v.y + q]) : 0u;
      }
#pragma unroll
      for (int u = 0; u < SR_STEPS; ++u) {
        cs += (uint32_t)__popcll(__ballot(c[u] & SEG_START));
        ce += (uint32_t)__popcll(__ballot(c[u] & SEG_END));
      }
    }
    if (lane == 0) atomicAdd(&hcnt[h], cs);
    hs += cs;
    he += ce;
  }
  __syncthreads();
  for (uint32_t h = threadIdx.x; h < nh; h += BLOCK) win_starts[tile0 + heavy[h]] = hcnt[h];
  ls = wave_sum(ls) + hs;
  le = wave_sum(le) + he;
  if (lane == 0) {
    wtot[wave] = ls;
    wtot[NW + wave] = le;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    uint64_t a = 0, b = 0;
#pragma unroll
    for (int x = 0; x < NW; ++x) {
      a += wtot[x];
      b += wtot[NW + x];
    }
    tile_starts[blockIdx.x] = a;
    tile_ends[blockIdx.x] = b;
  }
}

__global__ void __launch_bounds__(BLOCK)
k_segrec_emit(const uint32_t* __restrict__ qrec, const uint2* __restrict__ qmulti, int64_t Nw,
              int64_t w0, int kq, const int32_t* __restrict__ positions,
              const uint32_t* __restrict__ win_starts, const uint64_t* __restrict__ tile_soff,
              const uint64_t* __restrict__ tile_eoff, uint32_t S, uint64_t* __restrict__ skey,
              uint32_t* __restrict__ srank, uint64_t* __restrict__ ekey) {
  __shared__ uint16_t heavy[TILE];
  __shared__ uint32_t hbase[TILE];                  // rank of listed window h's first start
  __shared__ uint32_t n_heavy, end_ctr;
  __shared__ uint32_t cw[WPT * NW];
  __shared__ uint32_t gcnt[2][SR_STEPS * NW];
  const int64_t tile0 = (int64_t)blockIdx.x * TILE;
  const int32_t i0 = (int32_t)(w0 + tile0 + kq);    // window w of the tile has i = i0 + w
  const int wave = threadIdx.x >> 6, lane = lane_id();
  if (threadIdx.x == 0) {
    n_heavy = 0;
    end_ctr = 0;
  }
  uint32_t rec[WPT], pre[WPT];
  // the windows' start counts scanned in window order (element e = j * BLOCK + t)
#pragma unroll
  for (int j = 0; j < WPT; ++j) {
    const int64_t s = tile0 + j * BLOCK + threadIdx.x;
    rec[j] = s < Nw ? qrec[s] : 0u;
    const uint32_t ws = s < Nw ? win_starts[s] : 0u;
    const uint32_t inc = wave_incl_scan_u32(ws);
    pre[j] = inc - ws;
    if (lane == 63) cw[j * NW + wave] = inc;
  }
  __syncthreads();
  if (wave == 0) {                                  // lanes 0 .. WPT*NW-1 own one (j, wave) count
    const uint32_t c = lane < WPT * NW ? cw[lane] : 0u;
    const uint32_t inc = wave_incl_scan_u32(c);
    if (lane < WPT * NW) cw[lane] = inc - c;
  }
  __syncthreads();
  const uint32_t sbase = (uint32_t)tile_soff[blockIdx.x], ebase = (uint32_t)tile_eoff[blockIdx.x];
#pragma unroll
  for (int j = 0; j < WPT; ++j) pre[j] += cw[j * NW + wave] + sbase;
#pragma unroll
  for (int j = 0; j < WPT; ++j) {
    const int w = j * BLOCK + threadIdx.x;
    const int64_t s = tile0 + w;
    uint32_t n = 0, st0 = 0;
    if (rec[j] == SEGREC_MULTI) {
      const uint2 v = qmulti[s];
      if (v.x > SEGREC_DIRECT) {
        const uint32_t h = atomicAdd(&n_heavy, 1u);
        heavy[h] = (uint16_t)w;
        hbase[h] = pre[j];
      } else {
        n = v.x;
        st0 = v.y;
      }
    } else if (rec[j] != 0u) {
      n = 1;
    }
    uint32_t r = pre[j];
    for (uint32_t q = 0; q < SEGREC_DIRECT; ++q) {  // hit q of the wave's light windows
      if (!__ballot(q < n)) break;                  // uniform
      uint32_t c = 0;
      int32_t jj = 0;
      if (q < n) {
        jj = rec[j] != SEGREC_MULTI ? (int32_t)rec[j] : positions[st0 + q];
        c = segrec_classify(qrec, qmulti, positions, Nw, s, q, jj);
      }
      const uint64_t key = seg_key(i0 + w, jj);
      if (c & SEG_START) {
        if (r < S) {
          skey[r] = key;
          srank[r] = r;
        }
        ++r;
      }
      const uint32_t e = ebase + wave_slot((c & SEG_END) != 0u, &end_ctr);
      if ((c & SEG_END) && e < S) ekey[e] = key;
    }
  }
  __syncthreads();
  const uint32_t nh = n_heavy;
  int par = 0;
  for (uint32_t h = 0; h < nh; ++h) {               // uniform loops: every lane reaches the barrier
    const uint32_t w = heavy[h];
    const int64_t s = tile0 + w;
    const uint2 v = qmulti[s];
    uint32_t run = hbase[h];                        // rank of the window's next start
    for (uint32_t base = 0; base < v.x; base += SR_STEPS * BLOCK) {
      uint32_t c[SR_STEPS];
      int32_t jj[SR_STEPS];
      uint64_t ms[SR_STEPS];
#pragma unroll
      for (int u = 0; u < SR_STEPS; ++u) {
        const uint32_t q = base + u * BLOCK + threadIdx.x;
        jj[u] = q < v.x ? positions[v.y + q] : 0;
        c[u] = q < v.x ? segrec_classify(qrec, qmulti, positions, Nw, s, q, jj[u]) : 0u;
      }
#pragma unroll
      for (int u = 0; u < SR_STEPS; ++u) {
        ms[u] = __ballot(c[u] & SEG_START);
        if (lane == 0) gcnt[par][u * NW + wave] = (uint32_t)__popcll(ms[u]);
      }
      __syncthreads();
      // hits ascend by (step, wave, lane): the starts before this wave's, step by step.  The
      // other buffer is written next round, after a barrier every reader of this one has passed.
      uint32_t off[SR_STEPS];
#pragma unroll
      for (int u = 0; u < SR_STEPS; ++u) {
        off[u] = 0;
#pragma unroll
        for (int x = 0; x < NW; ++x) {
          if (x == wave) off[u] = run;
          run += gcnt[par][u * NW + x];
        }
      }
      par ^= 1;
#pragma unroll
      for (int u = 0; u < SR_STEPS; ++u) {
        const uint64_t key = seg_key(i0 + (int32_t)w, jj[u]);
        if (c[u] & SEG_START) {
          const uint32_t r = off[u] + (uint32_t)__popcll(ms[u] & lanemask_lt());
          if (r < S) {
            skey[r] = key;
            srank[r] = r;
          }
        }
        const uint32_t e = ebase + wave_slot((c[u] & SEG_END) != 0u, &end_ctr);
        if ((c[u] & SEG_END) && e < S) ekey[e] = key;
      }
    }
  }
}

}  // namespace

void launch_segrec_count(const uint32_t* qrec, const uint2* qmulti, int64_t Nw,
                         const int32_t* positions, uint64_t* tile_starts, uint64_t* tile_ends,
                         uint32_t* win_starts, hipStream_t s) {
  hipLaunchKernelGGL(k_segrec_count, dim3(tiles_for((uint64_t)Nw)), dim3(BLOCK), 0, s, qrec, qmulti,
                     Nw, positions, tile_starts, tile_ends, win_starts);
}
void launch_segrec_emit(const uint32_t* qrec, const uint2* qmulti, int64_t Nw, int64_t w0, int kq,
                        const int32_t* positions, const uint32_t* win_starts,
                        const uint64_t* tile_soff, const uint64_t* tile_eoff, uint64_t S,
                        uint64_t* skey, uint32_t* srank, uint64_t* ekey, hipStream_t s) {
  hipLaunchKernelGGL(k_segrec_emit, dim3(tiles_for((uint64_t)Nw)), dim3(BLOCK), 0, s, qrec, qmulti,
                     Nw, w0, kq, positions, win_starts, tile_soff, tile_eoff, (uint32_t)S, skey,
                     srank, ekey);
}

}  // namespace kmhg
