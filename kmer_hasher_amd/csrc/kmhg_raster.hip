// kmhg_raster.hip -- seq.kmer.raster on the device: (i, j) rows binned into an n_i x n_j matrix
// of u32 counts.  Definition, frame checks and the cell arithmetic: kmhg_raster.h.
//
//   R_rows      plain rows in tiles of TILE (element e = j * BLOCK + t, as the run kernels): each
//               lane bins its row, then the wave adds
//   R_records   the row-free route: one workgroup per tile of TILE query windows over the probe's
//               records (qrec / qmulti / positions, Q_emit's traversal), no row ever written.  A
//               window's i-cell is taken once; a window outside the frame's i range reads no
//               position.  Windows with at most RASTER_DIRECT hits are binned by their own lane,
//               hit q of every such window of the wave in one step; windows with more are listed
//               in LDS and then dealt to the whole workgroup one at a time, BLOCK consecutive
//               positions per step
//   wave_add    every add of both kernels.  Consecutive lanes hold consecutive rows, consecutive
//               windows (whose single hits lie along a diagonal) or consecutive positions of one
//               window (ascending j), so equal cells sit next to each other: a lane is a head where
//               its cell differs from the previous active lane's, and only heads add, the length of
//               their run of active lanes -- one atomic per run, not one per row.  Right for any
//               order of cells (unsorted rows only make shorter runs).
// Integer adds commute: the matrix is the same bytes on every run.  No saturation logic
// (raster_may_overflow is the host's refusal).
#include <hip/hip_runtime.h>
#include "kmhg_common.h"
#include "kmhg_device.h"
#include "kmhg_kernels.h"
#include "kmhg_raster.h"

namespace kmhg {

namespace {

constexpr uint32_t RQ_MULTI = 0x80000000u;       // QREC_MULTI of kmhg_kernels.hip (put_qrec)

// Called by all 64 lanes of a wave together; cell = RASTER_OUT: nothing to add for this lane.
__device__ __forceinline__ void wave_add(uint32_t* __restrict__ out, uint32_t cell) {
  const uint64_t act = __ballot(cell != RASTER_OUT);
  if (!act) return;                               // uniform
  const int lane = lane_id();
  const uint64_t lt = (1ull << lane) - 1;         // the lanes below this one
  const uint64_t below = act & lt;
  const int prev = below ? 63 - __clzll((long long)below) : lane;
  const uint32_t pc = __shfl(cell, prev);
  const bool head = cell != RASTER_OUT && (!below || pc != cell);
  const uint64_t heads = __ballot(head);
  if (head) {
    const uint64_t above = lane == 63 ? 0ull : heads >> (lane + 1);
    // the run: active lanes from this one up to the next head (lane + 1 + its rank in `above`)
    const uint64_t upto = above ? (1ull << (lane + __ffsll((unsigned long long)above))) - 1 : ~0ull;
    atomicAdd(out + cell, (uint32_t)__popcll(act & upto & ~lt));
  }
}

__global__ void __launch_bounds__(BLOCK)
k_raster_rows(const int2* __restrict__ rows, uint64_t n, RasterDev f, uint32_t* __restrict__ out) {
  const uint64_t t0 = (uint64_t)blockIdx.x * TILE;
  int2 r[WPT];
#pragma unroll
  for (int j = 0; j < WPT; ++j) {
    const uint64_t e = t0 + (uint64_t)j * BLOCK + threadIdx.x;
    r[j] = e < n ? rows[e] : make_int2(0, 0);     // (0, 0) lies outside every frame
  }
#pragma unroll
  for (int j = 0; j < WPT; ++j) wave_add(out, raster_cell(f, r[j].x, r[j].y));
}

__global__ void __launch_bounds__(BLOCK)
k_raster_records(const uint32_t* __restrict__ qrec, const uint2* __restrict__ qmulti, int64_t Nw,
                 int64_t w0, int kq, const int32_t* __restrict__ positions, RasterDev f,
                 uint32_t* __restrict__ out) {
  static_assert(TILE <= 65536, "heavy[] holds tile-local window indices");
  __shared__ uint16_t heavy[TILE];
  __shared__ uint32_t n_heavy;
  const int64_t tile0 = (int64_t)blockIdx.x * TILE;
  const int32_t i0 = (int32_t)(w0 + tile0 + kq);  // window w of the tile has i = i0 + w
  if (threadIdx.x == 0) n_heavy = 0;
  uint32_t rec[WPT];
#pragma unroll
  for (int j = 0; j < WPT; ++j) {
    const int64_t s = tile0 + j * BLOCK + threadIdx.x;
    rec[j] = s < Nw ? qrec[s] : 0u;
  }
  __syncthreads();
#pragma unroll 2
  for (int j = 0; j < WPT; ++j) {
    const int w = j * BLOCK + threadIdx.x;
    const uint32_t bi = rec[j] ? raster_axis(i0 + w, f.i_lo, f.mi, f.n_i) : RASTER_OUT;
    uint32_t cell = RASTER_OUT, n = 0, st0 = 0;
    if (bi != RASTER_OUT) {
      if (rec[j] != RQ_MULTI) {
        const uint32_t bj = raster_axis((int32_t)rec[j], f.j_lo, f.mj, f.n_j);
        if (bj != RASTER_OUT) cell = bi + f.n_i * bj;
      } else {
        const uint2 v = qmulti[tile0 + w];
        if (v.x > RASTER_DIRECT) heavy[atomicAdd(&n_heavy, 1u)] = (uint16_t)w;
        else { n = v.x; st0 = v.y; }
      }
    }
    wave_add(out, cell);                          // the single hits
    if (__ballot(n != 0)) {                       // uniform: hit q of the wave's light windows
      for (uint32_t q = 0; q < RASTER_DIRECT; ++q) {
        uint32_t c = RASTER_OUT;
        if (q < n) {
          const uint32_t bj = raster_axis(positions[st0 + q], f.j_lo, f.mj, f.n_j);
          if (bj != RASTER_OUT) c = bi + f.n_i * bj;
        }
        wave_add(out, c);
      }
    }
  }
  __syncthreads();
  const uint32_t nh = n_heavy;
  for (uint32_t h = 0; h < nh; ++h) {             // uniform loops: every lane reaches wave_add
    const uint32_t w = heavy[h];
    const uint2 v = qmulti[tile0 + w];
    const uint32_t bi = raster_axis(i0 + (int32_t)w, f.i_lo, f.mi, f.n_i);   // inside: it was listed
    for (uint32_t base = 0; base < v.x; base += BLOCK) {
      const uint32_t q = base + threadIdx.x;
      uint32_t c = RASTER_OUT;
      if (q < v.x) {
        const uint32_t bj = raster_axis(positions[v.y + q], f.j_lo, f.mj, f.n_j);
        if (bj != RASTER_OUT) c = bi + f.n_i * bj;
      }
      wave_add(out, c);
    }
  }
}

}  // namespace

void launch_raster_rows(const int2* rows, uint64_t n, const RasterDev& f, uint32_t* out,
                        hipStream_t s) {
  hipLaunchKernelGGL(k_raster_rows, dim3(tiles_for(n)), dim3(BLOCK), 0, s, rows, n, f, out);
}
void launch_raster_records(const uint32_t* qrec, const uint2* qmulti, int64_t Nw, int64_t w0,
                           int kq, const int32_t* positions, const RasterDev& f, uint32_t* out,
                           hipStream_t s) {
  hipLaunchKernelGGL(k_raster_records, dim3(tiles_for((uint64_t)Nw)), dim3(BLOCK), 0, s, qrec,
                     qmulti, Nw, w0, kq, positions, f, out);
}

}  // namespace kmhg
