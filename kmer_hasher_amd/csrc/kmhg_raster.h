// kmhg_raster.h -- the arithmetic of seq.kmer.raster that needs no device (no HIP: any C++
// compiler; the kernels of kmhg_raster.hip include the same functions).
//
// seq.kmer.raster bins (i, j) rows into an n_i x n_j matrix of u32 counts (include/kmhgpu.h has
// the definition): a frame is six integers {i_lo, j_lo, bin_i, bin_j, n_i, n_j}, row (i, j) falls
// into cell ((i - i_lo) / bin_i, (j - j_lo) / bin_j) where both are inside [0, n_i) x [0, n_j),
// and cell (bi, bj) lives at index bi + n_i * bj.  Here: the frame's validation with the entries'
// refusal code and text (raster_check_frame), the overflow rule (raster_may_overflow), the frame
// as the kernels take it (RasterDev: u32 fields and the two divisor constants), the cell of a
// coordinate pair (raster_cell) and the i-cells a tile of consecutive windows can touch
// (raster_tile_span).
//
// The per-row divisions are by run-time divisors, so they are multiply-shifts, the digit
// arithmetic of the radix passes (kmhg_build_v2.hip div_magic): floor(x / d) = mulhi64(x, m) with
// m = ceil(2^64 / d), exact whenever x * d < 2^64 -- here x, d < 2^31 -- and m = 0 standing for
// d = 1.  (The 32-bit form of kmhg_plan.h holds only for dividends below 2^16.)
// tools/asan/raster_check runs all of it under ASan + UBSan (tests/test_raster_host.py).
#pragma once
#include <stdint.h>

#include "../../include/kmhgpu.h"
#include "kmhg_common.h"

namespace kmhg {

constexpr int64_t RASTER_MAX_CELLS = 1ll << 26;
constexpr uint32_t RASTER_OUT = 0xFFFFFFFFu;     // raster_cell of a row outside the frame
// windows with at most this many hits are binned by their own lane (EMIT_DIRECT of Q_emit)
constexpr uint32_t RASTER_DIRECT = 4;

struct RasterFrame {
  int64_t i_lo, j_lo, bin_i, bin_j, n_i, n_j;
};
inline RasterFrame raster_frame(const int64_t f[6]) {
  return RasterFrame{f[0], f[1], f[2], f[3], f[4], f[5]};
}

struct RasterRefusal {
  int code;             // KMHG_OK: the frame is legal
  const char* text;
};

// The entries' frame refusals, in their order (after "null argument").
inline RasterRefusal raster_check_frame(const RasterFrame& f) {
  constexpr int64_t I32 = 0x7FFFFFFFll;
  if (f.bin_i < 1 || f.bin_j < 1)
    return {KMHG_EINVAL, "bin widths must be positive integers"};
  if (f.n_i < 1 || f.n_j < 1)
    return {KMHG_EINVAL, "bin counts must be positive integers"};
  // (n_i, n_j >= 1: either above 2^26 is too many on its own, and then the product fits)
  if (f.n_i > RASTER_MAX_CELLS || f.n_j > RASTER_MAX_CELLS || f.n_i * f.n_j > RASTER_MAX_CELLS)
    return {KMHG_EINVAL, "a raster has at most 2^26 cells"};
  // (bin <= 2^31 - 1 and n <= 2^26 from here: n * bin < 2^57)
  if (f.i_lo < 1 || f.j_lo < 1 || f.i_lo > I32 || f.j_lo > I32 || f.bin_i > I32 ||
      f.bin_j > I32 || f.i_lo + f.n_i * f.bin_i - 1 > I32 || f.j_lo + f.n_j * f.bin_j - 1 > I32)
    return {KMHG_EINVAL, "the frame must lie within 1..2^31-1 on both axes"};
  return {KMHG_OK, nullptr};
}

// Rows are distinct, so a cell holds at most min(H, bin_i * bin_j) of H rows: a u32 count can
// overflow only where both reach 2^32 (KMHG_EOVERFLOW "a raster cell could exceed 2^32-1 rows").
inline bool raster_may_overflow(const RasterFrame& f, uint64_t H) {
  return (uint64_t)f.bin_i * (uint64_t)f.bin_j >= (1ull << 32) && H >= (1ull << 32);
}

// ceil(2^64 / d) for d >= 2, 0 for d = 1 (magic64 of the radix digits).
inline uint64_t raster_magic(uint32_t d) { return d <= 1 ? 0 : (uint64_t)(~0ull / d) + 1; }

// floor(x / d) by m = raster_magic(d), for x, d < 2^31.
__host__ __device__ inline uint32_t raster_div(uint32_t x, uint64_t m) {
  if (m == 0) return x;
#if defined(__HIP_DEVICE_COMPILE__)
  return (uint32_t)__umul64hi((uint64_t)x, m);
#else
  return (uint32_t)(((unsigned __int128)x * m) >> 64);
#endif
}

// A checked frame as the kernels take it.
struct RasterDev {
  int32_t i_lo, j_lo;
  uint32_t bin_i, bin_j, n_i, n_j;
  uint64_t mi, mj;      // raster_magic of the bin widths
};
inline RasterDev raster_dev(const RasterFrame& f) {
  return RasterDev{(int32_t)f.i_lo, (int32_t)f.j_lo, (uint32_t)f.bin_i, (uint32_t)f.bin_j,
                   (uint32_t)f.n_i,  (uint32_t)f.n_j, raster_magic((uint32_t)f.bin_i),
                   raster_magic((uint32_t)f.bin_j)};
}

// The cell of coordinate x on an axis starting at lo with `n` bins of magic `m`, or RASTER_OUT.
// Any int32 is a legal x: below lo (zero and negatives too) it is outside.
__host__ __device__ inline uint32_t raster_axis(int32_t x, int32_t lo, uint64_t m, uint32_t n) {
  if (x < lo) return RASTER_OUT;
  const uint32_t b = raster_div((uint32_t)x - (uint32_t)lo, m);   // x >= lo >= 1: below 2^31
  return b < n ? b : RASTER_OUT;
}
// The index of row (i, j)'s cell in the matrix, or RASTER_OUT.
__host__ __device__ inline uint32_t raster_cell(const RasterDev& f, int32_t i, int32_t j) {
  const uint32_t bi = raster_axis(i, f.i_lo, f.mi, f.n_i);
  const uint32_t bj = raster_axis(j, f.j_lo, f.mj, f.n_j);
  return bi == RASTER_OUT || bj == RASTER_OUT ? RASTER_OUT : bi + f.n_i * bj;
}

// The i-cells that `tile` consecutive i values can touch: at most tile / bin_i + 2 (a run of
// `tile` values covers floor((tile - 1) / bin_i) + 1 cells when aligned and one more when not).
__host__ __device__ inline uint32_t raster_tile_span(uint32_t tile, uint32_t bin_i) {
  return tile / bin_i + 2;
}

}  // namespace kmhg
