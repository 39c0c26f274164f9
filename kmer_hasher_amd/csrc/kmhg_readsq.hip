// kmhg_readsq.hip -- reads.kmer.pos / reads.kmer.vote on the device: a batch of packed reads
// queried against a position index on both strands, and one vote per read over its rows.
// Definitions, the virtual window space and every rule: kmhg_readsq.h.
//
//   RQ_check    one lane per offset: rq_off_ok_at; a broken entry raises the host's flag (the
//               same value from every lane that sees one, as S_classify's faults)
//   RQ_probe    one lane per virtual entry, tiles of TILE entries (entry e = j * BLOCK + t).  The
//               tile's first and last read by two searches in off (two lanes); the offsets of the
//               reads between them staged in LDS where they fit (RQ_SLICE) and searched there by
//               every lane, in global memory where they do not (thousands of empty reads in one
//               tile).  The window's key by rq_window_key from the read's own bases -- the lanes
//               of a wave read consecutive bytes -- looked up with table_find, recorded with
//               put_qrec; the tile's hit total for the scan.  Broken offsets record no hit and
//               touch nothing outside seq[0, n_bases) and off[0 .. n_reads]
//   mask, scan  k_qrec_mask and launch_scan_u64 of the single query, unchanged
//   RQ_emit     Q_emit's shape over the same tiles: windows with at most EMIT_DIRECT hits write
//               their rows themselves, the others are dealt to the whole workgroup; a hit window
//               finds its (read, strand, i) as the probe did; each 16-B row is one int4 store
//   V_keys      one vote_key per row (and the two row faults: a read outside 1 .. n, a strand
//               that is not +-1); hipcub radix sort; hipcub run-length encode (head flags and a
//               scan) -> cells and their votes
//   V_best      per cell a 64-bit atomicMax of vote_pack into its read's word, an atomicAdd of its
//               votes into the read's total: a maximum and an integer sum, the same whatever the
//               order.  V_second: the largest count among the cells that are not the winner.
//               V_write: the six columns of every read
#include <hip/hip_runtime.h>
#include <hipcub/hipcub.hpp>
#include "kmhg_common.h"
#include "kmhg_device.h"
#include "kmhg_kernels.h"
#include "kmhg_readsq.h"
#include "kmhg_readsq_dev.h"

namespace kmhg {

namespace {

// Offsets of one tile's reads held in LDS: a tile of TILE entries spans at most TILE bases, so at
// most TILE + 1 non-empty reads and TILE + 2 offsets; more only with empty reads in between.
constexpr int RQ_SLICE = TILE + 16;
struct ReadSlice {
  int64_t off[RQ_SLICE];
  int64_t r_lo, r_hi;
  int staged;
};

// The reads of entries [v_lo, v_hi], for the whole workgroup.  n_reads >= 1: reads_call refuses
// bases without reads before anything is launched, so off[0 .. 1] exist whatever off holds.
__device__ __forceinline__ void slice_setup(ReadSlice& S, const int64_t* __restrict__ off,
                                            int64_t n_reads, int ns, int64_t v_lo, int64_t v_hi) {
  if (threadIdx.x == 0) S.r_lo = rq_last_le(off, 0, n_reads - 1, ns == 2 ? v_lo >> 1 : v_lo);
  if (threadIdx.x == 64) S.r_hi = rq_last_le(off, 0, n_reads - 1, ns == 2 ? v_hi >> 1 : v_hi);
  __syncthreads();
  if (threadIdx.x == 0) {
    if (S.r_hi < S.r_lo) S.r_hi = S.r_lo;              // (broken offsets)
    S.staged = S.r_hi - S.r_lo + 2 <= RQ_SLICE;
  }
  __syncthreads();
  if (S.staged) {
    const int m = (int)(S.r_hi - S.r_lo) + 2;          // off[r_lo .. r_hi + 1], r_hi + 1 <= n_reads
    for (int i = threadIdx.x; i < m; i += BLOCK) S.off[i] = off[S.r_lo + i];
  }
  __syncthreads();
}

// Entry v's window; false for an entry the offsets do not place (rq_locate).
__device__ __forceinline__ bool slice_window(const ReadSlice& S, const int64_t* __restrict__ off,
                                             int64_t v, int ns, bool rev_only, int64_t n_bases,
                                             RqWin& w, int64_t& read0) {
  const int64_t q = ns == 2 ? v >> 1 : v;
  int64_t a, b;
  if (S.staged) {
    const int64_t r = rq_last_le(S.off, 0, S.r_hi - S.r_lo, q);
    read0 = S.r_lo + r;
    a = S.off[r];
    b = S.off[r + 1];
  } else {
    read0 = rq_last_le(off, S.r_lo, S.r_hi, q);
    a = off[read0];
    b = off[read0 + 1];
  }
  return rq_locate(v, ns, rev_only, a, b, n_bases, w);
}

__global__ void __launch_bounds__(BLOCK)
k_rq_check(const int64_t* __restrict__ off, int64_t n_reads, int64_t n_bases,
           uint32_t* __restrict__ bad) {
  const int64_t i = (int64_t)blockIdx.x * BLOCK + threadIdx.x;
  if (i <= n_reads && !rq_off_ok_at(off, i, n_reads, n_bases)) *bad = 1u;
}

__global__ void __launch_bounds__(BLOCK)
k_rq_probe(const uint8_t* __restrict__ seq, int64_t n_bases, const int64_t* __restrict__ off,
           int64_t n_reads, int k, int ns, int rev_only, const Slot* __restrict__ T, Geom g,
           uint32_t* __restrict__ qrec, uint2* __restrict__ qmulti, int64_t V,
           uint64_t* __restrict__ tile_rows) {
  __shared__ ReadSlice S;
  __shared__ uint64_t sh[8];
  const int64_t tile0 = (int64_t)blockIdx.x * TILE;
  slice_setup(S, off, n_reads, ns, tile0, min(V, tile0 + TILE) - 1);
  uint64_t rows = 0;
#pragma unroll 2
  for (int j = 0; j < WPT; ++j) {
    const int64_t v = tile0 + j * BLOCK + threadIdx.x;
    if (v >= V) continue;
    RqWin w;
    int64_t read0;
    uint64_t key = 0;
    uint32_t count = 0, aux = 0;
    if (slice_window(S, off, v, ns, rev_only != 0, n_bases, w, read0) &&
        rq_window_key(seq + w.a, w.len, k, w.s, w.rc, key))
      table_find(T, g, key, count, aux);
    put_qrec(qrec, qmulti, v, count, aux);
    rows += count;
  }
  uint64_t tot;
  block_excl_scan(rows, sh, tot);
  if (threadIdx.x == 0) tile_rows[blockIdx.x] = tot;
}

constexpr uint32_t RQ_EMIT_DIRECT = 4;
__global__ void __launch_bounds__(BLOCK)
k_rq_emit(const uint32_t* __restrict__ qrec, const uint2* __restrict__ qmulti, int64_t V,
          const int64_t* __restrict__ off, int64_t n_reads, int64_t n_bases, int k, int ns,
          int rev_only, const int32_t* __restrict__ positions,
          const uint64_t* __restrict__ tile_row0, int4* __restrict__ out, uint64_t cap) {
  __shared__ ReadSlice S;
  __shared__ uint64_t incl[TILE];
  __shared__ uint32_t start[TILE];
  __shared__ uint16_t heavy[TILE];
  static_assert(TILE <= 65536, "heavy[] holds tile-local entries");
  __shared__ uint32_t n_heavy;
  __shared__ uint64_t sh[8];
  const int64_t tile0 = (int64_t)blockIdx.x * TILE;
  if (threadIdx.x == 0) n_heavy = 0;
  for (int j = 0; j < WPT; ++j) {
    const int w = j * BLOCK + threadIdx.x;
    const int64_t v = tile0 + w;
    const uint32_t rc = v < V ? qrec[v] : 0u;
    uint2 c = make_uint2(rc ? 1u : 0u, rc);
    if (rc == QREC_MULTI) c = qmulti[v];
    incl[w] = c.x;
    start[w] = c.y;
  }
  __syncthreads();
  uint64_t run = 0;
  uint64_t loc[WPT];
#pragma unroll
  for (int j = 0; j < WPT; ++j) { run += incl[threadIdx.x * WPT + j]; loc[j] = run; }
  uint64_t tot;
  const uint64_t ex = block_excl_scan(run, sh, tot);
#pragma unroll
  for (int j = 0; j < WPT; ++j) incl[threadIdx.x * WPT + j] = loc[j] + ex;
  __syncthreads();
  if (tot == 0) return;                 // uniform: the tile has no row
  slice_setup(S, off, n_reads, ns, tile0, min(V, tile0 + TILE) - 1);
  const uint64_t r0 = tile_row0[blockIdx.x];
#pragma unroll 2
  for (int j = 0; j < WPT; ++j) {
    const int w = j * BLOCK + threadIdx.x;
    const uint64_t before = w ? incl[w - 1] : 0;
    const uint64_t n = incl[w] - before;
    if (n == 0) continue;
    if (n > RQ_EMIT_DIRECT) {
      heavy[atomicAdd(&n_heavy, 1u)] = (uint16_t)w;
      continue;
    }
    RqWin win;
    int64_t read0;
    if (!slice_window(S, off, tile0 + w, ns, rev_only != 0, n_bases, win, read0)) continue;
    const int4 row = make_int4((int32_t)(read0 + 1), win.rc ? -1 : 1, (int32_t)(win.s + k), 0);
    const uint64_t r = r0 + before;
    const uint32_t st0 = start[w];
    if (n == 1) {
      if (r < cap) out[r] = make_int4(row.x, row.y, row.z, (int32_t)st0);
    } else {
      for (uint32_t q = 0; q < (uint32_t)n; ++q)
        if (r + q < cap) out[r + q] = make_int4(row.x, row.y, row.z, positions[st0 + q]);
    }
  }
  __syncthreads();
  const uint32_t nh = n_heavy;
  for (uint32_t h = 0; h < nh; ++h) {
    const uint32_t w = heavy[h];
    const uint64_t before = w ? incl[w - 1] : 0;
    const uint64_t n = incl[w] - before;
    const uint64_t r = r0 + before;
    const uint32_t st0 = start[w];
    RqWin win;
    int64_t read0;
    if (!slice_window(S, off, tile0 + w, ns, rev_only != 0, n_bases, win, read0)) continue;
    const int4 row = make_int4((int32_t)(read0 + 1), win.rc ? -1 : 1, (int32_t)(win.s + k), 0);
    for (uint64_t q = threadIdx.x; q < n; q += BLOCK)
      if (r + q < cap) out[r + q] = make_int4(row.x, row.y, row.z, positions[st0 + (uint32_t)q]);
  }
}

// ------------------------------------------------------------------ reads.kmer.vote
__global__ void __launch_bounds__(BLOCK)
k_vote_keys(const int4* __restrict__ rows, uint64_t n, int64_t n_reads, int k, int64_t band,
            uint64_t* __restrict__ keys, uint32_t* __restrict__ bad) {
  const uint64_t e = (uint64_t)blockIdx.x * BLOCK + threadIdx.x;
  if (e >= n) return;
  const int4 v = rows[e];
  int64_t read0 = (int64_t)v.x - 1;
  if (read0 < 0 || read0 >= n_reads || (v.y != 1 && v.y != -1)) {
    *bad = 1u;
    read0 = 0;                          // (the call fails: the key only has to stay in range)
  }
  keys[e] = vote_key(read0, v.y != 1, vote_bin((int64_t)v.w - (int64_t)v.z + k, band));
}

__global__ void __launch_bounds__(BLOCK)
k_vote_init(int64_t n_reads, uint64_t* __restrict__ best, uint32_t* __restrict__ second,
            uint32_t* __restrict__ total) {
  const int64_t r = (int64_t)blockIdx.x * BLOCK + threadIdx.x;
  if (r >= n_reads) return;
  best[r] = 0;
  second[r] = 0;
  total[r] = 0;
}

__global__ void __launch_bounds__(BLOCK)
k_vote_best(const uint64_t* __restrict__ cell, const uint32_t* __restrict__ votes,
            const uint32_t* __restrict__ n_cells, unsigned long long* __restrict__ best,
            uint32_t* __restrict__ total) {
  const uint64_t c = (uint64_t)blockIdx.x * BLOCK + threadIdx.x;
  if (c >= *n_cells) return;
  const int64_t r = vote_key_read0(cell[c]);
  atomicMax(&best[r], (unsigned long long)vote_pack(votes[c], cell[c]));
  atomicAdd(&total[r], votes[c]);
}

__global__ void __launch_bounds__(BLOCK)
k_vote_second(const uint64_t* __restrict__ cell, const uint32_t* __restrict__ votes,
              const uint32_t* __restrict__ n_cells, const uint64_t* __restrict__ best,
              uint32_t* __restrict__ second) {
  const uint64_t c = (uint64_t)blockIdx.x * BLOCK + threadIdx.x;
  if (c >= *n_cells) return;
  const int64_t r = vote_key_read0(cell[c]);
  if (vote_pack(votes[c], cell[c]) != best[r]) atomicMax(&second[r], votes[c]);
}

__global__ void __launch_bounds__(BLOCK)
k_vote_write(int64_t n_reads, int64_t band, const uint64_t* __restrict__ best,
             const uint32_t* __restrict__ second, const uint32_t* __restrict__ total,
             int32_t* __restrict__ out) {
  const int64_t r = (int64_t)blockIdx.x * BLOCK + threadIdx.x;
  if (r >= n_reads) return;
  const uint64_t p = best[r];
  int32_t* o = out + VOTE_COLS * r;
  o[0] = (int32_t)(r + 1);
  o[1] = p ? vote_pack_strand(p) : 0;
  o[2] = p ? (int32_t)(vote_pack_bin(p) * band) : 0;
  o[3] = (int32_t)vote_pack_count(p);
  o[4] = (int32_t)second[r];
  o[5] = (int32_t)total[r];
}

inline unsigned blocks_of(uint64_t n) { return (unsigned)((n + BLOCK - 1) / BLOCK); }

}  // namespace

void launch_rq_check(const int64_t* off, int64_t n_reads, int64_t n_bases, uint32_t* bad,
                     hipStream_t s) {
  hipLaunchKernelGGL(k_rq_check, dim3(blocks_of((uint64_t)n_reads + 1)), dim3(BLOCK), 0, s, off,
                     n_reads, n_bases, bad);
}
void launch_rq_probe(const uint8_t* seq, int64_t n_bases, const int64_t* off, int64_t n_reads,
                     int k, int ns, bool rev_only, const Slot* T, Geom g, uint32_t* qrec,
                     uint2* qmulti, uint64_t* tile_rows, hipStream_t s) {
  const int64_t V = rq_virtual(n_bases, ns);
  hipLaunchKernelGGL(k_rq_probe, dim3(tiles_for((uint64_t)V)), dim3(BLOCK), 0, s, seq, n_bases,
                     off, n_reads, k, ns, rev_only ? 1 : 0, T, g, qrec, qmulti, V, tile_rows);
}
void launch_rq_emit(const uint32_t* qrec, const uint2* qmulti, const int64_t* off, int64_t n_reads,
                    int64_t n_bases, int k, int ns, bool rev_only, const int32_t* positions,
                    const uint64_t* tile_row0, int32_t* out, uint64_t cap, hipStream_t s) {
  const int64_t V = rq_virtual(n_bases, ns);
  hipLaunchKernelGGL(k_rq_emit, dim3(tiles_for((uint64_t)V)), dim3(BLOCK), 0, s, qrec, qmulti, V,
                     off, n_reads, n_bases, k, ns, rev_only ? 1 : 0, positions, tile_row0,
                     reinterpret_cast<int4*>(out), cap);
}

hipError_t vote_temp_bytes(uint64_t n, size_t* bytes) {
  size_t a = 0, b = 0;
  hipError_t e = hipcub::DeviceRadixSort::SortKeys(nullptr, a, (const uint64_t*)nullptr,
                                                   (uint64_t*)nullptr, (int)n, 0, 64);
  if (e != hipSuccess) return e;
  e = hipcub::DeviceRunLengthEncode::Encode(nullptr, b, (const uint64_t*)nullptr,
                                            (uint64_t*)nullptr, (uint32_t*)nullptr,
                                            (uint32_t*)nullptr, (int)n);
  *bytes = a > b ? a : b;
  return e;
}

hipError_t launch_votes(const int32_t* rows, uint64_t n, int64_t n_reads, int k, int64_t band,
                        uint64_t* keys, uint64_t* cells, uint32_t* votes, uint32_t* n_cells,
                        void* temp, size_t temp_bytes, uint64_t* best, uint32_t* second,
                        uint32_t* total, int32_t* out, uint32_t* bad, hipStream_t s) {
  if (n_reads)
    hipLaunchKernelGGL(k_vote_init, dim3(blocks_of((uint64_t)n_reads)), dim3(BLOCK), 0, s, n_reads,
                       best, second, total);
  if (n) {
    hipLaunchKernelGGL(k_vote_keys, dim3(blocks_of(n)), dim3(BLOCK), 0, s,
                       reinterpret_cast<const int4*>(rows), n, n_reads, k, band, keys, bad);
    size_t tb = temp_bytes;
    hipError_t e = hipcub::DeviceRadixSort::SortKeys(temp, tb, keys, keys + n, (int)n, 0, 64, s);
    if (e != hipSuccess) return e;
    tb = temp_bytes;
    e = hipcub::DeviceRunLengthEncode::Encode(temp, tb, keys + n, cells, votes, n_cells, (int)n, s);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(k_vote_best, dim3(blocks_of(n)), dim3(BLOCK), 0, s, cells, votes, n_cells,
                       reinterpret_cast<unsigned long long*>(best), total);
    hipLaunchKernelGGL(k_vote_second, dim3(blocks_of(n)), dim3(BLOCK), 0, s, cells, votes, n_cells,
                       best, second);
  }
  if (n_reads)
    hipLaunchKernelGGL(k_vote_write, dim3(blocks_of((uint64_t)n_reads)), dim3(BLOCK), 0, s,
                       n_reads, band, best, second, total, out);
  return hipSuccess;
}

}  // namespace kmhg
