// kmhg_revcomp.h -- the reverse-complement stage's word transform and tiling arithmetic (no HIP:
// any C++ compiler; the device path includes the same functions through kmhg_device.h).
//
// A query's reverse complement is never materialised.  The probe stages 16 chars per word as
// 2-bit codes (MSB-first: char i of the word in bits 31 - 2i, 30 - 2i) and N flags (char i in bit
// 15 - i).  For rc(S)[p] = comp(S[L - 1 - p]) a stage word of rc chars [r, r + 16) is the word of
// forward chars [L - r - 16, L - r), mirrored, with every code complemented:
//   code: the 16 two-bit groups in reverse order, XOR 0xAAAAAAAA   ((c + 2) % 4 == c ^ 2, the
//         reference usage script's rev.comp, test.R:31-36: A<->T, C<->G under "ACTG"[code])
//   N:    the 16 flags in reverse order (an N stays an N: it breaks windows on both strands;
//         rev.comp would turn it into a C)
// Everything behind the stage then works in the reverse strand's own coordinates.
//
// tools/asan/revcomp_check runs these against a char-by-char restatement under ASan + UBSan
// (tests/test_revcomp_host.py).
#pragma once
#include <stdint.h>

#include "kmhg_common.h"

namespace kmhg {

// The code word of the mirrored, complemented 16 chars.
__host__ __device__ inline uint32_t rc_code16(uint32_t x) {
  x = ((x >> 2) & 0x33333333u) | ((x & 0x33333333u) << 2);    // pairs of groups
  x = ((x >> 4) & 0x0F0F0F0Fu) | ((x & 0x0F0F0F0Fu) << 4);    // nibbles
  x = (x >> 24) | ((x >> 8) & 0x0000FF00u) | ((x << 8) & 0x00FF0000u) | (x << 24);   // bytes
  return x ^ 0xAAAAAAAAu;
}

// The N-flag word (low 16 bits) of the mirrored 16 chars.
__host__ __device__ inline uint32_t rc_nbit16(uint32_t n) {
  n = ((n >> 1) & 0x5555u) | ((n & 0x5555u) << 1);
  n = ((n >> 2) & 0x3333u) | ((n & 0x3333u) << 2);
  n = ((n >> 4) & 0x0F0Fu) | ((n & 0x0F0Fu) << 4);
  return ((n >> 8) & 0x00FFu) | ((n & 0x00FFu) << 8);
}

// Stage base (an rc char index, possibly negative) of the tile whose first window starts at rc
// char t_start.  The forward stage aligns its base down to a multiple of 16; the rc stage spends
// the same 16 chars of slack to anchor its words at the sequence END instead: base == L (mod 16),
// so stage word w = rc chars [base + 16 w, base + 16 w + 16) is forward chars [c0, c0 + 16) with
// c0 = L - base - 16 (w + 1) a multiple of 16 -- one aligned 16-B load, as on the forward strand.
// The tile's first window sits at stage offset t_start - base in [HALO, HALO + 15].
__host__ __device__ inline int64_t rc_stage_base(int64_t t_start, int64_t L) {
  const int64_t b = t_start - HALO;
  return b - ((b - L) & 15);
}
// First forward char of stage word w of the rc stage at `base`.
__host__ __device__ inline int64_t rc_word_fwd0(int64_t L, int64_t base, int w) {
  return L - base - 16 * (int64_t)(w + 1);
}

}  // namespace kmhg
