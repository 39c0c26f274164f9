// kmhg_minimizer.h -- (w,k)-minimizer sampling of window starts (no HIP: any C++17 compiler; the
// device path includes the same rule through kmhg_minimizer.hip).
//
// Definition.  Nw = L - k + 1 window starts, 1-based.  valid(s): the build indexes window s (the
// window rule of window_key, kmhg_device.h).  h(s) = mix64(key(s)), the hash the build takes a
// window's bucket from: a bijection of the key, so equal h means equal k-mer.  A span is w
// consecutive window starts [t, t + w - 1] inside [1, Nw], all of them valid.  Window s is
// selected iff some span contains it in which h(s) < h(u) for every earlier u and h(s) <= h(u)
// for every later u -- the leftmost minimum of that span.  A window that lies in no span (fewer
// than w valid windows in a row around it) is never selected; with w = 1 every valid window is.
//
// The rule exists once, as minimizer_selected(): a walk over the window's neighbours.  With
//   a = the windows directly left of s, inside [1, Nw] and valid, with h(u) >  h(s), at most w - 1
//   b = the windows directly right of s, the same, with h(u) >= h(s), at most w - 1
// a span [s - a', s - a' + w - 1] with a' <= a needs w - 1 - a' <= b, so one exists iff
// a + b >= w - 1.  The caller says what a window is (`at(u, h)`: false for a window outside
// [1, Nw] or not valid, else its hash): the kernel reads its tile's hashes from LDS, the host
// function below an array it filled from the string.
//
// The host function restates the window rule char by char, because window_key reads a staged
// tile; tests/test_minimizer_ref.py holds it to the oracle's index on the edge strings, and the
// GPU suite holds the kernel, which does use window_key, to the host function.
//
// For the reverse strand the rule runs on rc(seq) in rc coordinates, N staying N
// (kmhg_revcomp.h): rc(seq)[p] = comp(seq[L - 1 - p]).
//
// tools/asan/minimizer_check runs all of it under ASan + UBSan (tests/test_minimizer_host.py).
#pragma once
#include <stddef.h>
#include <stdint.h>

#include <vector>

#include "kmhg_common.h"

// (hidden: nothing of this header joins the library's dynamic symbols)
#pragma GCC visibility push(hidden)
namespace kmhg {

constexpr int MINIMIZER_W_MAX = 256;

// The sampling entries' w: 1 .. 256.  nullptr: legal; else the entries' words (KMHG_EINVAL).
inline const char* minimizer_w_refusal(int64_t w) {
  return w < 1 || w > MINIMIZER_W_MAX ? "w must be between 1 and 256" : nullptr;
}

// Words of a window bit mask: bit (s - 1) & 31 of word (s - 1) >> 5 for window start s.
inline int64_t minimizer_mask_words(int64_t Nw) { return Nw > 0 ? (Nw + 31) >> 5 : 0; }

// Whether window u (any index type) is selected at sampling w.  at(v, hv): false if v is no
// window of the sequence or not valid, else hv = its hash.
template <class At>
__host__ __device__ inline bool minimizer_selected(const At& at, int64_t u, int w) {
  uint64_t hu = 0, hv = 0;
  if (!at(u, hu)) return false;
  int need = w - 1;                      // neighbours still to be found, left and right together
  for (int64_t v = u + 1; need > 0 && at(v, hv) && hv >= hu; ++v) --need;
  for (int64_t v = u - 1; need > 0 && at(v, hv) && hv > hu; --v) --need;
  return need == 0;
}

// ---------------------------------------------------------------------------- the host mask
// Char p (0-based) of the strand in the stage's terms: its 2-bit code ((c >> 1) & 3,
// src/kmer_util.h:8; complemented on the reverse strand, c ^ 2) and whether it is an N
// (LC(c) == 'n', src/kmer_util.h:10).
struct StrandChars {
  const uint8_t* seq;
  int64_t L;
  bool rc;
  uint32_t code(int64_t p) const {
    const uint32_t c = (uint32_t)(seq[rc ? L - 1 - p : p] >> 1) & 3u;
    return rc ? c ^ 2u : c;
  }
  bool isN(int64_t p) const { return (seq[rc ? L - 1 - p : p] | 0x20) == 'n'; }
};

// mask[s - 1] = 1 iff window start s of the strand is selected at (k, w), else 0; Nw = L - k + 1
// bytes.  Returns the number selected, or -1 for arguments the entries refuse (L <= k, k outside
// 1 .. 31, w outside 1 .. 256).  O(L w) worst case, O(L) expected on random input.
inline int64_t minimizer_mask_host(const uint8_t* seq, int64_t L, int k, int w, bool rc,
                                   uint8_t* mask) {
  if (!seq || !mask || k < 1 || k > 31 || L <= k || minimizer_w_refusal(w)) return -1;
  const int64_t Nw = L - k + 1;
  const StrandChars ch{seq, L, rc};
  std::vector<uint64_t> h((size_t)Nw);
  std::vector<uint8_t> ok((size_t)Nw);
  const uint64_t kmask = (1ull << (2 * k)) - 1ull;
  uint64_t key = 0;
  int64_t run = 0;                       // chars since the last N
  for (int64_t p = 0; p < L; ++p) {
    key = ((key << 2) | ch.code(p)) & kmask;
    run = ch.isN(p) ? 0 : run + 1;
    const int64_t s = p - k + 1;         // the window ending at p (0-based start)
    if (s < 0) continue;
    bool v = run >= k;
    // the last window is dropped when the char before it is an N or it starts the sequence
    if (v && s + k == L && (s == 0 || ch.isN(s - 1))) v = false;
    ok[(size_t)s] = v ? 1 : 0;
    h[(size_t)s] = mix64(key);
  }
  const auto at = [&](int64_t v, uint64_t& hv) {
    if (v < 0 || v >= Nw || !ok[(size_t)v]) return false;
    hv = h[(size_t)v];
    return true;
  };
  int64_t n = 0;
  for (int64_t s = 0; s < Nw; ++s) {
    mask[s] = minimizer_selected(at, s, w) ? 1 : 0;
    n += mask[s];
  }
  return n;
}

}  // namespace kmhg
#pragma GCC visibility pop
