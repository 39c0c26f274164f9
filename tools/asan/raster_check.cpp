// raster_check.cpp -- kmhg_raster.h (seq.kmer.raster's frame checks, overflow rule, divisor
// constants, cell index and tile span) on the host under ASan + UBSan.
//
//   raster_check frames           the refusals in their order and words, the legal edge frames
//                                 (width 1, width 2^31 - 1, coordinate 2^31 - 1, 2^26 cells), the
//                                 overflow rule at its two thresholds
//   raster_check divisors         raster_div(x, raster_magic(d)) == x / d: every d in [1, 4096] and
//                                 around every power of two up to 2^31 - 1, against x over
//                                 [0, 2^31) densely near 0, near the top and near every multiple
//                                 boundary sampled, plus a fixed pseudo-random sample
//   raster_check cells            raster_cell against the definition written with plain / on
//                                 int64: edge frames, a frame that excludes everything, negative
//                                 and zero coordinates, coordinate 2^31 - 1; every index it returns
//                                 is written into an exact-size matrix (a stray one is a report)
//   raster_check span             the i-cells touched by `tile` consecutive coordinates never
//                                 exceed raster_tile_span, for every bin width and offset tried
// Prints "ok <cases checked>" or the first difference (exit 1).
#include <climits>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <random>
#include <string>
#include <vector>

#include "../../kmer_hasher_amd/csrc/kmhg_raster.h"

using namespace kmhg;

static const int64_t M = 0x7FFFFFFFll;

static void die(const char* what, long long a = 0, long long b = 0, long long c = 0) {
  std::printf("%s (%lld, %lld, %lld)\n", what, a, b, c);
  std::exit(1);
}

static long long frames() {
  long long n = 0;
  struct Case { RasterFrame f; const char* text; };
  const char* W = "bin widths must be positive integers";
  const char* C = "bin counts must be positive integers";
  const char* Z = "a raster has at most 2^26 cells";
  const char* F = "the frame must lie within 1..2^31-1 on both axes";
  const Case cases[] = {
      {{0, 0, 0, 1, 0, 1ll << 30}, W},  {{1, 1, 1, 0, 1, 1}, W},   {{1, 1, -1, 1, 1, 1}, W},
      {{1, 1, LLONG_MIN, 1, 1, 1}, W},  {{0, 0, 1, 1, 0, 1ll << 30}, C},
      {{1, 1, 1, 1, 1, -1}, C},         {{1, 1, 1, 1, LLONG_MIN, 1}, C},
      {{0, 0, 1, 1, 8192, 8193}, Z},    {{0, 0, 1ll << 40, 1, 1ll << 62, 1ll << 62}, Z},
      {{1, 1, 1, 1, LLONG_MAX, LLONG_MAX}, Z}, {{1, 1, 1, 1, (1ll << 26) + 1, 1}, Z},
      {{0, 1, 1, 1, 4, 4}, F},          {{1, 0, 1, 1, 4, 4}, F},   {{-5, 1, 1, 1, 4, 4}, F},
      {{M, 1, 1, 1, 2, 1}, F},          {{1, 2, 1, M, 1, 1}, F},   {{1, 1, 1ll << 31, 1, 1, 1}, F},
      {{1, 1, 1, LLONG_MAX, 1, 4}, F},  {{M + 1, 1, 1, 1, 1, 1}, F},
      {{LLONG_MAX, 1, 1, 1, 1, 1}, F},  {{1, 1, 33, 1, 1ll << 26, 1}, F},
      {{1, 1, 1, 1, 1, 1}, nullptr},    {{M, M, 1, 1, 1, 1}, nullptr},
      {{1, 1, M, M, 1, 1}, nullptr},    {{1, 1, 1, 1, 8192, 8192}, nullptr},
      {{1, 1, 31, 1, 1ll << 26, 1}, nullptr}, {{M - 3, 5, 2, 7, 2, 9}, nullptr},
      {{2, 2, M - 1, M - 1, 1, 1}, nullptr},
  };
  for (const Case& c : cases) {
    const RasterRefusal r = raster_check_frame(c.f);
    if (c.text == nullptr ? r.code != KMHG_OK
                          : (r.code != KMHG_EINVAL || std::strcmp(r.text, c.text) != 0))
      die("frame refusal", c.f.i_lo, c.f.bin_i, c.f.n_i);
    ++n;
  }
  // the overflow rule: both thresholds at once, nothing else
  const RasterFrame wide{1, 1, 1ll << 16, 1ll << 16, 1, 1}, below{1, 1, 1ll << 16, (1ll << 16) - 1, 1, 1},
      widest{1, 1, M, M, 1, 1};
  if (!raster_may_overflow(wide, 1ull << 32) || raster_may_overflow(wide, (1ull << 32) - 1) ||
      raster_may_overflow(below, ~0ull) || !raster_may_overflow(widest, 1ull << 32) ||
      raster_may_overflow(widest, 2207684196ull))
    die("overflow rule");
  return n + 5;
}

static long long check_div(uint32_t d, uint32_t x) {
  if (raster_div(x, raster_magic(d)) != x / d) die("raster_div", d, x, x / d);
  return 1;
}

static long long divisors() {
  long long n = 0;
  std::vector<uint32_t> ds;
  for (uint32_t d = 1; d <= 4096; ++d) ds.push_back(d);
  for (int p = 12; p <= 31; ++p)
    for (int64_t o = -3; o <= 3; ++o) {
      const int64_t d = (1ll << p) + o;
      if (d >= 1 && d <= M) ds.push_back((uint32_t)d);
    }
  for (uint32_t d : {1000003u, 46u, 1000000007u, 2147483629u, 715827883u, 1431655765u}) ds.push_back(d);
  std::mt19937_64 rng(20240611);
  for (int t = 0; t < 2000; ++t) ds.push_back((uint32_t)(rng() % (uint64_t)M) + 1);
  for (uint32_t d : ds) {
    for (uint32_t x = 0; x < 300; ++x) n += check_div(d, x);
    for (uint32_t x = (uint32_t)M - 300; x <= (uint32_t)M; ++x) n += check_div(d, x);
    // around multiples of d: the only places a quotient can be off by one
    const uint32_t qmax = (uint32_t)M / d;
    for (int t = 0; t < 64; ++t) {
      const uint64_t q = t < 8 ? (uint64_t)t : (t < 16 ? (uint64_t)qmax - (t - 8) : rng() % ((uint64_t)qmax + 1));
      if (q > qmax) continue;
      const uint64_t b = q * d;
      for (int64_t o = -2; o <= 2; ++o) {
        const int64_t x = (int64_t)b + o;
        if (x >= 0 && x <= M) n += check_div(d, (uint32_t)x);
      }
    }
    for (int t = 0; t < 64; ++t) n += check_div(d, (uint32_t)(rng() % ((uint64_t)M + 1)));
  }
  for (uint32_t d = 1; d <= 300; ++d)              // small divisors: every x of a dense stretch
    for (uint32_t x = 0; x < 70000; ++x) n += check_div(d, x);
  return n;
}

// the definition, with plain division on int64; -1: outside
static int64_t naive_cell(const RasterFrame& f, int64_t i, int64_t j) {
  if (i < f.i_lo || j < f.j_lo) return -1;
  const int64_t bi = (i - f.i_lo) / f.bin_i, bj = (j - f.j_lo) / f.bin_j;
  if (bi >= f.n_i || bj >= f.n_j) return -1;
  return bi + f.n_i * bj;
}

static long long cells() {
  long long n = 0;
  const RasterFrame fs[] = {
      {1, 1, 1, 1, 1, 1},       {1, 1, 1, 1, 40, 30},     {3, 5, 1, 1, 7, 9},   {1, 1, 2, 3, 10, 10},
      {10, 9, 7, 64, 5, 3},     {1, 1, M, M, 1, 1},       {M, M, 1, 1, 1, 1},   {M - 1, 1, 1, M, 2, 1},
      {M - 9, M - 9, 3, 4, 3, 2}, {1, 1, 1ll << 29, 1ll << 29, 3, 3}, {2, 2, M - 1, M - 1, 1, 1},
      {1, 1, 46, 46, 1022, 1022}, {M, 7, 1, 1, 1, 1},     {1000, 1000, 1, 1, 1, 1},   // excludes the rest
  };
  std::vector<int64_t> xs;
  for (int64_t v = -3; v <= 70; ++v) xs.push_back(v);
  for (int64_t v : std::initializer_list<int64_t>{INT32_MIN, INT32_MIN + 1, -M, M - 12, M - 11, M - 10, M - 9,
                    M - 8, M - 7, M - 6, M - 5, M - 4, M - 3, M - 2, M - 1, M, 999ll, 1000ll, 1001ll,
                    (1ll << 29), (1ll << 29) + 1, (1ll << 30), (1ll << 30) + 1, 3 * (1ll << 29),
                    3 * (1ll << 29) + 1, 47000ll, 47012ll, 47013ll})
    xs.push_back(v);
  for (const RasterFrame& f : fs) {
    if (raster_check_frame(f).code != KMHG_OK) die("illegal test frame", f.i_lo, f.bin_i, f.n_i);
    const RasterDev d = raster_dev(f);
    std::vector<uint32_t> m((size_t)(f.n_i * f.n_j), 0u);   // exact size: a stray index is a report
    long long inside = 0;
    for (int64_t i : xs)
      for (int64_t j : xs) {
        const uint32_t c = raster_cell(d, (int32_t)i, (int32_t)j);
        const int64_t want = naive_cell(f, i, j);
        if (want < 0 ? c != RASTER_OUT : (int64_t)c != want) die("raster_cell", i, j, want);
        if (c != RASTER_OUT) { ++m[c]; ++inside; }
        ++n;
      }
    long long sum = 0;
    for (uint32_t v : m) sum += v;
    if (sum != inside) die("matrix sum", sum, inside);
  }
  return n;
}

static long long span() {
  long long n = 0;
  for (uint32_t tile : {1u, 64u, 2048u})
    for (uint32_t bin : {1u, 2u, 3u, 7u, 63u, 64u, 65u, 2047u, 2048u, 2049u, 1u << 20, (uint32_t)M}) {
      const uint64_t m = raster_magic(bin);
      for (uint32_t off = 0; off < 2 * 2049u && off < 3 * bin; ++off) {
        const uint32_t first = raster_div(off, m), last = raster_div(off + tile - 1, m);
        if (last - first + 1 > raster_tile_span(tile, bin)) die("tile span", tile, bin, off);
        ++n;
      }
    }
  return n;
}

int main(int argc, char** argv) {
  const std::string mode = argc > 1 ? argv[1] : "";
  long long n;
  if (mode == "frames") n = frames();
  else if (mode == "divisors") n = divisors();
  else if (mode == "cells") n = cells();
  else if (mode == "span") n = span();
  else {
    std::printf("usage: raster_check frames|divisors|cells|span\n");
    return 2;
  }
  std::printf("ok %lld\n", n);
  return 0;
}
