// digit_check.cpp -- the radix digits' 32-bit magic multipliers (kmhg_plan.h: magic32,
// digit32_ok, div_magic32, digit32 -- the code the kernels run for builds of fewer than 2^16
// buckets) against plain division and against the general 64-bit form, exhaustively over the
// 16-bit dividends.  Stand-alone, built with ASan + UBSan (make -C tools/asan digit_check).
//   digit_check divisors   every d in [1, 320] and the bound's edge, every x < 2^16
//   digit_check plans      every (div, R) a one- or two-pass plan makes for up to 13,824 buckets
//   digit_check predicate  what digit32_ok accepts and refuses
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <set>
#include <utility>

#include "../../kmer_hasher_amd/csrc/kmhg_plan.h"

using namespace kmhg;

// the 64-bit form of kmhg_kernels.h / kmhg_build_v2.hip: m = ceil(2^64 / d), 0 for d = 1
static uint64_t magic64(uint32_t d) { return d <= 1 ? 0 : (uint64_t)(~0ull / d) + 1; }
static uint32_t div_magic64(uint32_t x, uint64_t m) {
  return m ? (uint32_t)(((unsigned __int128)x * m) >> 64) : x;
}
static uint32_t digit64(uint32_t b, uint32_t div, uint32_t R, uint32_t& hi) {
  const uint32_t q = div_magic64(b, magic64(div));
  hi = div_magic64(q, magic64(R));
  return q - hi * R;
}

static int fail(const char* what, uint32_t a, uint32_t b, uint32_t c) {
  std::printf("FAIL %s %u %u %u\n", what, a, b, c);
  return 1;
}

static int check_divisor(uint32_t d) {
  const uint32_t m = magic32(d);
  if (d >= 2 && (uint64_t)m != (0x100000000ull + d - 1) / d) return fail("magic32", d, m, 0);
  for (uint32_t x = 0; x < DIGIT32_LIMIT; ++x)
    if (div_magic32(x, m) != x / d) return fail("div", d, x, div_magic32(x, m));
  return 0;
}

static int check_pair(uint32_t div, uint32_t R) {
  const uint32_t md = magic32(div), mr = magic32(R);
  for (uint32_t x = 0; x < DIGIT32_LIMIT; ++x) {
    uint32_t h32, h64;
    const uint32_t d32 = digit32(x, md, mr, R, h32), d64 = digit64(x, div, R, h64);
    if (d32 != d64 || h32 != h64) return fail("pair", div, R, x);
    if (d32 != x / div % R || h32 != x / div / R) return fail("pair-div", div, R, x);
  }
  return 0;
}

int main(int argc, char** argv) {
  const char* mode = argc > 1 ? argv[1] : "";
  if (!std::strcmp(mode, "divisors")) {
    uint32_t n = 0;
    for (uint32_t d = 1; d <= V2_MAXR_IL; ++d, ++n)
      if (check_divisor(d)) return 1;
    for (uint32_t d : {65535u, 65536u, 32768u, 32769u, 13824u, 40000u}) {
      if (check_divisor(d)) return 1;
      ++n;
    }
    std::printf("ok %u\n", n);
    return 0;
  }
  if (!std::strcmp(mode, "plans")) {
    // the radix of every bucket count (and of every part's count: any nb below it) in one and
    // two passes, at every widest radix: pass p divides by R^p
    std::set<std::pair<uint32_t, uint32_t>> pairs;
    for (uint32_t nb = 1; nb <= 13824; ++nb) {
      for (uint32_t maxr : {V2_MAXR_IL, 256u, 118u}) {
        uint32_t R = 0;
        const uint32_t passes = plan_detail::radix_for(nb, maxr, R);
        if (passes > 2) continue;
        if (!digit32_ok(nb, passes == 2 ? R : 1u, R)) return fail("refused", nb, R, passes);
        pairs.insert({1u, R});
        if (passes == 2) pairs.insert({R, R});
      }
    }
    for (const auto& pr : pairs)
      if (check_pair(pr.first, pr.second)) return 1;
    std::printf("ok %zu\n", pairs.size());
    return 0;
  }
  if (!std::strcmp(mode, "predicate")) {
    int bad = 0;
    bad += !digit32_ok(1, 1, 1) || !digit32_ok(13824, 118, 118) || !digit32_ok(65535, 1, 256) ||
           !digit32_ok(65535, 65536, 65536);
    bad += digit32_ok(65536, 1, 256) || digit32_ok(65537, 1, 257) || digit32_ok(1u << 20, 1, 320) ||
           digit32_ok(0xFFFFFFFFu, 1, 2) || digit32_ok(0, 1, 2);
    bad += digit32_ok(100, 65537, 2) || digit32_ok(100, 2, 65537) || digit32_ok(100, 0, 2) ||
           digit32_ok(100, 2, 0);
    // the plan: the headline's 9,766+ buckets take the 32-bit form, a 100 Mbp build does not
    const BuildKnobs kn;
    bad += !plan_build(BuildRequest::sequence(10'000'000, 31, true), kn, 2048).digit32;
    bad += plan_build(BuildRequest::sequence(100'000'000, 31, true), kn, 2048).digit32;
    bad += !plan_build(BuildRequest::sequence_part(10'000'000, 31, 1, 2), kn, 2048).digit32;
    if (bad) return fail("predicate", (uint32_t)bad, 0, 0);
    std::printf("ok\n");
    return 0;
  }
  std::printf("usage: digit_check divisors|plans|predicate\n");
  return 2;
}
