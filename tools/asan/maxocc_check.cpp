// maxocc_check.cpp -- the occurrence cap's host rules (kmhg_querycall.h: max_occ_refusal,
// qrec_kept, qrec_rows, QueryCall::with_max_occ) on the host under ASan + UBSan.  k_qrec_mask of
// kmhg_kernels.hip evaluates the same two record functions per window.
//
//   maxocc_check refusals      the argument rule: 0, 1 and 2^31-1 legal; -1, 2^31, int64's extremes
//                              refused with KMHG_EINVAL and the entry's words; with_max_occ carries
//                              the value and nothing else of a call changes
//   maxocc_check records       kept / dropped at count = max_occ, max_occ - 1, max_occ + 1 for
//                              max_occ = 1, 2, 4, 5, 256, 2^31-2, 2^31-1; no-hit and single-hit
//                              records under every cap; the tile-total contribution of each
//   maxocc_check tile          a 2,048-window tile of mixed records masked in place the way the
//                              kernel does it (records and counts in exact-size arrays): the new
//                              total equals the kept rows counted one by one, kept records are
//                              untouched, a second pass changes nothing
// Prints "ok <cases checked>" or the first difference (exit 1).
#include <climits>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../../kmer_hasher_amd/csrc/kmhg_querycall.h"

using namespace kmhg;

static const int64_t M = 0x7FFFFFFFll;
static const uint32_t MULTI = QREC_MAXOCC_MULTI;

static void die(const char* what, long long a = 0, long long b = 0, long long c = 0) {
  std::printf("%s (%lld, %lld, %lld)\n", what, a, b, c);
  std::exit(1);
}

static long long refusals() {
  long long n = 0;
  const char* W = "max.occ must be between 0 and 2^31-1";
  for (int64_t v : {(int64_t)0, (int64_t)1, (int64_t)2, M - 1, M}) {
    const QueryCall r = max_occ_refusal(v);
    if (r.code != KMHG_OK || r.text != nullptr) die("legal value refused", v);
    ++n;
  }
  for (int64_t v : {(int64_t)-1, (int64_t)-2, M + 1, (int64_t)1 << 32, (int64_t)1 << 40,
                    (int64_t)LLONG_MAX, (int64_t)LLONG_MIN}) {
    const QueryCall r = max_occ_refusal(v);
    if (r.code != KMHG_EINVAL || !r.text || std::strcmp(r.text, W) != 0) die("refusal", v);
    ++n;
  }
  // the value rides on the call; the modes keep it and it keeps them
  const QueryCall c = query_call_range(1000, 15, 7, 900);
  if (c.code != KMHG_OK || c.max_occ != 0) die("default is off");
  const QueryCall d = c.with_max_occ(M).as_runs().on_rc().of_part();
  if (d.max_occ != M || !d.runs || !d.rc || !d.part || d.w0 != 7 || d.w1 != 900 || d.L != 1000 ||
      d.k != 15 || d.code != KMHG_OK)
    die("with_max_occ", d.max_occ);
  const QueryCall e = c.as_runs().with_max_occ(3);
  if (e.max_occ != 3 || !e.runs || e.rc || e.part || e.w0 != 7 || e.w1 != 900) die("order of modes");
  if (d.with_max_occ(0).max_occ != 0) die("back to off");
  return n + 4;
}

static long long records() {
  long long n = 0;
  const uint32_t caps[] = {1u, 2u, 4u, 5u, 256u, (uint32_t)M - 1, (uint32_t)M};
  for (uint32_t cap : caps) {
    // no hit and one hit: kept under every cap, 0 and 1 rows, whatever `count` holds
    for (uint32_t junk : {0u, 1u, 2u, cap, cap + 1u, 0xFFFFFFFFu}) {
      if (!qrec_kept(0u, junk, cap) || qrec_rows(0u, junk, cap) != 0u) die("no hit", cap, junk);
      for (uint32_t pos : {1u, 2u, cap, (uint32_t)M}) {
        if (!qrec_kept(pos, junk, cap) || qrec_rows(pos, junk, cap) != 1u) die("one hit", cap, pos);
        ++n;
      }
      ++n;
    }
    // a multi-hit record: counts are 2 .. 2^31-1 (positions of one index)
    for (int64_t d = -2; d <= 2; ++d) {
      const int64_t cnt = (int64_t)cap + d;
      if (cnt < 2 || cnt > M) continue;
      const bool keep = cnt <= (int64_t)cap;
      if (qrec_kept(MULTI, (uint32_t)cnt, cap) != keep) die("kept", cap, cnt);
      if (qrec_rows(MULTI, (uint32_t)cnt, cap) != (keep ? (uint32_t)cnt : 0u)) die("rows", cap, cnt);
      ++n;
    }
    if (cap >= 2 && (!qrec_kept(MULTI, 2u, cap) || qrec_rows(MULTI, 2u, cap) != 2u)) die("two", cap);
    if (cap < (uint32_t)M && (qrec_kept(MULTI, (uint32_t)M, cap) || qrec_rows(MULTI, (uint32_t)M, cap)))
      die("largest count", cap);
    n += 2;
  }
  // n = 1 keeps unique k-mers only: every multi-hit record goes
  for (uint32_t cnt = 2; cnt < 5000; ++cnt) {
    if (qrec_kept(MULTI, cnt, 1u) || qrec_rows(MULTI, cnt, 1u) != 0u) die("cap one", cnt);
    ++n;
  }
  static_assert(qrec_kept(QREC_MAXOCC_MULTI, 7u, 7u) && !qrec_kept(QREC_MAXOCC_MULTI, 8u, 7u) &&
                    qrec_rows(QREC_MAXOCC_MULTI, 7u, 7u) == 7u,
                "the rule is a constant expression");
  return n;
}

static long long tile() {
  long long n = 0;
  const int T = 2048;
  uint64_t x = 0x9E3779B97F4A7C15ull;
  auto next = [&] { x ^= x << 13; x ^= x >> 7; x ^= x << 17; return x; };
  const uint32_t counts[] = {2u, 3u, 4u, 5u, 255u, 257u, 2100u, (uint32_t)M};
  for (uint32_t cap : {1u, 2u, 4u, 5u, 256u, 2100u, (uint32_t)M}) {
    for (int nw : {1, 7, 255, 256, 257, T - 1, T}) {
      std::vector<uint32_t> rec((size_t)nw), cnt((size_t)nw);     // exact size: a stray index reports
      for (int w = 0; w < nw; ++w) {
        const uint64_t r = next();
        const int kind = (int)(r % 4);
        rec[(size_t)w] = kind == 0 ? 0u : kind == 1 ? (uint32_t)(1 + (r >> 8) % (uint64_t)M) : MULTI;
        cnt[(size_t)w] = counts[(r >> 40) % 8];
      }
      const std::vector<uint32_t> before = rec;
      uint64_t want = 0;
      for (int w = 0; w < nw; ++w) {
        const uint32_t r = before[(size_t)w], c = cnt[(size_t)w];
        want += r == 0 ? 0u : r != MULTI ? 1u : c <= cap ? c : 0u;
      }
      for (int pass = 0; pass < 2; ++pass) {
        uint64_t total = 0;
        for (int w = 0; w < nw; ++w) {                            // k_qrec_mask's body per window
          const uint32_t r = rec[(size_t)w];
          const uint32_t c = r == MULTI ? cnt[(size_t)w] : 1u;
          if (!qrec_kept(r, c, cap)) rec[(size_t)w] = 0u;
          total += qrec_rows(r, c, cap);
        }
        if (total != want) die("tile total", cap, nw, pass);
        for (int w = 0; w < nw; ++w) {
          const uint32_t b = before[(size_t)w];
          const bool gone = b == MULTI && cnt[(size_t)w] > cap;
          if (rec[(size_t)w] != (gone ? 0u : b)) die("record", cap, nw, w);
        }
        ++n;
      }
    }
  }
  return n;
}

int main(int argc, char** argv) {
  if (argc != 2) die("usage: maxocc_check refusals|records|tile");
  long long n = 0;
  if (!std::strcmp(argv[1], "refusals")) n = refusals();
  else if (!std::strcmp(argv[1], "records")) n = records();
  else if (!std::strcmp(argv[1], "tile")) n = tile();
  else die("unknown mode");
  std::printf("ok %lld\n", n);
  return 0;
}
