// segrec_check.cpp -- kmhg_segrec.h (the row-free segment route's list search with a hint, the
// membership in a window's record, the start / end classes and the refusal rule) on the host under
// ASan + UBSan.
//
// host_pairs is the device pass restated as one loop over the same functions: every hit of every
// window classified by segrec_classify, the starts' and ends' seg_key collected, paired by
// std::sort, scattered to the start's rank.  naive_segments is the definition (include/kmhgpu.h)
// over a std::set of the rows the records stand for.  Every list lives in an exact-size
// allocation, so a search that leaves its list is an ASan report.
//
//   segrec_check crafted         empty, single and list windows; equal and disjoint neighbour
//                                lists; j = 1 and j = INT32_MAX; every hint, out of range too;
//                                lists that are not ascending (termination only); the refusal rule
//                                with totals around 2^31 and 2^32
//   segrec_check random SEED N   N random record sets: a few windows over a small position range
//                                of varying density, at the low and the high end of the positions
// Prints "ok <checks>" or the first difference (exit 1).
#include <algorithm>
#include <climits>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <random>
#include <set>
#include <utility>
#include <vector>

#include "../../kmer_hasher_amd/csrc/kmhg_segrec.h"

using namespace kmhg;

struct Multi { uint32_t x, y; };
struct Seg {
  int32_t i, j, len;
  bool operator==(const Seg& o) const { return i == o.i && j == o.j && len == o.len; }
};

// The records of some windows' hit sets (each ascending), in exact-size allocations.
struct Records {
  int64_t Nw = 0;
  uint32_t* qrec = nullptr;
  Multi* qmulti = nullptr;
  int32_t* positions = nullptr;
  explicit Records(const std::vector<std::vector<int32_t>>& P) {
    Nw = (int64_t)P.size();
    size_t np = 0;
    for (const auto& p : P) np += p.size() > 1 ? p.size() : 0;
    qrec = (uint32_t*)std::malloc(std::max<size_t>(1, (size_t)Nw) * sizeof(uint32_t));
    qmulti = (Multi*)std::malloc(std::max<size_t>(1, (size_t)Nw) * sizeof(Multi));
    positions = np ? (int32_t*)std::malloc(np * sizeof(int32_t)) : nullptr;
    size_t at = 0;
    for (int64_t s = 0; s < Nw; ++s) {
      const auto& p = P[(size_t)s];
      qmulti[s] = Multi{0xDEADu, 0xFFFFFFF0u};       // read only under SEGREC_MULTI
      if (p.empty()) qrec[s] = 0u;
      else if (p.size() == 1) qrec[s] = (uint32_t)p[0];
      else {
        qrec[s] = SEGREC_MULTI;
        qmulti[s] = Multi{(uint32_t)p.size(), (uint32_t)at};
        for (int32_t v : p) positions[at++] = v;
      }
    }
  }
  ~Records() { std::free(qrec); std::free(qmulti); std::free(positions); }
};

static long checked = 0;
[[noreturn]] static void die(const char* what, const char* why) {
  std::printf("%s: %s\n", what, why);
  std::exit(1);
}

// window s has i = i0 + s
static void host_pairs(const std::vector<std::vector<int32_t>>& P, int32_t i0, const char* what,
                       std::vector<Seg>& out) {
  Records R(P);
  std::vector<std::pair<uint64_t, uint32_t>> st;
  std::vector<uint64_t> en;
  for (int64_t s = 0; s < R.Nw; ++s) {
    const auto& p = P[(size_t)s];
    for (uint32_t q = 0; q < p.size(); ++q) {
      const uint32_t c = segrec_classify(R.qrec, R.qmulti, R.positions, R.Nw, s, q, p[q]);
      const uint64_t key = seg_key(i0 + (int32_t)s, p[q]);
      if (c & SEG_START) st.push_back({key, (uint32_t)st.size()});
      if (c & SEG_END) en.push_back(key);
    }
  }
  out.clear();
  if (st.empty() && en.empty()) return;
  const SegrecRefusal rf = segrec_check_totals(st.size(), en.size());
  if (rf.code != KMHG_OK) die(what, rf.text);
  std::sort(st.begin(), st.end());
  std::sort(en.begin(), en.end());
  out.resize(st.size());
  for (size_t m = 0; m < st.size(); ++m) {
    if ((st[m].first >> 32) != (en[m] >> 32)) die(what, "a pair off its diagonal");
    out[st[m].second] = Seg{seg_key_i(st[m].first), seg_key_j(st[m].first), seg_len(st[m].first, en[m])};
  }
}

static void naive_segments(const std::vector<std::vector<int32_t>>& P, int32_t i0,
                           std::vector<Seg>& out) {
  std::set<std::pair<int64_t, int64_t>> R;
  for (size_t s = 0; s < P.size(); ++s)
    for (int32_t j : P[s]) R.insert({(int64_t)i0 + (int64_t)s, j});
  out.clear();
  for (const auto& v : R) {                          // (i, j) order
    if (R.count({v.first - 1, v.second - 1})) continue;
    int64_t len = 1;
    while (R.count({v.first + len, v.second + len})) ++len;
    out.push_back(Seg{(int32_t)v.first, (int32_t)v.second, (int32_t)len});
  }
}

static void check(const char* what, const std::vector<std::vector<int32_t>>& P, int32_t i0 = 15) {
  std::vector<Seg> got, want;
  host_pairs(P, i0, what, got);
  naive_segments(P, i0, want);
  if (!(got == want)) {
    std::printf("%s: %zu segments, want %zu\n", what, got.size(), want.size());
    std::exit(1);
  }
  int64_t sum = 0, hits = 0;
  for (const Seg& s : got) sum += s.len;
  for (const auto& p : P) hits += (int64_t)p.size();
  if (sum != hits) die(what, "the lengths do not sum to the hits");
  ++checked;
}

// segrec_find against std::binary_search for every target around the list and every hint
static void check_find(const char* what, const std::vector<int32_t>& list) {
  const uint32_t n = (uint32_t)list.size();
  int32_t* p = n ? (int32_t*)std::malloc(n * sizeof(int32_t)) : nullptr;
  if (n) std::memcpy(p, list.data(), n * sizeof(int32_t));
  std::vector<int64_t> targets;
  for (int32_t v : list)
    for (int64_t d = -2; d <= 2; ++d) targets.push_back((int64_t)v + d);
  for (int64_t t : {(int64_t)INT32_MIN, (int64_t)-1, (int64_t)0, (int64_t)1, (int64_t)INT32_MAX}) targets.push_back(t);
  std::vector<uint32_t> hints;
  for (uint32_t h = 0; h < n + 3 && h < 70; ++h) hints.push_back(h);
  for (uint32_t h : {n / 2, n - 1, n, n + 1, 0x7FFFFFFFu, 0x80000000u, 0xFFFFFFFFu}) hints.push_back(h);
  for (int64_t t : targets) {
    if (t < INT32_MIN || t > INT32_MAX) continue;
    const bool want = std::binary_search(list.begin(), list.end(), (int32_t)t);
    for (uint32_t h : hints)
      if (segrec_find(p, n, h, (int32_t)t) != want) {
        std::printf("%s: find(%lld) from hint %u is not %d\n", what, (long long)t, h, (int)want);
        std::exit(1);
      }
  }
  std::free(p);
  ++checked;
}

static std::vector<int32_t> range(int32_t a, int32_t n, int32_t step = 1) {
  std::vector<int32_t> v;
  for (int32_t t = 0; t < n; ++t) v.push_back(a + t * step);
  return v;
}

static void refusal(uint64_t starts, uint64_t ends, int code, const char* text) {
  const SegrecRefusal r = segrec_check_totals(starts, ends);
  if (r.code != code || (text == nullptr) != (r.text == nullptr) || (text && std::strcmp(text, r.text))) {
    std::printf("totals %llu / %llu: code %d\n", (unsigned long long)starts, (unsigned long long)ends, r.code);
    std::exit(1);
  }
  ++checked;
}

static void crafted() {
  const int32_t M = INT32_MAX;
  check_find("empty list", {});
  check_find("one", {7});
  check_find("two", {1, M});
  check_find("extremes", {1, 2, M - 1, M});
  for (int n : {2, 3, 4, 5, 63, 64, 65, 255, 257, 1000}) {
    check_find("consecutive", range(1, n));
    check_find("stride 4", range(3, n, 4));
    check_find("high", range(M - n + 1, n));
  }
  {  // not ascending: any answer, but inside the list and in finite time
    std::mt19937 g(11);
    for (int t = 0; t < 200; ++t) {
      const uint32_t n = 1 + g() % 300;
      int32_t* p = (int32_t*)std::malloc(n * sizeof(int32_t));
      for (uint32_t x = 0; x < n; ++x) p[x] = (int32_t)(g() % 50) + 1;
      for (int r = 0; r < 50; ++r) (void)segrec_find(p, n, (uint32_t)g(), (int32_t)(g() % 52));
      std::free(p);
    }
    ++checked;
  }
  check("no windows", {});
  check("empty windows", {{}, {}, {}});
  check("one hit", {{5}});
  check("single diagonal", {{5}, {6}, {7}, {}, {9}});
  check("single to list", {{5}, {1, 6, 9}, {7}, {2, 8}});
  check("list to none to list", {range(1, 10), {}, range(1, 10)});
  check("equal lists", {range(1, 300), range(1, 300), range(1, 300)});          // a homopolymer
  check("disjoint lists", {range(1, 100, 2), range(1, 100, 2), range(2, 100, 2)});
  check("shifted lists", {range(1, 70, 4), range(2, 70, 4), range(3, 70, 4), range(4, 70, 4), range(5, 69, 4)});   // a period-4 repeat
  check("long beside short", {range(1, 1000), {500}, range(1, 1000), {1}, {2, 1000}});
  check("j = 1", {{1}, {1, 2}, {1, 2, 3}});
  check("j = INT32_MAX", {{M - 2, M}, {M - 1, M}, {M}, {M}});
  check("both ends", {{1, M}, {1, 2, M}, {1, 3, M}}, M - 2);
  check("i at the top", {{1}, {2}, {3}}, M - 2);
  refusal(0, 0, KMHG_EDEVICE, "segment starts and ends do not pair");
  refusal(5, 4, KMHG_EDEVICE, "segment starts and ends do not pair");
  refusal(1, 1, KMHG_OK, nullptr);
  refusal((1ull << 31) - 1, (1ull << 31) - 1, KMHG_OK, nullptr);
  refusal(1ull << 31, 1ull << 31, KMHG_EOVERFLOW, "result has more than 2^31-1 segments");
  refusal((1ull << 31) - 1, 1ull << 31, KMHG_EDEVICE, "segment starts and ends do not pair");
  refusal(1ull << 32, 1ull << 32, KMHG_EOVERFLOW, "result has more than 2^31-1 segments");
  refusal((1ull << 32) + 7, 7, KMHG_EDEVICE, "segment starts and ends do not pair");    // equal modulo 2^32
  refusal(7, (1ull << 32) + 7, KMHG_EDEVICE, "segment starts and ends do not pair");
  refusal((1ull << 32) + 7, (1ull << 32) + 7, KMHG_EOVERFLOW, "result has more than 2^31-1 segments");
}

static void random_sets(unsigned seed, int n) {
  std::mt19937 g(seed);
  for (int t = 0; t < n; ++t) {
    const int Nw = 1 + (int)(g() % 30), W = 1 + (int)(g() % 60);
    const unsigned dens = 1 + g() % 100;             // percent of the grid kept
    const int32_t oj = (g() & 1) ? 1 : INT32_MAX - W + 1;
    const int32_t i0 = (g() & 1) ? 15 : INT32_MAX - Nw + 1;
    std::vector<std::vector<int32_t>> P((size_t)Nw);
    for (int s = 0; s < Nw; ++s)
      for (int j = 0; j < W; ++j)
        if (g() % 100 < dens) P[(size_t)s].push_back(oj + j);
    check("random", P, i0);
  }
}

int main(int argc, char** argv) {
  if (argc >= 2 && !std::strcmp(argv[1], "crafted")) crafted();
  else if (argc >= 4 && !std::strcmp(argv[1], "random")) random_sets((unsigned)std::atoi(argv[2]), std::atoi(argv[3]));
  else { std::fprintf(stderr, "usage: segrec_check crafted | random SEED N\n"); return 2; }
  std::printf("ok %ld\n", checked);
  return 0;
}
