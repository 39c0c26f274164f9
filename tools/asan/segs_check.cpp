// segs_check.cpp -- kmhg_segs.h (the diagonal-segment pass's key packing, (i, j) compare and
// galloping bounded search) on the host under ASan + UBSan.
//
// host_segments is the device pass restated as one loop over the same functions: classify every
// row with seg_classify, collect the starts' and ends' seg_key in row order, pair them by
// std::sort, scatter (i, j, len) to the start's rank, filter by min_len.  naive_segments is the
// definition (include/kmhgpu.h) over a std::set of the rows: a row starts a segment when
// (i - 1, j - 1) is not a row, and the segment is walked row by row.
//
//   segs_check crafted          literal row sets: empty, one row, one diagonal, all length 1,
//                               interleaved diagonals, full blocks (every window hits every
//                               position), the extreme coordinates, faults
//   segs_check random SEED N    N random row sets on small grids of varying density
// Prints "ok <row sets checked>" or the first difference (exit 1).
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

#include "../../kmer_hasher_amd/csrc/kmhg_segs.h"

using namespace kmhg;

struct Row { int32_t x, y; };
struct Seg {
  int32_t i, j, len;
  bool operator==(const Seg& o) const { return i == o.i && j == o.j && len == o.len; }
};

static uint32_t host_segments(const std::vector<Row>& rows, int64_t min_len, std::vector<Seg>& out) {
  const int64_t n = (int64_t)rows.size();
  // exact-size copy: a search that leaves [0, n) is an ASan report
  Row* r = n ? (Row*)std::malloc((size_t)n * sizeof(Row)) : nullptr;
  if (n) std::memcpy(r, rows.data(), (size_t)n * sizeof(Row));
  std::vector<std::pair<uint64_t, uint32_t>> st;
  std::vector<uint64_t> en;
  uint32_t fault = 0;
  for (int64_t t = 0; t < n; ++t) {
    const uint32_t c = seg_classify(r, t, n);
    fault |= c & (SEG_UNSORTED | SEG_NONPOS);
    const uint64_t key = seg_key(r[t].x, r[t].y);
    if (c & SEG_START) st.push_back({key, (uint32_t)st.size()});
    if (c & SEG_END) en.push_back(key);
  }
  std::free(r);
  out.clear();
  if (fault) return fault;
  if (st.size() != en.size()) { std::printf("starts %zu != ends %zu\n", st.size(), en.size()); std::exit(1); }
  std::sort(st.begin(), st.end());
  std::sort(en.begin(), en.end());
  std::vector<Seg> all(st.size());
  for (size_t m = 0; m < st.size(); ++m) {
    if ((st[m].first >> 32) != (en[m] >> 32)) { std::printf("pair %zu off its diagonal\n", m); std::exit(1); }
    all[st[m].second] = Seg{seg_key_i(st[m].first), seg_key_j(st[m].first), seg_len(st[m].first, en[m])};
  }
  for (const Seg& s : all)
    if (s.len >= min_len) out.push_back(s);
  return 0;
}

static void naive_segments(const std::vector<Row>& rows, int64_t min_len, std::vector<Seg>& out) {
  std::set<std::pair<int64_t, int64_t>> R;
  for (const Row& v : rows) R.insert({v.x, v.y});
  out.clear();
  for (const Row& v : rows) {
    if (R.count({(int64_t)v.x - 1, (int64_t)v.y - 1})) continue;
    int64_t len = 1;
    while (R.count({(int64_t)v.x + len, (int64_t)v.y + len})) ++len;
    if (len >= min_len) out.push_back(Seg{v.x, v.y, (int32_t)len});
  }
}

static long checked = 0;
static void check(const char* what, const std::vector<Row>& rows) {
  int64_t longest = 1;
  for (int64_t min_len : {(int64_t)1, (int64_t)2, (int64_t)3, (int64_t)16, (int64_t)-1, (int64_t)-2}) {
    if (min_len == -1) min_len = longest;
    if (min_len == -2) min_len = longest + 1;
    std::vector<Seg> got, want;
    const uint32_t f = host_segments(rows, min_len, got);
    if (f) { std::printf("%s: fault %u on valid rows\n", what, f); std::exit(1); }
    naive_segments(rows, min_len, want);
    if (!(got == want)) {
      std::printf("%s min_len %lld: %zu segments, want %zu\n", what, (long long)min_len, got.size(), want.size());
      std::exit(1);
    }
    if (min_len == 1) {
      int64_t sum = 0;
      for (const Seg& s : got) { sum += s.len; longest = std::max<int64_t>(longest, s.len); }
      if (sum != (int64_t)rows.size()) { std::printf("%s: lengths sum to %lld of %zu rows\n", what, (long long)sum, rows.size()); std::exit(1); }
    }
  }
  ++checked;
}

static void expect_fault(const char* what, const std::vector<Row>& rows, uint32_t bit) {
  std::vector<Seg> got;
  const uint32_t f = host_segments(rows, 1, got);
  if (!(f & bit)) { std::printf("%s: fault bits %u, want %u\n", what, f, bit); std::exit(1); }
  ++checked;
}

static void crafted() {
  check("empty", {});
  check("one row", {{1, 1}});
  check("one row far", {{7, 3}});
  for (int n : {2, 3, 63, 64, 65, 2047, 2048, 2049, 3 * 2048 + 7}) {
    std::vector<Row> d, u;
    for (int t = 0; t < n; ++t) d.push_back({t + 1, t + 1});          // one diagonal
    for (int t = 0; t < n; ++t) u.push_back({t + 1, 2 * t + 1});      // all length 1
    check("diagonal", d);
    check("singles", u);
  }
  {  // two interleaved diagonals: every neighbour test fails, every search succeeds
    std::vector<Row> r;
    for (int i = 1; i <= 5000; ++i) { r.push_back({i, i}); r.push_back({i, i + 5}); }
    check("interleaved", r);
  }
  for (int m : {2, 3, 17, 70}) {  // every window hits every position: m diagonals of each length
    std::vector<Row> r;
    for (int i = 1; i <= m; ++i) for (int j = 1; j <= m; ++j) r.push_back({i, j});
    check("block", r);
  }
  {  // period-4 repeat: window i hits every position congruent to it
    std::vector<Row> r;
    for (int i = 1; i <= 300; ++i) for (int j = 1 + (i - 1) % 4; j <= 300; j += 4) r.push_back({i, j});
    check("period 4", r);
  }
  const int32_t M = INT32_MAX;
  check("far right", {{1, M - 1}, {2, M}});
  check("far down", {{M - 1, 1}, {M, 2}});
  check("corner", {{M - 1, M - 1}, {M, M}});
  check("corners", {{1, 1}, {1, M}, {M, 1}, {M, M}});
  check("mixed extremes", {{1, 1}, {1, M - 1}, {2, 2}, {2, M}, {M - 1, 1}, {M, 2}});
  for (auto p : {std::pair<int32_t, int32_t>{1, 1}, {1, M}, {M, 1}, {M, M}, {12345, 7}, {7, 12345}}) {
    const uint64_t key = seg_key(p.first, p.second);
    if (seg_key_i(key) != p.first || seg_key_j(key) != p.second) { std::printf("key round trip (%d, %d)\n", p.first, p.second); std::exit(1); }
    ++checked;
  }
  if (!(seg_key(5, 5) < seg_key(1, 2) && seg_key(1, 2) < seg_key(2, 3) && seg_key(M, 1) < seg_key(1, 1) &&
        seg_key(1, 1) < seg_key(1, M))) { std::printf("key order\n"); std::exit(1); }
  expect_fault("descending", {{2, 2}, {1, 1}}, SEG_UNSORTED);
  expect_fault("repeated row", {{1, 1}, {2, 2}, {2, 2}, {3, 3}}, SEG_UNSORTED);
  expect_fault("j descending", {{1, 5}, {1, 4}}, SEG_UNSORTED);
  expect_fault("zero i", {{0, 1}, {1, 2}}, SEG_NONPOS);
  expect_fault("negative j", {{1, -3}}, SEG_NONPOS);
  {  // the searches stay inside [0, n) on unsorted input too
    std::mt19937 g(7);
    std::vector<Row> r;
    for (int t = 0; t < 4000; ++t) r.push_back({(int32_t)(g() % 50) + 1, (int32_t)(g() % 50) + 1});
    std::vector<Seg> got;
    (void)host_segments(r, 1, got);
    ++checked;
  }
}

static void random_sets(unsigned seed, int n) {
  std::mt19937 g(seed);
  for (int t = 0; t < n; ++t) {
    const int W = 1 + (int)(g() % 40), H = 1 + (int)(g() % 40);
    const unsigned dens = 1 + g() % 100;                              // percent of the grid kept
    const int32_t oi = (g() & 1) ? 1 : INT32_MAX - H + 1, oj = (g() & 1) ? 1 : INT32_MAX - W + 1;
    std::vector<Row> r;
    for (int i = 0; i < H; ++i)
      for (int j = 0; j < W; ++j)
        if (g() % 100 < dens) r.push_back({oi + i, oj + j});
    check("random", r);
  }
}

int main(int argc, char** argv) {
  if (argc >= 2 && !std::strcmp(argv[1], "crafted")) crafted();
  else if (argc >= 4 && !std::strcmp(argv[1], "random")) random_sets((unsigned)std::atoi(argv[2]), std::atoi(argv[3]));
  else { std::fprintf(stderr, "usage: segs_check crafted | random SEED N\n"); return 2; }
  std::printf("ok %ld\n", checked);
  return 0;
}
