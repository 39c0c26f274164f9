// blocks_check.cpp -- kmhg_blocks.h (the block pass's same-diagonal test, gap, span and head
// predicate over the pairing keys of kmhg_segs.h) on the host under ASan + UBSan.
//
// host_blocks is the device pass restated as one loop over the same functions: the segment
// pass's front half (seg_classify, the starts' and ends' seg_key, std::sort), the min_len filter
// on the sorted arrays, blk_head per segment, running sums for the block id and the len prefix,
// the slot array indexed by the first row's rank, and its compaction.  naive_blocks is the
// definition (include/kmhgpu.h): the segments found by walking a std::set of the rows, put into
// a std::map per diagonal and merged by walking each diagonal in ascending i.
//
//   blocks_check crafted          literal row sets: empty, one row, singles on one diagonal at
//                                 the tile sizes, interleaved diagonals, alternating gaps, bridged
//                                 and unbridged dropped segments, the extreme coordinates
//   blocks_check random SEED N    N random row sets on small grids of varying density
// Prints "ok <row sets checked>" or the first difference (exit 1).
#include <algorithm>
#include <climits>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <map>
#include <random>
#include <set>
#include <utility>
#include <vector>

#include "../../kmer_hasher_amd/csrc/kmhg_blocks.h"

using namespace kmhg;

struct Row { int32_t x, y; };
struct Blk {
  int32_t i, j, span, hits;
  bool operator==(const Blk& o) const { return i == o.i && j == o.j && span == o.span && hits == o.hits; }
};

static void host_blocks(const std::vector<Row>& rows, int64_t min_len, int64_t max_gap,
                        int64_t min_hits, std::vector<Blk>& out) {
  const int64_t n = (int64_t)rows.size();
  out.clear();
  const std::vector<Row> exact(rows);   // capacity == size: a search that leaves [0, n) is a report
  std::vector<std::pair<uint64_t, uint32_t>> st;
  std::vector<uint64_t> en;
  for (int64_t t = 0; t < n; ++t) {
    const uint32_t c = seg_classify(exact.data(), t, n);
    if (c & (SEG_UNSORTED | SEG_NONPOS)) { std::printf("fault on valid rows\n"); std::exit(1); }
    const uint64_t key = seg_key(rows[t].x, rows[t].y);
    if (c & SEG_START) st.push_back({key, (uint32_t)st.size()});
    if (c & SEG_END) en.push_back(key);
  }
  if (st.size() != en.size()) { std::printf("starts %zu != ends %zu\n", st.size(), en.size()); std::exit(1); }
  std::sort(st.begin(), st.end());
  std::sort(en.begin(), en.end());
  const size_t S = st.size();
  if (min_len > INT32_MAX || min_hits > INT32_MAX) return;
  // filter: exact-size arrays, so an index past the kept segments is an ASan report
  std::vector<uint64_t> skey, ekey;
  std::vector<uint32_t> rank;
  for (size_t m = 0; m < S; ++m)
    if (seg_len(st[m].first, en[m]) >= min_len) {
      skey.push_back(st[m].first);
      ekey.push_back(en[m]);
      rank.push_back(st[m].second);
    }
  const size_t K = skey.size();
  if (!K) return;
  skey.shrink_to_fit(); ekey.shrink_to_fit(); rank.shrink_to_fit();
  const uint32_t lim = blk_gap_limit(max_gap);
  // heads, block ids and len prefixes (the scans, as running sums)
  std::vector<uint64_t> bstart, bend;
  std::vector<uint32_t> brank, bpre, bpost;
  uint32_t len_before = 0;
  for (size_t m = 0; m < K; ++m) {
    const bool head = m == 0 || blk_head(ekey[m - 1], skey[m], lim);
    if (head) { bstart.push_back(skey[m]); brank.push_back(rank[m]); bpre.push_back(len_before); }
    len_before += (uint32_t)seg_len(skey[m], ekey[m]);
    if (m + 1 == K || blk_head(ekey[m], skey[m + 1], lim)) { bend.push_back(ekey[m]); bpost.push_back(len_before); }
  }
  if (bend.size() != bstart.size()) { std::printf("heads %zu != tails %zu\n", bstart.size(), bend.size()); std::exit(1); }
  std::vector<uint32_t> slot(S, 0u);
  for (size_t b = 0; b < bstart.size(); ++b)
    if ((int64_t)(bpost[b] - bpre[b]) >= min_hits) {
      if (slot.at(brank[b])) { std::printf("two blocks at one rank\n"); std::exit(1); }
      slot[brank[b]] = (uint32_t)b + 1u;
    }
  for (size_t r = 0; r < S; ++r)
    if (slot[r]) {
      const uint32_t b = slot[r] - 1u;
      out.push_back(Blk{seg_key_i(bstart[b]), seg_key_j(bstart[b]), blk_span(bstart[b], bend[b]),
                        (int32_t)(bpost[b] - bpre[b])});
    }
}

static void naive_blocks(const std::vector<Row>& rows, int64_t min_len, int64_t max_gap,
                         int64_t min_hits, std::vector<Blk>& out) {
  std::set<std::pair<int64_t, int64_t>> R;
  for (const Row& v : rows) R.insert({v.x, v.y});
  std::map<int64_t, std::map<int64_t, int64_t>> diag;      // d -> i -> len, kept segments
  for (const Row& v : rows) {
    if (R.count({(int64_t)v.x - 1, (int64_t)v.y - 1})) continue;
    int64_t len = 1;
    while (R.count({(int64_t)v.x + len, (int64_t)v.y + len})) ++len;
    if (len >= min_len) diag[(int64_t)v.y - v.x][v.x] = len;
  }
  std::vector<std::pair<std::pair<int64_t, int64_t>, Blk>> found;
  for (const auto& dg : diag) {
    int64_t i0 = 0, end = 0, hits = 0;
    bool open = false;
    auto close = [&] {
      if (open && hits >= min_hits)
        found.push_back({{i0, i0 + dg.first}, Blk{(int32_t)i0, (int32_t)(i0 + dg.first), (int32_t)(end - i0), (int32_t)hits}});
    };
    for (const auto& sg : dg.second) {
      if (open && sg.first - end <= max_gap) {
        end = sg.first + sg.second;
        hits += sg.second;
      } else {
        close();
        open = true;
        i0 = sg.first;
        end = sg.first + sg.second;
        hits = sg.second;
      }
    }
    close();
  }
  std::sort(found.begin(), found.end(), [](const auto& a, const auto& b) { return a.first < b.first; });
  out.clear();
  for (const auto& f : found) out.push_back(f.second);
}

static long checked = 0;
static void check1(const char* what, const std::vector<Row>& rows, int64_t min_len, int64_t max_gap,
                   int64_t min_hits, std::vector<Blk>* keep = nullptr) {
  std::vector<Blk> got, want;
  host_blocks(rows, min_len, max_gap, min_hits, got);
  naive_blocks(rows, min_len, max_gap, min_hits, want);
  if (!(got == want)) {
    std::printf("%s min_len %lld max_gap %lld min_hits %lld: %zu blocks, want %zu\n", what, (long long)min_len,
                (long long)max_gap, (long long)min_hits, got.size(), want.size());
    std::exit(1);
  }
  if (keep) *keep = got;
}

static void check(const char* what, const std::vector<Row>& rows) {
  for (int64_t min_len : {(int64_t)1, (int64_t)2, (int64_t)3, (int64_t)1 << 31}) {
    int64_t prev = -1;
    for (int64_t max_gap : {(int64_t)0, (int64_t)1, (int64_t)2, (int64_t)3, (int64_t)7, (int64_t)INT32_MAX - 2, (int64_t)1 << 40}) {
      std::vector<Blk> b;
      check1(what, rows, min_len, max_gap, 1, &b);
      int64_t hits = 0;
      for (const Blk& x : b) {
        hits += x.hits;
        if (x.hits > x.span || x.hits < 1) { std::printf("%s: hits %d span %d\n", what, x.hits, x.span); std::exit(1); }
      }
      if (prev >= 0 && hits != prev) { std::printf("%s: hits change with max_gap\n", what); std::exit(1); }
      prev = hits;
      if (max_gap == 0 && min_len == 1 && hits != (int64_t)rows.size()) { std::printf("%s: hits %lld of %zu rows\n", what, (long long)hits, rows.size()); std::exit(1); }
      for (int64_t min_hits : {(int64_t)2, (int64_t)5, (int64_t)1 << 31}) check1(what, rows, min_len, max_gap, min_hits);
    }
  }
  ++checked;
}

static void expect(const char* what, const std::vector<Row>& rows, int64_t min_len, int64_t max_gap,
                   int64_t min_hits, const std::vector<Blk>& want) {
  std::vector<Blk> got;
  host_blocks(rows, min_len, max_gap, min_hits, got);
  if (!(got == want)) { std::printf("%s: literal differs (%zu blocks, want %zu)\n", what, got.size(), want.size()); std::exit(1); }
  ++checked;
}

// segments {i, j, len} as rows, sorted by (i, j)
static std::vector<Row> rows_of(const std::vector<std::vector<int32_t>>& segs) {
  std::vector<Row> r;
  for (const auto& s : segs)
    for (int32_t t = 0; t < s[2]; ++t) r.push_back({s[0] + t, s[1] + t});
  std::sort(r.begin(), r.end(), [](const Row& a, const Row& b) { return seg_lex(a) < seg_lex(b); });
  return r;
}

static void crafted() {
  check("empty", {});
  check("one row", {{1, 1}});
  for (int n : {2, 3, 64, 65, 2047, 2048, 2049, 3 * 2048 + 7}) {
    std::vector<Row> a, b;
    for (int t = 0; t < n; ++t) a.push_back({2 * t + 1, 2 * t + 1});   // singles, gaps of 1
    for (int t = 0; t < n; ++t) { b.push_back({2 * t + 1, 2 * t + 1}); b.push_back({2 * t + 1, 2 * t + 6}); }
    check("singles", a);
    check("two diagonals", b);
    expect("singles merged", a, 1, 1, 1, {Blk{1, 1, 2 * n - 1, n}});
    expect("two diagonals merged", b, 1, 1, 1, {Blk{1, 1, 2 * n - 1, n}, Blk{1, 6, 2 * n - 1, n}});
  }
  {  // gaps of 1 and 3 alternate
    std::vector<std::vector<int32_t>> s;
    int32_t i = 1;
    for (int t = 0; t < 2 * 2048 + 5; ++t) { s.push_back({i, i + 2, 1}); i += 1 + ((t & 1) ? 3 : 1); }
    check("alternating gaps", rows_of(s));
  }
  {  // lengths 3, 1, 3, 1, ...: min_len = 2 drops the singles; the kept gap is 1 + 1 + 1 = 3
    std::vector<std::vector<int32_t>> s;
    int32_t i = 1;
    for (int t = 0; t < 2 * 2048 + 3; ++t) { const int32_t len = (t & 1) ? 1 : 3; s.push_back({i, i, len}); i += len + 1; }
    const std::vector<Row> r = rows_of(s);
    check("bridged singles", r);
    const int32_t heads = 2048 + 2;
    expect("bridge holds", r, 2, 3, 1, {Blk{1, 1, 6 * heads - 3, 3 * heads}});
    std::vector<Blk> apart;
    for (int32_t t = 0; t < heads; ++t) apart.push_back(Blk{6 * t + 1, 6 * t + 1, 3, 3});
    expect("bridge too short", r, 2, 2, 1, apart);
  }
  // two diagonals; a dropped segment that is bridged, and one whose absence opens the gap
  const std::vector<Row> lit = rows_of({{1, 1, 3}, {5, 5, 1}, {7, 7, 2}, {2, 9, 2}, {6, 13, 4}});
  check("literal", lit);
  expect("literal gap 0", lit, 1, 0, 1, {Blk{1, 1, 3, 3}, Blk{2, 9, 2, 2}, Blk{5, 5, 1, 1}, Blk{6, 13, 4, 4}, Blk{7, 7, 2, 2}});
  expect("literal gap 1", lit, 1, 1, 1, {Blk{1, 1, 8, 6}, Blk{2, 9, 2, 2}, Blk{6, 13, 4, 4}});
  expect("literal bridged", lit, 2, 3, 1, {Blk{1, 1, 8, 5}, Blk{2, 9, 8, 6}});
  expect("literal gap opened", lit, 2, 2, 1, {Blk{1, 1, 3, 3}, Blk{2, 9, 8, 6}, Blk{7, 7, 2, 2}});
  expect("literal min_hits", lit, 1, 2, 5, {Blk{1, 1, 8, 6}, Blk{2, 9, 8, 6}});
  const int32_t M = INT32_MAX;
  const std::vector<Row> ext = {{1, 1}, {2, 2}, {M - 1, M - 1}, {M, M}};
  check("extremes", ext);
  expect("extremes apart", ext, 1, (int64_t)M - 5, 1, {Blk{1, 1, 2, 2}, Blk{M - 1, M - 1, 2, 2}});
  expect("extremes joined", ext, 1, (int64_t)M - 4, 1, {Blk{1, 1, M, 4}});
  check("corners", {{1, 1}, {1, M}, {M, 1}, {M, M}});
  check("far diagonals", {{1, M - 1}, {2, M}, {M - 1, 1}, {M, 2}});
  if (blk_gap(seg_key(2, 2), seg_key(M - 1, M - 1)) != (uint32_t)M - 4u || blk_span(seg_key(1, 1), seg_key(M, M)) != M ||
      blk_same_diag(seg_key(1, 2), seg_key(1, 1)) || !blk_same_diag(seg_key(1, M), seg_key(1, M)) ||
      blk_gap_limit((int64_t)1 << 40) != 0xFFFFFFFFu || blk_gap_limit(0) != 0u) { std::printf("arithmetic\n"); std::exit(1); }
  ++checked;
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
  else { std::fprintf(stderr, "usage: blocks_check crafted | random SEED N\n"); return 2; }
  std::printf("ok %ld\n", checked);
  return 0;
}
