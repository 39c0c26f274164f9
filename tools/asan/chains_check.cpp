// chains_check.cpp -- kmhg_chains.h (the chain pass's parameter and block checks, candidate
// predicate, cost, key packing and window search) on the host under ASan + UBSan.
//
// host_chains is the device pass restated as loops over the same functions: the block checks and
// sort keys, std::sort, the window of every block by chain_window, the minimum key over the
// window, the children as running minima, the surviving links, pointer jumping for
// chain_rounds(B) rounds of four hops, the per-head sums, and the compaction in block order.
// naive_chains is the definition (include/kmhgpu.h): every block looks at every other block.
//
//   chains_check crafted          literal block sets: empty, one block, the max_dist and
//                                 max_drift edges, overlaps, contests and ties, a staircase, the
//                                 extreme coordinates, the refusals and the arithmetic
//   chains_check random SEED N    N random sets of non-overlapping blocks
// Prints "ok <block sets checked>" or the first difference (exit 1).
#include <algorithm>
#include <climits>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <random>
#include <string>
#include <vector>

#include "../../kmer_hasher_amd/csrc/kmhg_chains.h"

using namespace kmhg;

struct Blk { int32_t i, j, span, hits; };
struct Chain {
  int32_t i, j, ie, je, hits, blocks;
  bool operator==(const Chain& o) const {
    return i == o.i && j == o.j && ie == o.ie && je == o.je && hits == o.hits && blocks == o.blocks;
  }
};
struct Result {
  std::vector<Chain> chains;
  std::vector<int32_t> member;
  bool operator==(const Result& o) const { return chains == o.chains && member == o.member; }
};

[[noreturn]] static void die(const std::string& what) {
  std::printf("%s\n", what.c_str());
  std::exit(1);
}

// the faults of a block set, as the keys kernel reports them
static uint32_t faults_of(const std::vector<Blk>& b) {
  uint32_t f = 0;
  for (size_t t = 0; t < b.size(); ++t) {
    const Blk& p = b[t ? t - 1 : 0];
    f |= chain_check_block(t != 0, p.i, p.j, b[t].i, b[t].j, b[t].span, b[t].hits);
  }
  return f;
}

static void host_chains(const std::vector<Blk>& in, int64_t max_dist, int64_t max_drift,
                        int64_t min_hits, Result& out) {
  const std::vector<Blk> b(in);         // capacity == size: an index past B is a report
  const uint32_t B = (uint32_t)b.size();
  out.chains.clear();
  out.member.assign(B, 0);
  if (!B) return;
  if (faults_of(b)) die("fault on valid blocks");
  const uint32_t dist = chain_limit(max_dist), drift = chain_limit(max_drift);
  const uint32_t mh = chain_min_hits(min_hits);
  std::vector<uint64_t> skey(B);
  for (uint32_t t = 0; t < B; ++t) skey[t] = chain_sort_key((int32_t)chain_end(b[t].i, b[t].span), t);
  std::sort(skey.begin(), skey.end());
  std::vector<int32_t> sej(B);
  for (uint32_t r = 0; r < B; ++r) {
    const Blk& a = b.at(chain_sort_key_index(skey[r]));
    sej[r] = (int32_t)chain_end(a.j, a.span);
  }
  std::vector<uint64_t> pred(B, CHAIN_NONE), child(B, CHAIN_NONE);
  for (uint32_t t = 0; t < B; ++t) {
    uint32_t lo, hi;
    chain_window(skey.data(), B, b[t].i, dist, &lo, &hi);
    if (lo > hi || hi > B) die("window outside the keys");
    // nothing outside the window is a candidate
    for (uint32_t r = 0; r < B; ++r) {
      uint32_t c;
      if ((r < lo || r >= hi) &&
          chain_candidate(chain_sort_key_end(skey[r]), sej[r], b[t].i, b[t].j, dist, drift, &c))
        die("a candidate outside its window");
    }
    uint64_t best = CHAIN_NONE;
    for (uint32_t r = lo; r < hi; ++r) {
      uint32_t c;
      if (chain_candidate(chain_sort_key_end(skey.at(r)), sej.at(r), b[t].i, b[t].j, dist, drift, &c))
        best = std::min(best, chain_key(c, chain_sort_key_index(skey[r])));
    }
    pred[t] = best;
    if (best != CHAIN_NONE) {
      uint64_t& w = child.at(chain_key_index(best));
      w = std::min(w, chain_key(chain_key_cost(best), t));
    }
  }
  std::vector<uint32_t> up(B);
  for (uint32_t t = 0; t < B; ++t) {
    up[t] = t;
    if (pred[t] != CHAIN_NONE && chain_key_index(child.at(chain_key_index(pred[t]))) == t)
      up[t] = chain_key_index(pred[t]);
  }
  for (int r = chain_rounds(B); r > 0; --r)
    for (uint32_t t = 0; t < B; ++t) {      // in place, in index order: one of the orders a device has
      uint32_t x = up[t];
      for (int hop = 0; hop < 3; ++hop) x = up.at(x);
      up[t] = x;
    }
  for (uint32_t t = 0; t < B; ++t)
    if (up.at(up[t]) != up[t]) die("pointer jumping did not reach the first block");
  std::vector<uint32_t> hits(B, 0), count(B, 0), cid(B, 0);
  std::vector<int32_t> ie(B, 0), je(B, 0);
  for (uint32_t t = 0; t < B; ++t) {
    hits.at(up[t]) += (uint32_t)b[t].hits;
    count[up[t]] += 1;
    if (child[t] == CHAIN_NONE) {
      if (ie[up[t]]) die("two last blocks in one chain");
      ie[up[t]] = (int32_t)chain_end(b[t].i, b[t].span);
      je[up[t]] = (int32_t)chain_end(b[t].j, b[t].span);
    }
  }
  for (uint32_t t = 0; t < B; ++t)
    if (up[t] == t && hits[t] >= mh) {
      out.chains.push_back(Chain{b[t].i, b[t].j, ie[t], je[t], (int32_t)hits[t], (int32_t)count[t]});
      cid[t] = (uint32_t)out.chains.size();
    }
  for (uint32_t t = 0; t < B; ++t) out.member[t] = (int32_t)cid.at(up[t]);
}

static void naive_chains(const std::vector<Blk>& b, int64_t max_dist, int64_t max_drift,
                         int64_t min_hits, Result& out) {
  const size_t B = b.size();
  std::vector<int64_t> pred(B, -1), cost(B, 0), child(B, -1);
  for (size_t t = 0; t < B; ++t)
    for (size_t a = 0; a < B; ++a) {
      const int64_t gi = (int64_t)b[t].i - ((int64_t)b[a].i + b[a].span - 1) - 1;
      const int64_t gj = (int64_t)b[t].j - ((int64_t)b[a].j + b[a].span - 1) - 1;
      if (gi < 0 || gj < 0 || std::max(gi, gj) > max_dist || std::llabs(gj - gi) > max_drift) continue;
      if (pred[t] < 0 || gi + gj < cost[t]) { pred[t] = (int64_t)a; cost[t] = gi + gj; }
    }
  for (size_t t = 0; t < B; ++t)
    if (pred[t] >= 0 && (child[pred[t]] < 0 || cost[t] < cost[child[pred[t]]])) child[pred[t]] = (int64_t)t;
  out.chains.clear();
  out.member.assign(B, 0);
  std::vector<int64_t> owner(B, -1);
  std::vector<Chain> all;
  for (size_t h = 0; h < B; ++h) {
    if (pred[h] >= 0 && child[pred[h]] == (int64_t)h) continue;       // has a link in
    Chain c{b[h].i, b[h].j, 0, 0, 0, 0};
    int64_t total = 0;
    for (int64_t t = (int64_t)h;; t = child[t]) {
      if (owner[t] >= 0) die("naive: a block in two chains");
      owner[t] = (int64_t)all.size();
      total += b[t].hits;
      c.blocks += 1;
      c.ie = (int32_t)((int64_t)b[t].i + b[t].span - 1);
      c.je = (int32_t)((int64_t)b[t].j + b[t].span - 1);
      if (child[t] < 0) break;
      if (b[child[t]].i <= c.ie || b[child[t]].j <= c.je) die("naive: a chain does not ascend");
    }
    if (total > INT32_MAX) die("naive: hits beyond int32");
    c.hits = (int32_t)total;
    all.push_back(c);
  }
  std::vector<int32_t> number(all.size(), 0);
  for (size_t c = 0; c < all.size(); ++c)
    if (all[c].hits >= min_hits) {
      out.chains.push_back(all[c]);
      number[c] = (int32_t)out.chains.size();
    }
  for (size_t t = 0; t < B; ++t) {
    if (owner[t] < 0) die("naive: a block in no chain");
    out.member[t] = number[owner[t]];
  }
}

static long checked = 0;

static Result check1(const char* what, const std::vector<Blk>& b, int64_t max_dist,
                     int64_t max_drift, int64_t min_hits) {
  Result got, want;
  host_chains(b, max_dist, max_drift, min_hits, got);
  naive_chains(b, max_dist, max_drift, min_hits, want);
  if (!(got == want))
    die(std::string(what) + ": max_dist " + std::to_string(max_dist) + " max_drift " +
        std::to_string(max_drift) + " min_hits " + std::to_string(min_hits) + ": " +
        std::to_string(got.chains.size()) + " chains, want " + std::to_string(want.chains.size()));
  return got;
}

static void check(const char* what, const std::vector<Blk>& b) {
  int64_t hits = 0;
  for (const Blk& x : b) hits += x.hits;
  for (int64_t max_dist : {(int64_t)0, (int64_t)1, (int64_t)3, (int64_t)20, (int64_t)INT32_MAX, (int64_t)1 << 40})
    for (int64_t max_drift : {(int64_t)0, (int64_t)1, (int64_t)5, (int64_t)1 << 40}) {
      const Result r = check1(what, b, max_dist, max_drift, 1);
      int64_t h = 0, n = 0;
      for (const Chain& c : r.chains) { h += c.hits; n += c.blocks; }
      if (h != hits || n != (int64_t)b.size()) die(std::string(what) + ": the sums");
      for (int64_t min_hits : {(int64_t)2, (int64_t)7, (int64_t)1 << 31}) check1(what, b, max_dist, max_drift, min_hits);
    }
  ++checked;
}

static void expect(const char* what, const std::vector<Blk>& b, int64_t max_dist, int64_t max_drift,
                   int64_t min_hits, const std::vector<Chain>& chains,
                   const std::vector<int32_t>& member) {
  Result got;
  host_chains(b, max_dist, max_drift, min_hits, got);
  if (!(got.chains == chains) || got.member != member) die(std::string(what) + ": literal differs");
  ++checked;
}

static void refusals() {
  auto is = [](ChainRefusal r, const char* text) { return r.code == KMHG_EINVAL && !std::strcmp(r.text, text); };
  if (!is(chain_check_params(-1, -1, 0), "max_dist must not be negative") ||
      !is(chain_check_params(0, -1, 0), "max_drift must not be negative") ||
      !is(chain_check_params(0, 0, 0), "min_hits must be a positive integer") ||
      !is(chain_check_params((int64_t)1 << 40, (int64_t)1 << 40, -5), "min_hits must be a positive integer") ||
      chain_check_params(0, 0, 1).code != KMHG_OK ||
      chain_check_params((int64_t)1 << 40, (int64_t)1 << 40, (int64_t)1 << 40).code != KMHG_OK ||
      !is(chain_check_count(-1), "bad block count") || !is(chain_check_count((int64_t)1 << 31), "bad block count") ||
      chain_check_count(0).code != KMHG_OK || chain_check_count(INT32_MAX).code != KMHG_OK)
    die("parameter refusals");
  const int32_t M = INT32_MAX;
  if (faults_of({{1, 1, 1, 1}, {1, 2, 1, 1}, {2, 1, M - 1, 1}}) != 0 ||
      faults_of({{1, 2, 1, 1}, {1, 2, 1, 1}}) != CHAIN_UNSORTED ||          // repeated
      faults_of({{2, 1, 1, 1}, {1, 9, 1, 1}}) != CHAIN_UNSORTED ||
      faults_of({{1, 2, 1, 1}, {1, 1, 1, 1}}) != CHAIN_UNSORTED ||
      faults_of({{1, 1, 0, 1}}) != CHAIN_BAD_BLOCK || faults_of({{1, 1, -3, 1}}) != CHAIN_BAD_BLOCK ||
      faults_of({{1, 1, 2, 0}}) != CHAIN_BAD_BLOCK || faults_of({{1, 1, 2, 3}}) != CHAIN_BAD_BLOCK ||
      faults_of({{0, 1, 1, 1}}) != CHAIN_BAD_BLOCK || faults_of({{1, -1, 1, 1}}) != CHAIN_BAD_BLOCK ||
      faults_of({{2, 1, M, 1}}) != CHAIN_BAD_BLOCK || faults_of({{1, 2, M, 1}}) != CHAIN_BAD_BLOCK ||
      faults_of({{1, 1, M, M}}) != 0 ||
      faults_of({{3, 3, 1, 1}, {2, 2, 0, 1}}) != (CHAIN_UNSORTED | CHAIN_BAD_BLOCK))
    die("block faults");
  if (!is(chain_fault_refusal(CHAIN_UNSORTED | CHAIN_BAD_BLOCK), "blocks are not in ascending (i, j) order") ||
      !is(chain_fault_refusal(CHAIN_BAD_BLOCK),
          "blocks must have i, j >= 1, 1 <= hits <= span and ends within 2^31 - 1") ||
      chain_fault_refusal(0).code != KMHG_OK)
    die("fault refusals");
  ++checked;
}

static void arithmetic() {
  const int32_t M = INT32_MAX;
  uint32_t c = 7;
  // the max_dist edge: gaps (D, D) pass at D, (D + 1, D) does not; the max_drift edge likewise
  if (!chain_candidate(10, 10, 16, 16, 5, 0, &c) || c != 10 || chain_candidate(10, 10, 17, 16, 5, 9, &c) ||
      chain_candidate(10, 10, 16, 17, 5, 9, &c) || !chain_candidate(10, 10, 16, 13, 5, 3, &c) || c != 7 ||
      chain_candidate(10, 10, 16, 13, 5, 2, &c) || !chain_candidate(10, 10, 13, 16, 5, 3, &c) ||
      chain_candidate(10, 10, 13, 16, 5, 2, &c))
    die("candidate edges");
  // overlap by one row in i only, in j only; touching (gap 0) passes
  if (chain_candidate(10, 10, 10, 20, 99, 99, &c) || chain_candidate(10, 10, 20, 10, 99, 99, &c) ||
      !chain_candidate(10, 10, 11, 11, 0, 0, &c) || c != 0)
    die("candidate overlap");
  // the extremes: the largest gaps, "any" limits, a cost below 2^32
  if (!chain_candidate(1, 1, M, M, chain_limit((int64_t)1 << 40), chain_limit(0), &c) || c != 2u * ((uint32_t)M - 2u) ||
      chain_candidate(1, 1, M, M, (uint32_t)M - 3u, 0, &c) || !chain_candidate(1, 1, M, M, (uint32_t)M - 2u, 0, &c) ||
      !chain_candidate(1, M - 1, M, M, 0xFFFFFFFFu, 0xFFFFFFFFu, &c) || c != (uint32_t)M - 2u ||
      chain_candidate(M, M, 1, 1, 0xFFFFFFFFu, 0xFFFFFFFFu, &c))
    die("candidate extremes");
  if (chain_limit(0) != 0u || chain_limit(0xFFFFFFFFll) != 0xFFFFFFFFu || chain_limit((int64_t)1 << 32) != 0xFFFFFFFFu ||
      chain_min_hits(1) != 1u || chain_min_hits(M) != (uint32_t)M || chain_min_hits((int64_t)M + 1) != 0x80000000u ||
      chain_min_hits((int64_t)1 << 40) != 0x80000000u)
    die("limits");
  // key order: cost first, then the index; no key is CHAIN_NONE
  if (!(chain_key(3, 9) < chain_key(4, 0)) || !(chain_key(3, 1) < chain_key(3, 2)) ||
      chain_key(0xFFFFFFFFu, 0x7FFFFFFFu) == CHAIN_NONE || chain_key_cost(chain_key(5, 6)) != 5 ||
      chain_key_index(chain_key(5, 6)) != 6 || chain_sort_key_end(chain_sort_key(M, 3)) != M ||
      chain_sort_key_index(chain_sort_key(M, 0x7FFFFFFEu)) != 0x7FFFFFFEu ||
      !(chain_sort_key(4, 0x7FFFFFFEu) < chain_sort_key(5, 0)))
    die("keys");
  if (chain_rounds(0) != 0 || chain_rounds(1) != 0 || chain_rounds(2) != 1 || chain_rounds(4) != 1 ||
      chain_rounds(5) != 2 || chain_rounds(5000) != 7 || chain_rounds((uint64_t)M) != 16)
    die("rounds");
  const std::vector<uint64_t> keys = {chain_sort_key(3, 0), chain_sort_key(3, 5), chain_sort_key(7, 1), chain_sort_key(M, 2)};
  uint32_t lo, hi;
  chain_window(keys.data(), 4, 8, 4, &lo, &hi);          // ei in [3, 7]
  if (lo != 0 || hi != 3) die("window");
  chain_window(keys.data(), 4, 8, 3, &lo, &hi);          // ei in [4, 7]
  if (lo != 2 || hi != 3) die("window lo");
  chain_window(keys.data(), 4, 3, 0xFFFFFFFFu, &lo, &hi);   // ei <= 2
  if (lo != 0 || hi != 0) die("window empty");
  chain_window(keys.data(), 4, M, 0, &lo, &hi);          // ei == M - 1
  if (lo != 3 || hi != 3) die("window high");
  chain_window(keys.data(), 0, 5, 5, &lo, &hi);
  if (lo != 0 || hi != 0) die("window of nothing");
  ++checked;
}

static void crafted() {
  refusals();
  arithmetic();
  check("empty", {});
  check("one block", {{5, 9, 4, 3}});
  const int64_t ANY = (int64_t)1 << 40;
  // two blocks at gi = gj = D and D + 1 (D = 3): ends (4, 4); starts (8, 8) and (9, 9)
  expect("max_dist edge in", {{1, 1, 4, 4}, {8, 8, 2, 2}}, 3, 0, 1, {{1, 1, 9, 9, 6, 2}}, {1, 1});
  expect("max_dist edge out", {{1, 1, 4, 4}, {9, 9, 2, 2}}, 3, 0, 1, {{1, 1, 4, 4, 4, 1}, {9, 9, 10, 10, 2, 1}}, {1, 2});
  // drift = 2 and 3 at max_drift = 2
  expect("max_drift edge in", {{1, 1, 4, 4}, {6, 8, 2, 2}}, 9, 2, 1, {{1, 1, 7, 9, 6, 2}}, {1, 1});
  expect("max_drift edge out", {{1, 1, 4, 4}, {6, 9, 2, 2}}, 9, 2, 1, {{1, 1, 4, 4, 4, 1}, {6, 9, 7, 10, 2, 1}}, {1, 2});
  // overlap by one row in i only, in j only
  expect("overlap in i", {{1, 1, 4, 4}, {4, 9, 2, 2}}, ANY, ANY, 1, {{1, 1, 4, 4, 4, 1}, {4, 9, 5, 10, 2, 1}}, {1, 2});
  expect("overlap in j", {{1, 1, 4, 4}, {9, 4, 2, 2}}, ANY, ANY, 1, {{1, 1, 4, 4, 4, 1}, {9, 4, 10, 5, 2, 1}}, {1, 2});
  // two successors choose block 0: the nearer (cost 2) wins, the other starts its own chain
  expect("contest", {{1, 1, 4, 4}, {6, 6, 2, 2}, {7, 9, 1, 1}}, 9, 9, 1,
         {{1, 1, 7, 7, 6, 2}, {7, 9, 7, 9, 1, 1}}, {1, 1, 2});
  // two equal-cost predecessors (cost 4 from (1, 3) and from (3, 1)): the lower index wins
  expect("equal predecessors", {{1, 3, 1, 1}, {3, 1, 1, 1}, {5, 5, 1, 1}}, 9, 9, 1,
         {{1, 3, 5, 5, 2, 2}, {3, 1, 3, 1, 1, 1}}, {1, 2, 1});
  // two equal-cost successors (cost 4 to (4, 6) and to (6, 4)): the lower index wins
  expect("equal successors", {{1, 1, 2, 2}, {4, 6, 1, 1}, {6, 4, 1, 1}}, 9, 9, 1,
         {{1, 1, 4, 6, 3, 2}, {6, 4, 6, 4, 1, 1}}, {1, 1, 2});
  // min_hits drops the middle chain: its blocks get 0 and the later chain is renumbered
  expect("min_hits", {{1, 1, 4, 4}, {2, 50, 1, 1}, {6, 6, 2, 2}, {90, 90, 3, 3}}, 9, 9, 2,
         {{1, 1, 7, 7, 6, 2}, {90, 90, 92, 92, 3, 1}}, {1, 0, 1, 2});
  check("contest", {{1, 1, 4, 4}, {6, 6, 2, 2}, {7, 9, 1, 1}});
  check("equal predecessors", {{1, 3, 1, 1}, {3, 1, 1, 1}, {5, 5, 1, 1}});
  check("equal successors", {{1, 1, 2, 2}, {4, 6, 1, 1}, {6, 4, 1, 1}});
  for (int n : {2, 4, 5, 16, 17, 64, 65, 257, 1025}) {      // a staircase: one chain of n blocks
    std::vector<Blk> st;
    for (int t = 0; t < n; ++t) st.push_back({1 + 5 * t, 1 + 5 * t + (t & 1), 3, 2});
    check("staircase", st);
    expect("staircase chain", st, 3, 1, 1,               // gaps (2, 1), (2, 3) alternate
           {{1, 1, 5 * (n - 1) + 3, 5 * (n - 1) + ((n - 1) & 1) + 3, 2 * n, n}}, std::vector<int32_t>(n, 1));
  }
  {  // many short blocks on distinct diagonals before one block: the last examined wins
    std::vector<Blk> b;
    for (int t = 0; t < 300; ++t) b.push_back({1 + t, 2000 - 3 * t, 1, 1});
    b.push_back({302, 2001, 2, 2});
    check("fan", b);
  }
  const int32_t M = INT32_MAX;
  check("extremes", {{1, 1, 2, 2}, {M - 1, M - 1, 2, 1}});
  expect("extremes joined", {{1, 1, 2, 2}, {M - 1, M - 1, 2, 1}}, (int64_t)M - 4, 0, 1, {{1, 1, M, M, 3, 2}}, {1, 1});
  expect("extremes apart", {{1, 1, 2, 2}, {M - 1, M - 1, 2, 1}}, (int64_t)M - 5, 0, 1,
         {{1, 1, 2, 2, 2, 1}, {M - 1, M - 1, M, M, 1, 1}}, {1, 2});
  check("corners", {{1, 1, 1, 1}, {1, M, 1, 1}, {M, 1, 1, 1}, {M, M, 1, 1}});
  check("full span", {{1, 1, M, M}});
}

static void random_sets(unsigned seed, int n) {
  std::mt19937 g(seed);
  for (int t = 0; t < n; ++t) {
    // blocks on a coarse grid of cells, each inside its cell: sorted by (i, j), free of repeats
    const int cells = 2 + (int)(g() % 14), cell = 2 + (int)(g() % 9);
    const unsigned dens = 5 + g() % 95;
    const int32_t oi = (g() & 1) ? 1 : INT32_MAX - cells * cell, oj = (g() & 1) ? 1 : INT32_MAX - cells * cell;
    std::vector<Blk> b;
    for (int ci = 0; ci < cells; ++ci)
      for (int cj = 0; cj < cells; ++cj)
        if (g() % 100 < dens) {
          const int32_t span = 1 + (int32_t)(g() % cell);
          const int32_t di = (int32_t)(g() % (cell - span + 1)), dj = (int32_t)(g() % (cell - span + 1));
          b.push_back({oi + ci * cell + di, oj + cj * cell + dj, span, 1 + (int32_t)(g() % span)});
        }
    std::sort(b.begin(), b.end(), [](const Blk& x, const Blk& y) { return x.i != y.i ? x.i < y.i : x.j < y.j; });
    check("random", b);
  }
}

int main(int argc, char** argv) {
  if (argc >= 2 && !std::strcmp(argv[1], "crafted")) crafted();
  else if (argc >= 4 && !std::strcmp(argv[1], "random")) random_sets((unsigned)std::atoi(argv[2]), std::atoi(argv[3]));
  else { std::fprintf(stderr, "usage: chains_check crafted | random SEED N\n"); return 2; }
  std::printf("ok %ld\n", checked);
  return 0;
}
