// readsq_check.cpp -- kmhg_readsq.h (the host side of reads.kmer.pos / reads.kmer.vote) against
// plain restatements, under ASan + UBSan (tools/asan/Makefile, tests/test_readsq_host.py).
//
//   readsq_check map K       batches at k = K -- empty reads; reads of k - 1, k and k + 1 bases;
//                            5,000 one-base reads; one read of three tiles; mixtures -- on one
//                            strand and on both: every virtual entry's (read, strand, window) by
//                            rq_last_le + rq_locate == a linear scan over the reads; rq_entry is
//                            its inverse; the offsets pass rq_off_ok_at, and broken ones (a
//                            decrease, a wrong first or last entry) are refused and locate nothing
//                            outside the buffers
//   readsq_check window K SEED  reads over ACGT, N, n, lower case and ambiguity characters,
//                            every length 0 .. K + 3 and longer ones: rq_window_key on the
//                            reverse strand == the forward rule applied to an explicitly reversed
//                            and complemented copy, and the forward rule == the reference's walk
//                            restated char by char; in forward coordinates window 0's mirror is
//                            dropped iff the read has exactly k bases or read[k] is N
//   readsq_check refusals    every refusal of reads_call, reads_off_refusal, rq_fill_refusal and
//                            vote_refusal with its code, and the calls they accept
//   readsq_check votes SEED  vote_bin == floor division for negative and positive pos at bands 1,
//                            7, 64 and 2^30; vote_key orders by read, forward first, bin; the
//                            largest vote_pack is the most votes, then forward, then the smaller
//                            bin, and unpacks to what was packed; rq_rows_guess / rq_rows_bytes
// Prints "ok <checks>" and exits 0, or the first difference and exits 1.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "../../kmer_hasher_amd/csrc/kmhg_readsq.h"

using namespace kmhg;

namespace {

uint64_t g_checks = 0;
#define CHECK(cond, ...)                                  \
  do {                                                    \
    ++g_checks;                                           \
    if (!(cond)) {                                        \
      fprintf(stdout, "FAIL %s:%d: ", __FILE__, __LINE__); \
      fprintf(stdout, __VA_ARGS__);                       \
      fprintf(stdout, "\n");                              \
      exit(1);                                            \
    }                                                     \
  } while (0)

struct Rng {
  uint64_t s;
  uint64_t next() {
    s += 0x9E3779B97F4A7C15ull;
    uint64_t z = s;
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    return z ^ (z >> 31);
  }
  uint64_t below(uint64_t n) { return next() % n; }
};

constexpr int64_t TILE_W = TILE;

// ---------------------------------------------------------------- map
void check_batch(const std::vector<int64_t>& lens, int ns, bool rev_only) {
  const int64_t n = (int64_t)lens.size();
  std::vector<int64_t> off(n + 1, 0);
  for (int64_t r = 0; r < n; ++r) off[r + 1] = off[r] + lens[r];
  const int64_t nb = off[n];
  CHECK(reads_off_refusal(off.data(), n, nb).code == KMHG_OK, "good offsets refused");
  for (int64_t i = 0; i <= n; ++i) CHECK(rq_off_ok_at(off.data(), i, n, nb), "entry %lld", (long long)i);
  const int64_t V = rq_virtual(nb, ns);
  CHECK(V == nb * ns, "virtual size");
  int64_t v = 0;                                  // the linear scan: entries in read order
  for (int64_t r = 0; r < n; ++r) {
    for (int st = 0; st < ns; ++st) {
      for (int64_t s = 0; s < lens[r]; ++s, ++v) {
        const int64_t q = ns == 2 ? v >> 1 : v;
        const int64_t got = rq_last_le(off.data(), 0, n - 1, q);
        CHECK(got == r, "entry %lld: read %lld, want %lld", (long long)v, (long long)got, (long long)r);
        RqWin w;
        CHECK(rq_locate(v, ns, rev_only, off[got], off[got + 1], nb, w), "entry %lld not placed", (long long)v);
        CHECK(w.a == off[r] && w.len == lens[r] && w.s == s, "entry %lld: window", (long long)v);
        CHECK(w.rc == (ns == 2 ? st == 1 : rev_only), "entry %lld: strand", (long long)v);
        CHECK(rq_entry(w.a, w.len, ns, ns == 2 && st == 1, s) == v, "entry %lld: inverse", (long long)v);
        // a slice search (the kernels' LDS copy) finds the same read
        const int64_t lo = r > 3 ? r - 3 : 0, hi = r + 2 < n ? r + 2 : n - 1;
        if (off[lo] <= q) CHECK(rq_last_le(off.data(), lo, hi, q) == r, "entry %lld: slice", (long long)v);
      }
    }
  }
  CHECK(v == V, "entries %lld of %lld", (long long)v, (long long)V);
  if (n < 1 || nb < 2) return;
  // broken offsets: refused, and whatever they place stays inside [0, nb)
  for (int kind = 0; kind < 3; ++kind) {
    std::vector<int64_t> bad = off;
    if (kind == 0) bad[0] = 1;
    if (kind == 1) bad[n] = nb - 1;
    if (kind == 2 && n < 2) continue;
    if (kind == 2) bad[n / 2] = bad[n / 2 + 1] + 1;   // a decrease (1 <= n / 2 < n)
    CHECK(reads_off_refusal(bad.data(), n, nb).code == KMHG_EINVAL, "bad offsets %d accepted", kind);
    bool flagged = false;
    for (int64_t i = 0; i <= n; ++i) flagged |= !rq_off_ok_at(bad.data(), i, n, nb);
    CHECK(flagged, "bad offsets %d not flagged", kind);
    for (int64_t e = 0; e < V; e += (V > 4096 ? 7 : 1)) {
      const int64_t q = ns == 2 ? e >> 1 : e;
      const int64_t r = rq_last_le(bad.data(), 0, n - 1, q);
      CHECK(r >= 0 && r < n, "bad offsets: read out of range");
      RqWin w;
      if (rq_locate(e, ns, rev_only, bad[r], bad[r + 1], nb, w))
        CHECK(w.a >= 0 && w.len >= 0 && w.a + w.len <= nb && w.s >= 0 && w.s < w.len,
              "bad offsets: window leaves the buffer");
    }
  }
}

void run_map(int k) {
  std::vector<std::vector<int64_t>> batches = {
      {}, {0}, {0, 0, 0}, {k - 1, k, k + 1}, {0, k, 0, 0, k + 1, 0}, {3 * TILE_W},
      {150, 3 * TILE_W, 150}, {TILE_W - 1, 1, 1}, {TILE_W, 0, TILE_W + 1}};
  batches.push_back(std::vector<int64_t>(5000, 1));
  std::vector<int64_t> mix(5000, 1);
  for (size_t i = 0; i < mix.size(); i += 3) mix[i] = 0;
  mix.push_back(150);
  mix.push_back(2 * TILE_W + 300);
  mix.push_back(k);
  batches.push_back(mix);
  for (const auto& b : batches) {
    check_batch(b, 1, false);
    check_batch(b, 1, true);
    check_batch(b, 2, false);
  }
}

// ---------------------------------------------------------------- window
unsigned char rc_char(unsigned char c) {          // include/kmhgpu.h: N stays N, else by its code
  if ((c | 0x20u) == 'n') return 'N';
  return (unsigned char)"ACTG"[((c >> 1) & 3u) ^ 2u];
}

// The reference's walk with the read as the whole sequence, char by char.
bool walk_key(const std::string& s, int k, int64_t w, uint64_t& key) {
  const int64_t L = (int64_t)s.size();
  if (w + k > L) return false;
  for (int i = 0; i < k; ++i)
    if ((s[w + i] | 0x20) == 'n') return false;
  if (w + k == L && (w == 0 || (s[w - 1] | 0x20) == 'n')) return false;
  key = 0;
  for (int i = 0; i < k; ++i) key = (key << 2) | (((unsigned char)s[w + i] >> 1) & 3u);
  return true;
}

void run_window(int k, uint64_t seed) {
  Rng rng{seed};
  const char alpha[] = "ACGTACGTACGTACGTacgtNnRYKMSWBDHV-.";
  std::vector<int> lens;
  for (int l = 0; l <= k + 3; ++l) lens.push_back(l);
  for (int l : {2 * k, 2 * k + 1, 150, 333}) lens.push_back(l);
  for (int rep = 0; rep < 200; ++rep) {
    for (int len : lens) {
      std::string s((size_t)len, 'A');
      for (auto& c : s) c = alpha[rng.below(rep % 4 == 0 ? 4 : sizeof(alpha) - 1)];
      if (len > k && rep % 5 == 1) s[(size_t)k] = 'N';          // the mirrored drop's trigger
      if (len > k && rep % 5 == 2) s[(size_t)(len - k - 1)] = 'n';   // the forward drop's
      std::string rc(s.rbegin(), s.rend());
      for (auto& c : rc) c = (char)rc_char((unsigned char)c);
      // heap copies of exactly len bytes: ASan sees any read outside the read
      std::vector<uint8_t> fwd(s.begin(), s.end()), rev(rc.begin(), rc.end());
      for (int64_t w = -1; w <= len; ++w) {
        uint64_t a = 0, b = 0, c = 0, d = 0;
        const bool va = rq_window_key(fwd.data(), len, k, w, false, a);
        const bool vb = w >= 0 && walk_key(s, k, w, b);
        CHECK(va == vb && (!va || a == b), "forward len %d w %lld", len, (long long)w);
        const bool vc = rq_window_key(fwd.data(), len, k, w, true, c);
        const bool vd = rq_window_key(rev.data(), len, k, w, false, d);
        CHECK(vc == vd && (!vc || c == d), "reverse len %d w %lld", len, (long long)w);
      }
      if (len >= k) {                      // forward window 0 is rc window len - k
        bool clean = true;
        for (int i = 0; i < k; ++i) clean &= (s[(size_t)i] | 0x20) != 'n';
        uint64_t key = 0;
        const bool kept = rq_window_key(fwd.data(), len, k, len - k, true, key);
        const bool dropped = len == k || (s[(size_t)k] | 0x20) == 'n';
        CHECK(kept == (clean && !dropped), "mirrored end-drop len %d", len);
      }
    }
  }
}

// ---------------------------------------------------------------- refusals
void run_refusals() {
  const int64_t big = (int64_t)INT32_MAX;
  CHECK(reads_call(100, 3, 15, 3, 0, 15, 1).code == KMHG_OK, "plain call");
  const ReadsCall both = reads_call(100, 3, 15, 3, 0, 15, 1);
  CHECK(both.ns == 2 && !both.rev_only && both.k == 15 && both.n_reads == 3 && both.n_bases == 100, "both");
  const ReadsCall fw = reads_call(100, 3, 1, 1, 0, 15, 1), rv = reads_call(100, 3, 31, 2, 0, 15, 4);
  CHECK(fw.code == KMHG_OK && fw.ns == 1 && !fw.rev_only, "forward");
  CHECK(rv.code == KMHG_OK && rv.ns == 1 && rv.rev_only, "reverse (a sampled index at another k)");
  CHECK(both.with_max_occ(8).max_occ == 8 && both.max_occ == 0, "max_occ");
  for (int k : {0, -1, 32, 100}) {
    const ReadsCall c = reads_call(100, 3, k, 3, 0, 15, 1);
    CHECK(c.code == KMHG_EINVAL && c.text && strstr(c.text, "between 1 and 31"), "k = %d", k);
  }
  for (int st : {0, 4, -1})
    CHECK(reads_call(100, 3, 15, st, 0, 15, 1).code == KMHG_EINVAL, "strands = %d", st);
  CHECK(reads_call(-1, 3, 15, 3, 0, 15, 1).code == KMHG_EINVAL, "negative bases");
  CHECK(reads_call(1, -3, 15, 3, 0, 15, 1).code == KMHG_EINVAL, "negative reads");
  const ReadsCall orphan = reads_call(5, 0, 15, 3, 0, 15, 1);      // bases that no read holds
  CHECK(orphan.code == KMHG_EINVAL && strstr(orphan.text, "non-decreasing"), "bases without reads");
  CHECK(reads_call(0, 0, 15, 3, 0, 15, 1).code == KMHG_OK, "no reads, no bases");
  CHECK(reads_call(0, 4, 15, 3, 0, 15, 1).code == KMHG_OK, "empty reads only");
  const ReadsCall cnt = reads_call(100, 3, 15, 3, 2, 15, 1);
  CHECK(cnt.code == KMHG_EINVAL && strstr(cnt.text, "counts index"), "counts index");
  const ReadsCall smp = reads_call(100, 3, 15, 3, 0, 15, 4);
  CHECK(smp.code == KMHG_EINVAL && strstr(smp.text, "follow-up"), "sampled index at its own k");
  CHECK(reads_call(big - 1, 3, 15, 3, 0, 15, 1).code == KMHG_OK, "2^31 - 2 bases");
  CHECK(reads_call(big, 3, 15, 3, 0, 15, 1).code == KMHG_EOVERFLOW, "2^31 - 1 bases");
  CHECK(reads_call(100, big, 15, 3, 0, 15, 1).code == KMHG_OK, "2^31 - 1 reads");
  CHECK(reads_call(100, big + 1, 15, 3, 0, 15, 1).code == KMHG_EOVERFLOW, "2^31 reads");
  const int64_t zero[1] = {0};
  CHECK(reads_off_refusal(zero, 0, 0).code == KMHG_OK, "no reads");
  CHECK(reads_off_refusal(zero, 0, 5).code == KMHG_EINVAL, "no reads, some bases");
  const int64_t dec[4] = {0, 10, 5, 20}, first[3] = {2, 5, 9}, last[3] = {0, 5, 9};
  CHECK(reads_off_refusal(dec, 3, 20).code == KMHG_EINVAL, "a decrease");
  CHECK(reads_off_refusal(first, 2, 9).code == KMHG_EINVAL, "first not 0");
  CHECK(reads_off_refusal(last, 2, 10).code == KMHG_EINVAL, "last not the length");
  CHECK(reads_off_refusal(last, 2, 9).code == KMHG_OK, "good");
  CHECK(strstr(reads_off_refusal(dec, 3, 20).text, "non-decreasing"), "text");
  CHECK(rq_fill_refusal(big).code == KMHG_OK && rq_fill_refusal(big + 1).code == KMHG_EOVERFLOW, "fill");
  CHECK(vote_refusal(10, 3, 15, 64).code == KMHG_OK, "vote");
  CHECK(vote_refusal(10, 3, 15, 1).code == KMHG_OK && vote_refusal(10, 3, 15, VOTE_BAND_MAX).code == KMHG_OK, "bands");
  CHECK(vote_refusal(10, 3, 15, 0).code == KMHG_EINVAL, "band 0");
  CHECK(vote_refusal(10, 3, 15, VOTE_BAND_MAX + 1).code == KMHG_EINVAL, "band 2^30 + 1");
  CHECK(vote_refusal(10, 3, 0, 64).code == KMHG_EINVAL && vote_refusal(10, 3, 32, 64).code == KMHG_EINVAL, "vote k");
  CHECK(vote_refusal(-1, 3, 15, 64).code == KMHG_EINVAL && vote_refusal(1, -3, 15, 64).code == KMHG_EINVAL, "negative");
  CHECK(vote_refusal(big + 1, 3, 15, 64).code == KMHG_EOVERFLOW, "rows");
  CHECK(vote_refusal(1, big + 1, 15, 64).code == KMHG_EOVERFLOW, "reads");
}

// ---------------------------------------------------------------- votes
int64_t floor_div(int64_t a, int64_t b) {          // by subtraction of the remainder's sign
  int64_t q = a / b, r = a % b;
  return r < 0 ? q - 1 : q;
}

void run_votes(uint64_t seed) {
  Rng rng{seed};
  const int64_t bands[] = {1, 7, 64, VOTE_BAND_MAX};
  const int64_t lim = ((int64_t)1 << 31) + 30;
  for (int64_t band : bands) {
    for (int64_t pos : {(int64_t)0, (int64_t)1, (int64_t)-1, (int64_t)-6, (int64_t)-7, (int64_t)-8, (int64_t)6,
                        (int64_t)7, (int64_t)63, (int64_t)64, (int64_t)-64, (int64_t)-65, lim, -lim + 31})
      CHECK(vote_bin(pos, band) == floor_div(pos, band), "bin %lld / %lld", (long long)pos, (long long)band);
    for (int i = 0; i < 20000; ++i) {
      const int64_t pos = (int64_t)rng.below(2 * (uint64_t)lim) - lim;
      const int64_t b = vote_bin(pos, band);
      CHECK(b == floor_div(pos, band) && b * band <= pos && pos < (b + 1) * band, "bin");
      CHECK(b + ((int64_t)1 << 31) >= 0 && b + ((int64_t)1 << 31) <= (int64_t)UINT32_MAX, "bin fits");
    }
  }
  CHECK(vote_bin(-1, 7) == -1 && vote_bin(-7, 7) == -1 && vote_bin(-8, 7) == -2, "floor, not truncation");
  for (int i = 0; i < 20000; ++i) {
    const int64_t r1 = (int64_t)rng.below(1000), r2 = (int64_t)rng.below(1000);
    const bool s1 = rng.below(2), s2 = rng.below(2);
    const int64_t b1 = (int64_t)rng.below(4000) - 2000, b2 = (int64_t)rng.below(4000) - 2000;
    const uint64_t k1 = vote_key(r1, s1, b1), k2 = vote_key(r2, s2, b2);
    const bool lt = r1 != r2 ? r1 < r2 : s1 != s2 ? !s1 : b1 < b2;
    const bool eq = r1 == r2 && s1 == s2 && b1 == b2;
    CHECK((k1 == k2) == eq && (eq || (k1 < k2) == lt), "key order");
    CHECK(vote_key_read0(k1) == r1, "key read");
    const uint32_t c1 = 1 + (uint32_t)rng.below(5), c2 = 1 + (uint32_t)rng.below(5);
    const uint64_t p1 = vote_pack(c1, k1), p2 = vote_pack(c2, vote_key(r1, s2, b2));
    CHECK(p1 != 0 && vote_pack_count(p1) == c1 && vote_pack_strand(p1) == (s1 ? -1 : 1) &&
              vote_pack_bin(p1) == b1, "pack round trip");
    const bool wins = c1 != c2 ? c1 > c2 : s1 != s2 ? !s1 : b1 < b2;   // over the same read's cell
    if (!(c1 == c2 && s1 == s2 && b1 == b2)) CHECK((p1 > p2) == wins, "winner order");
  }
  const uint64_t top = vote_pack((uint32_t)INT32_MAX, vote_key(RQ_MAX_READS - 1, true, -((int64_t)1 << 31)));
  CHECK(vote_pack_count(top) == (uint32_t)INT32_MAX && vote_pack_bin(top) == -((int64_t)1 << 31), "extremes");
  CHECK(vote_key_read0(vote_key(RQ_MAX_READS - 1, true, ((int64_t)1 << 31) - 1)) == RQ_MAX_READS - 1, "read bits");
  CHECK(rq_rows_guess(0) == 64 && rq_rows_guess(800) == 964, "guess");
  CHECK(rq_rows_bytes(3) == 48 && rq_rows_bytes((uint64_t)INT32_MAX) == 16ull * INT32_MAX, "row bytes");
}

}  // namespace

int main(int argc, char** argv) {
  const std::string mode = argc > 1 ? argv[1] : "";
  if (mode == "map" && argc == 3) run_map(atoi(argv[2]));
  else if (mode == "window" && argc == 4) run_window(atoi(argv[2]), strtoull(argv[3], nullptr, 10));
  else if (mode == "refusals") run_refusals();
  else if (mode == "votes" && argc == 3) run_votes(strtoull(argv[2], nullptr, 10));
  else {
    fprintf(stderr, "usage: readsq_check map K | window K SEED | refusals | votes SEED\n");
    return 2;
  }
  printf("ok %llu\n", (unsigned long long)g_checks);
  return 0;
}
