// minimizer_check.cpp -- (w,k)-minimizer sampling's host side (kmhg_minimizer.h: the argument rule
// minimizer_w_refusal, the shared rule minimizer_selected, the host mask minimizer_mask_host) on
// the host under ASan + UBSan.  k_minimizer_mask of kmhg_minimizer.hip evaluates the same
// minimizer_selected per window on the device.
//
//   minimizer_check refusals   w = 1 and 256 legal; 0, 257, -1 and int64's extremes refused in the
//                              entries' words; the host mask refuses them and k, L out of range
//                              without touching its output
//   minimizer_check edges      the host mask against a span-by-span restatement written here
//                              (every span, its leftmost minimum) on random ACGT strings, strings
//                              with single Ns and runs of Ns, an N before the last window, "A" x
//                              300 and a period-3 repeat, forward and rc, at w = 1, 2, 5, 19, 255,
//                              256 and, on short strings, Nw - 1, Nw and Nw + 1 (nothing selected)
//
//   minimizer_check plan       the build plan of a sampled request (kmhg_plan.h): a part with
//                              w > 1 and a key stream with w > 1 refused in their words; a whole
//                              sequence at w = 5 compacts first, on key streams without Pack8,
//                              codes or tags, in the unsampled request's geometry; w = 1 plans
//                              what the unsampled request plans
//
// Prints "ok <checks>"; a mismatch prints the case and exits 1; a sanitizer report aborts.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <limits>
#include <string>
#include <vector>

#include "../../kmer_hasher_amd/csrc/kmhg_minimizer.h"
#include "../../kmer_hasher_amd/csrc/kmhg_plan.h"

using namespace kmhg;

static long g_checks = 0;

[[noreturn]] static void die(const char* what, long a = 0, long b = 0, long c = 0) {
  std::printf("FAIL %s %ld %ld %ld\n", what, a, b, c);
  std::exit(1);
}

static int refusals() {
  const char* const text = "w must be between 1 and 256";
  for (int64_t w : {int64_t(1), int64_t(2), int64_t(255), int64_t(256)}) {
    if (minimizer_w_refusal(w)) die("legal refused", (long)w);
    ++g_checks;
  }
  for (int64_t w : {int64_t(0), int64_t(257), int64_t(-1), int64_t(1) << 31,
                    std::numeric_limits<int64_t>::min(), std::numeric_limits<int64_t>::max()}) {
    const char* r = minimizer_w_refusal(w);
    if (!r || std::strcmp(r, text)) die("refusal text");
    ++g_checks;
  }
  const std::string s(40, 'A');
  std::vector<uint8_t> m(40, 7);
  const uint8_t* p = reinterpret_cast<const uint8_t*>(s.data());
  const int bad_w[] = {0, 257, -1};
  for (int w : bad_w)
    if (minimizer_mask_host(p, 40, 5, w, false, m.data()) != -1) die("host mask took w", w);
  if (minimizer_mask_host(p, 40, 0, 2, false, m.data()) != -1) die("k = 0");
  if (minimizer_mask_host(p, 40, 32, 2, false, m.data()) != -1) die("k = 32");
  if (minimizer_mask_host(p, 5, 5, 2, false, m.data()) != -1) die("L = k");
  if (minimizer_mask_host(nullptr, 40, 5, 2, false, m.data()) != -1) die("null seq");
  if (minimizer_mask_host(p, 40, 5, 2, false, nullptr) != -1) die("null mask");
  for (uint8_t x : m)
    if (x != 7) die("a refused call wrote its output");
  g_checks += 9;
  if (minimizer_mask_words(0) != 0 || minimizer_mask_words(1) != 1 || minimizer_mask_words(32) != 1 ||
      minimizer_mask_words(33) != 2)
    die("mask words");
  ++g_checks;
  std::printf("ok %ld\n", g_checks);
  return 0;
}

// The strand as a string of its own: rc(S)[p] = N for an N, else "ACTG"[code ^ 2].
static std::string strand(const std::string& s, bool rc) {
  if (!rc) return s;
  std::string r(s.size(), 'N');
  for (size_t p = 0; p < s.size(); ++p) {
    const unsigned char c = (unsigned char)s[s.size() - 1 - p];
    r[p] = (c | 0x20) == 'n' ? 'N' : "ACTG"[((c >> 1) & 3) ^ 2];
  }
  return r;
}

// Span by span: every run of w valid windows inside [0, Nw) marks its leftmost minimum.
static std::vector<uint8_t> restated(const std::string& s, int k, int w) {
  const int64_t L = (int64_t)s.size(), Nw = L - k + 1;
  std::vector<uint8_t> ok((size_t)Nw), sel((size_t)Nw, 0);
  std::vector<uint64_t> h((size_t)Nw);
  for (int64_t t = 0; t < Nw; ++t) {
    uint64_t key = 0;
    bool v = true;
    for (int i = 0; i < k; ++i) {
      const unsigned char c = (unsigned char)s[(size_t)(t + i)];
      if ((c | 0x20) == 'n') v = false;
      key = (key << 2) | ((c >> 1) & 3);
    }
    if (v && t + k == L && (t == 0 || ((unsigned char)s[(size_t)(t - 1)] | 0x20) == 'n')) v = false;
    ok[(size_t)t] = v;
    h[(size_t)t] = mix64(key);
  }
  for (int64_t t = 0; t + w <= Nw; ++t) {
    int64_t best = t;
    bool all = true;
    for (int64_t u = t; u < t + w; ++u) {
      if (!ok[(size_t)u]) { all = false; break; }
      if (h[(size_t)u] < h[(size_t)best]) best = u;
    }
    if (all) sel[(size_t)best] = 1;
  }
  return sel;
}

static void one(const std::string& s, int k, int w, int id) {
  const int64_t Nw = (int64_t)s.size() - k + 1;
  for (int rc = 0; rc < 2; ++rc) {
    // exactly Nw bytes on the heap: a write past them is a sanitizer report
    std::vector<uint8_t> got((size_t)Nw, 9);
    const int64_t n = minimizer_mask_host(reinterpret_cast<const uint8_t*>(s.data()),
                                          (int64_t)s.size(), k, w, rc != 0, got.data());
    const std::vector<uint8_t> want = restated(strand(s, rc != 0), k, w);
    int64_t nw = 0;
    for (int64_t t = 0; t < Nw; ++t) {
      if (got[(size_t)t] != want[(size_t)t]) die("mask", id, w * 2 + rc, (long)t);
      nw += want[(size_t)t];
    }
    if (n != nw) die("count", id, w, (long)n);
    if (w > Nw && n != 0) die("w beyond Nw selects", id, w);
    ++g_checks;
  }
}

static int edges() {
  uint64_t r = 0x9E3779B97F4A7C15ull;
  auto rnd = [&] { r ^= r << 13; r ^= r >> 7; r ^= r << 17; return r; };
  auto iid = [&](size_t n) {
    std::string s(n, 'A');
    for (auto& c : s) c = "ACGT"[rnd() & 3];
    return s;
  };
  std::vector<std::string> longs;
  longs.push_back(iid(3000));
  { std::string s = iid(2500); s[100] = 'N'; s[101 + 15] = 'n'; s[700] = 'N';
    for (int i = 0; i < 40; ++i) s[(size_t)(1200 + i)] = 'N';
    s[s.size() - 16] = 'N';                       // the char before the last window at k = 15
    longs.push_back(s); }
  longs.push_back(std::string(300, 'A'));
  { std::string s; for (int i = 0; i < 400; ++i) s += "ACG"; longs.push_back(s); }
  { std::string s = iid(600); for (auto& c : s) if (rnd() % 7 == 0) c = (char)(c | 0x20);
    longs.push_back(s); }
  int id = 0;
  for (const std::string& s : longs) {
    for (int k : {5, 15, 31})
      for (int w : {1, 2, 5, 19, 255, 256}) one(s, k, w, id);
    ++id;
    // short pieces: w around the window count
    for (int k : {5, 15, 31})
      for (size_t nwin : {size_t(3), size_t(40), size_t(255)}) {
        const std::string t = s.substr(0, nwin + k - 1);
        const int Nw = (int)nwin;
        for (int w : {1, 2, Nw - 1, Nw, Nw + 1})
          if (w >= 1 && w <= MINIMIZER_W_MAX) one(t, k, w, id);
      }
    ++id;
  }
  // "A" x 300: every window with a full span to its right is selected (equal hashes, leftmost)
  {
    const std::string s(300, 'A');
    const int k = 5, w = 10, Nw = 296;
    std::vector<uint8_t> m((size_t)Nw);
    minimizer_mask_host(reinterpret_cast<const uint8_t*>(s.data()), 300, k, w, false, m.data());
    for (int t = 0; t < Nw; ++t)
      if (m[(size_t)t] != (t + w <= Nw ? 1 : 0)) die("homopolymer", t);
    ++g_checks;
  }
  std::printf("ok %ld\n", g_checks);
  return 0;
}

static int plan() {
  const BuildKnobs kn;
  for (int64_t L : {int64_t(6000), int64_t(10'000'000), int64_t(60'000'000)}) {
    const int k = 21;
    BuildRequest part = BuildRequest::sequence_part(L, k, 1, 4);
    part.w = 5;
    part.n_selected = L / 3;
    const BuildPlan pp = plan_build(part, kn, 2048);
    if (pp.err != KMHG_EINVAL || !pp.msg ||
        std::strcmp(pp.msg, "part builds index every window (w must be 1)"))
      die("a sampled part is planned", (long)L);
    BuildRequest keys = BuildRequest::key_stream(k, 1000);
    keys.w = 5;
    if (plan_build(keys, kn, 2048).err != KMHG_EINVAL) die("a sampled key stream is planned");
    const BuildPlan u = plan_build(BuildRequest::sequence(L, k, true), kn, 2048);
    const BuildPlan s = plan_build(BuildRequest::sequence_sampled(L, k, 5, L / 3), kn, 2048);
    if (s.err != KMHG_OK || !s.sampled || !s.partc || s.is_part || s.bid || s.pack8 ||
        s.want_tags || s.first_pass != 0)
      die("sampled plan", (long)L);
    if (s.geom.nb != u.geom.nb || s.geom.capb != u.geom.capb || s.geom.b0 || s.geom.nbh ||
        s.ntiles != u.ntiles || s.Nw != u.Nw)
      die("sampled geometry", (long)L, s.geom.nb, u.geom.nb);
    if (s.F(-1) != StreamFmt::KeyPos && s.F(-1) != StreamFmt::Packed12) die("dense stream format");
    BuildRequest one = BuildRequest::sequence(L, k, true);
    one.w = 1;
    const BuildPlan o = plan_build(one, kn, 2048);
    if (o.sampled || o.partc != u.partc || o.bid != u.bid || o.pack8 != u.pack8 ||
        o.passes != u.passes || o.R != u.R || o.fmt != u.fmt || o.first_pass != u.first_pass ||
        o.want_tags != u.want_tags || o.geom.nb != u.geom.nb)
      die("w = 1 plans differently", (long)L);
    g_checks += 5;
  }
  std::printf("ok %ld\n", g_checks);
  return 0;
}

int main(int argc, char** argv) {
  if (argc != 2) die("usage: minimizer_check refusals|edges|plan");
  if (!std::strcmp(argv[1], "plan")) return plan();
  if (!std::strcmp(argv[1], "refusals")) return refusals();
  if (!std::strcmp(argv[1], "edges")) return edges();
  die("usage: minimizer_check refusals|edges");
}
