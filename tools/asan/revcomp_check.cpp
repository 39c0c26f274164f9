// revcomp_check.cpp -- kmhg_revcomp.h (the reverse-complement stage's word transform and tiling
// arithmetic) against a char-by-char restatement, under ASan + UBSan (tools/asan/Makefile,
// tests/test_revcomp_host.py).
//
//   revcomp_check words SEED N    N 16-char words from a seeded stream over ACGT, N, n, lower
//                                 case and the ambiguity characters: rc_code16 / rc_nbit16 of the
//                                 packed word == the packed word of the chars reversed and
//                                 complemented one by one; the transform twice is the identity
//   revcomp_check stage LMAX      for every L <= LMAX and every tile start: the rc stage's words
//                                 are 16-aligned forward blocks, the first window sits HALO ..
//                                 HALO + 15 chars in, and a whole stage assembled word by word
//                                 from a forward string equals the packed rc string
// Prints "ok <checks>" and exits 0, or the first difference and exits 1.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "../../kmer_hasher_amd/csrc/kmhg_revcomp.h"

using namespace kmhg;

namespace {

// the stage's packing of 16 chars (kmhg_device.h pack16): codes MSB-first, N flags MSB-first
void pack16(const unsigned char* c, uint32_t& code, uint32_t& nb) {
  code = 0; nb = 0;
  for (int i = 0; i < 16; ++i) {
    code = (code << 2) | ((c[i] >> 1) & 3u);
    nb = (nb << 1) | (((c[i] | 0x20u) == 'n') ? 1u : 0u);
  }
}

// the definition (include/kmhgpu.h): N stays N, everything else by its 2-bit code
unsigned char rc_char(unsigned char c) {
  if ((c | 0x20u) == 'n') return 'N';
  return (unsigned char)"ACTG"[((c >> 1) & 3u) ^ 2u];
}

uint64_t splitmix(uint64_t& x) {
  uint64_t z = (x += 0x9E3779B97F4A7C15ull);
  z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
  z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
  return z ^ (z >> 31);
}

const char ALPHABET[] = "ACGTacgtNnRYKMSWBDHVrykmswbdhv-.";

int check_words(uint64_t seed, long n) {
  long checks = 0;
  const size_t na = sizeof(ALPHABET) - 1;
  for (long it = 0; it < n; ++it) {
    unsigned char f[16], r[16];
    for (int i = 0; i < 16; ++i) f[i] = (unsigned char)ALPHABET[splitmix(seed) % na];
    for (int i = 0; i < 16; ++i) r[i] = rc_char(f[15 - i]);
    uint32_t cf, nf, cr, nr;
    pack16(f, cf, nf);
    pack16(r, cr, nr);
    // codes under an N flag are never read (no valid window holds an N): compare the others
    uint32_t keep = 0;
    for (int i = 0; i < 16; ++i)
      if (!((nr >> (15 - i)) & 1u)) keep |= 3u << (30 - 2 * i);
    if ((rc_code16(cf) & keep) != (cr & keep) || rc_nbit16(nf) != nr) {
      std::printf("word %ld: '%.16s' code %08x -> %08x want %08x (mask %08x), N %04x -> %04x want %04x\n",
                  it, (const char*)f, cf, rc_code16(cf), cr, keep, nf, rc_nbit16(nf), nr);
      return 1;
    }
    if (rc_code16(rc_code16(cf)) != cf || rc_nbit16(rc_nbit16(nf)) != nf) {
      std::printf("word %ld: not an involution\n", it);
      return 1;
    }
    checks += 4;
  }
  std::printf("ok %ld\n", checks);
  return 0;
}

int check_stage(long lmax) {
  long checks = 0;
  uint64_t seed = 12345;
  const size_t na = sizeof(ALPHABET) - 1;
  for (long L = 1; L <= lmax; ++L) {
    std::vector<unsigned char> f((size_t)L), r((size_t)L);
    for (long i = 0; i < L; ++i) f[(size_t)i] = (unsigned char)ALPHABET[splitmix(seed) % na];
    for (long p = 0; p < L; ++p) r[(size_t)p] = rc_char(f[(size_t)(L - 1 - p)]);
    // tile starts: every start near the ends, a few in between (any w0 is a legal range begin)
    for (long t = 0; t < L; t += (t < 40 || t + 40 >= L) ? 1 : 17) {
      const int64_t base = rc_stage_base(t, L);
      const int64_t o0 = t - base;
      if (o0 < HALO || o0 > HALO + 15 || ((base - L) & 15) != 0) {
        std::printf("L %ld t %ld: base %lld\n", L, t, (long long)base);
        return 1;
      }
      for (int w = 0; w < 8; ++w) {       // the first words of the stage (the rest repeat them)
        const int64_t c0 = rc_word_fwd0(L, base, w);
        if (c0 & 15) {
          std::printf("L %ld t %ld w %d: forward block %lld not 16-aligned\n", L, t, w,
                      (long long)c0);
          return 1;
        }
        unsigned char fw[16], rw[16];     // chars outside [0, L) read as N on either strand
        for (int i = 0; i < 16; ++i) {
          const int64_t pf = c0 + i, pr = base + 16 * (int64_t)w + i;
          fw[i] = (pf >= 0 && pf < L) ? f[(size_t)pf] : (unsigned char)'N';
          rw[i] = (pr >= 0 && pr < L) ? r[(size_t)pr] : (unsigned char)'N';
        }
        uint32_t cf, nf, cr, nr;
        pack16(fw, cf, nf);
        pack16(rw, cr, nr);
        uint32_t keep = 0;
        for (int i = 0; i < 16; ++i)
          if (!((nr >> (15 - i)) & 1u)) keep |= 3u << (30 - 2 * i);
        if ((rc_code16(cf) & keep) != (cr & keep) || rc_nbit16(nf) != nr) {
          std::printf("L %ld t %ld w %d: stage word differs\n", L, t, w);
          return 1;
        }
        ++checks;
      }
    }
  }
  std::printf("ok %ld\n", checks);
  return 0;
}

}  // namespace

int main(int argc, char** argv) {
  if (argc == 4 && !std::strcmp(argv[1], "words"))
    return check_words(std::strtoull(argv[2], nullptr, 10), std::atol(argv[3]));
  if (argc == 3 && !std::strcmp(argv[1], "stage")) return check_stage(std::atol(argv[2]));
  std::fprintf(stderr, "usage: revcomp_check words SEED N | stage LMAX\n");
  return 2;
}
