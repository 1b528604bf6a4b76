// TEST INFRASTRUCTURE: a stand-alone program that checks the visible-letter sampler of crbm_amd/csrc/crbm_kernels.h
// (push_letter, sample_letter, letter_byte: the letter from the signs of t - threshold, two bits shifted into the byte per
// position) and the 32-bit packing of the mask window (pack_masks) against the expressions they replaced, which are
// written out below: three comparisons added up, a select per position, 64-bit shifts.  Not one disagreement is
// tolerated.  tests/test_emu_letter_sampler.py builds it with ASan + UBSan and runs it directly.
// usage: letter_main      prints "LETTER OK cases=<n> ties=<n>"
#include "crbm_kernels.h"

#include <cstdio>
#include <cstdlib>

using namespace crbm;

namespace {
struct Lcg {
  uint64_t s;
  uint32_t next() { s = s * 6364136223846793005ull + 1442695040888963407ull; return (uint32_t)(s >> 32); }
  float uniform() { return (float)(next() >> 8) * (1.0f / 16777216.0f); }
  float normalish() { return (uniform() + uniform() + uniform() + uniform() - 2.0f) * 1.7320508f; }   // variance 1
};

// the sampler as it stood: the letter is the number of thresholds t has reached
uint32_t old_letter(float y0, float y1, float y2, float y3, float u, int* tie = nullptr) {
  const float mx = fmaxf(fmaxf(y0, y1), fmaxf(y2, y3));
  const float e0 = __builtin_amdgcn_exp2f(y0 - mx), e1 = __builtin_amdgcn_exp2f(y1 - mx), e2 = __builtin_amdgcn_exp2f(y2 - mx),
              e3 = __builtin_amdgcn_exp2f(y3 - mx);
  const float t = u * ((e0 + e1) + (e2 + e3));
  if (tie) *tie = (t == e0) + (t == e0 + e1) + (t == (e0 + e1) + e2);
  return (uint32_t)(t >= e0) + (uint32_t)(t >= e0 + e1) + (uint32_t)(t >= (e0 + e1) + e2);
}
uint32_t old_byte(const float (&y)[4][4], const float (&u)[4], int p0, int Lv) {
  uint32_t byte = 0u;
  for (int i = 0; i < 4; ++i) byte |= (p0 + i < Lv ? old_letter(y[i][0], y[i][1], y[i][2], y[i][3], u[i]) : 0u) << (2 * i);
  return byte;
}
uint32_t new_inv(const float (&y)[4][4], const float (&u)[4]) {
  uint32_t inv = 0u;
  for (int i = 3; i >= 0; --i) inv = push_letter(inv, y[i][0], y[i][1], y[i][2], y[i][3], u[i]);
  return inv;
}

unsigned long long cases = 0, ties = 0;
int failures = 0;

void check_letter(float y0, float y1, float y2, float y3, float u) {
  int tie = 0;
  const uint32_t want = old_letter(y0, y1, y2, y3, u, &tie), got = sample_letter(y0, y1, y2, y3, u);
  ++cases;
  ties += (unsigned)tie;
  if (want != got && failures++ < 20)
    fprintf(stderr, "letter differs: y = (%a, %a, %a, %a), u = %a: %u, was %u\n", y0, y1, y2, y3, u, got, want);
}

// every byte of a row of Lv positions (all four remainders of Lv come through the callers)
void check_row(const float (&y)[4][4], const float (&u)[4], int Lv) {
  const uint32_t inv = new_inv(y, u);
  for (int p0 = 0; p0 < Lv; p0 += 4) {
    const uint32_t want = old_byte(y, u, p0, Lv), got = letter_byte<false>(inv, p0, Lv);
    ++cases;
    if (want != got && failures++ < 20) fprintf(stderr, "byte differs at p0 = %d of Lv = %d: %02x, was %02x\n", p0, Lv, got, want);
    if (Lv % 4 == 0 && letter_byte<true>(inv, p0, Lv) != want && failures++ < 20)
      fprintf(stderr, "whole byte differs at p0 = %d of Lv = %d\n", p0, Lv);
  }
}

template <int K>
void check_pack(Lcg& rng) {
  constexpr int PPW = 64 / K;
  for (int rep = 0; rep < 2000; ++rep) {
    uint32_t m[PPW];
    for (int t = 0; t < PPW; ++t) {
      const uint32_t r = rng.next(), full = K == 32 ? 0xFFFFFFFFu : (1u << K) - 1u;
      m[t] = rep % 3 == 0 ? full : (rep % 3 == 1 ? r & full : r & rng.next() & rng.next() & full);
    }
    for (int n = 0; n <= PPW + 1; ++n) {      // n > PPW: more masks wanted than a word holds
      unsigned long long want = 0ull;
      for (int t = 0; t < PPW; ++t)
        if (t < n) want |= (unsigned long long)m[t] << (t * K);
      uint32_t lo = 0u, hi = 0u;
      pack_masks<K, 0, PPW>(m, n, lo, hi);
      ++cases;
      if (((unsigned long long)lo | ((unsigned long long)hi << 32)) != want && failures++ < 20)
        fprintf(stderr, "window word differs: K = %d, %d masks: %08x%08x, was %016llx\n", K, n, hi, lo, want);
    }
  }
}
}  // namespace

int main() {
  Lcg rng{0x5EEDull};
  const float U_MAX = 1.0f - 1.0f / 16777216.0f, ULP = 1.0f / 16777216.0f;
  // 2^22 random (y0..y3, u): activations of every scale the tables can give, u on the 24-bit grid of u01
  const float scales[6] = {0.05f, 1.0f, 4.0f, 30.0f, 120.0f, 400.0f};
  for (int i = 0; i < (1 << 22); ++i) {
    const float s = scales[rng.next() % 6u], off = 50.0f * rng.normalish();
    check_letter(off + s * rng.normalish(), off + s * rng.normalish(), off + s * rng.normalish(), off + s * rng.normalish(), rng.uniform());
  }
  // equal activations: all four, every pair; differences beyond 150 (e = 0); both ends of u
  const float us[7] = {0.0f, ULP, 0.25f, 0.5f, 0.75f, U_MAX - ULP, U_MAX};
  const float lv[6] = {0.0f, -1.0f, 3.5f, -151.0f, -200.0f, 170.0f};
  for (float a : lv) for (float b : lv) for (float c : lv) for (float d : lv) for (float u : us) check_letter(a, b, c, d, u);
  for (int i = 0; i < 200000; ++i) {
    float y[4];
    for (float& v : y) v = 3.0f * rng.normalish();
    const unsigned a = rng.next() % 4u, b = rng.next() % 4u;
    y[a] = y[b];                                                        // a pair of equal activations
    if (i % 3 == 0) y[rng.next() % 4u] -= 150.0f + 100.0f * rng.uniform();   // one letter out of reach
    if (i % 7 == 0) y[0] = y[1] = y[2] = y[3];
    const float u = i % 5 == 0 ? 0.0f : (i % 5 == 1 ? U_MAX : rng.uniform());
    check_letter(y[0], y[1], y[2], y[3], u);
  }
  // constructed ties t == threshold: activations that differ by whole numbers make every e a power of two; where their
  // sum is one as well, u = threshold / sum is on the grid and t meets the threshold exactly.  One step of u to
  // either side as well.
  const unsigned long long ties_before = ties;
  {
    const float sets[6][4] = {{0, 0, 0, 0}, {-2, -2, -1, 0}, {0, -1, -1, -300}, {-1, -1, 0, -300}, {-300, 0, -300, -300}, {-3, -3, -2, -1}};
    for (const auto& y : sets)
      for (int p = 0; p < 24; ++p) {       // every permutation keeps the sum a power of two
        int idx[4] = {0, 1, 2, 3}, k = p;
        for (int i = 0; i < 3; ++i) { const int j = i + k % (4 - i); k /= (4 - i); const int t = idx[i]; idx[i] = idx[j]; idx[j] = t; }
        for (float shift : {0.0f, 7.0f, -40.0f})
          for (int q = 0; q <= 64; ++q)
            for (int d = -1; d <= 1; ++d) {
              const float u = (float)q / 64.0f + (float)d * ULP;
              if (u < 0.0f || u > U_MAX) continue;
              check_letter(y[idx[0]] + shift, y[idx[1]] + shift, y[idx[2]] + shift, y[idx[3]] + shift, u);
            }
      }
  }
  const unsigned long long made_ties = ties - ties_before;
  if (made_ties < 100) { fprintf(stderr, "the constructed ties did not tie (%llu)\n", made_ties); return 1; }
  // the byte of four positions, for every remainder of Lv % 4 in the last byte
  for (int i = 0; i < 20000; ++i) {
    float y[4][4], u[4];
    for (auto& row : y) for (float& v : row) v = 4.0f * rng.normalish();
    for (float& v : u) v = rng.uniform();
    for (int Lv = 17; Lv <= 24; ++Lv) check_row(y, u, Lv);
  }
  // the mask window: every width that packs several masks into a word (K <= 32), straddling bit 32 or not
  check_pack<2>(rng); check_pack<3>(rng); check_pack<7>(rng); check_pack<9>(rng); check_pack<10>(rng); check_pack<11>(rng);
  check_pack<12>(rng); check_pack<16>(rng); check_pack<20>(rng); check_pack<21>(rng); check_pack<22>(rng); check_pack<31>(rng);
  check_pack<32>(rng);
  if (failures) { fprintf(stderr, "%d disagreements\n", failures); return 1; }
  printf("LETTER OK cases=%llu ties=%llu\n", cases, ties);
  return 0;
}
