// TEST INFRASTRUCTURE: a stand-alone program that runs the chain kernel body of crbm_amd/csrc/crbm_kernels.h
// (gibbs_body, set-bit walk) on CPU threads in both geometry forms -- GeomRT, the geometry in the arguments, and GeomCT,
// the geometry compiled in -- from the same state and seeds, and compares the hidden masks of both strands and the
// letters of the last visible sample word for word.  Which form a case takes is decided as the library decides it
// (crbm_plan.h, geo_spec): a case whose launch has a ragged last tile must come out in the run-time form.
// tests/test_emu_geom.py builds it with ASan + UBSan and runs it directly.
// usage: geom_main <case> <steps>      prints "GEOM OK <case> <steps> form=<ct|rt> set=<bits>"
#include "crbm_kernels.h"
#include "crbm_plan.h"
#include "emu_launch.h"

#include <cstdio>
#include <cstdlib>
#include <cstring>

// block after block: the results are compared bit for bit
const bool emu::concurrent_blocks = false;

using namespace crbm;

namespace {
struct Lcg {
  uint64_t s;
  uint32_t next() { s = s * 6364136223846793005ull + 1442695040888963407ull; return (uint32_t)(s >> 33); }
  float uniform() { return (float)(next() & 0xFFFFFF) * (1.0f / 16777216.0f); }
  float normalish() { return (uniform() + uniform() + uniform() + uniform() - 2.0f) * 1.7320508f; }   // variance 1
};

struct Outputs {
  std::vector<uint32_t> hm, hmp, vout, ones;
};

// One launch of `steps` steps in geometry policy GP.  Every buffer has exactly the size the library gives it.
template <class C, class GP>
Outputs run(const std::vector<float>& tables, const std::vector<uint32_t>& hm0, const std::vector<uint32_t>& hmp0, int nchains, int Lf,
            int S, int threads, int grid, int steps) {
  const ModelShape ms = model_shape(C::K, C::M, C::DS, C::G, C::POOL);
  const GibbsLayout gl = gibbs_layout(ms, Lf, S, true);
  Outputs o;
  o.hm = hm0; o.hmp = hmp0;
  o.vout.assign((size_t)nchains * gl.LWs, 0xDEADBEEFu);
  o.ones.assign((size_t)grid * (threads / 64), 0xDEADBEEFu);
  GibbsArgs a;
  a.tables = tables.data();
  a.hm = o.hm.data(); a.hmp = C::DS ? o.hmp.data() : nullptr; a.vout = o.vout.data(); a.ones = o.ones.data();
  a.nchains = nchains; a.Lf = Lf; a.Lv = gl.Lv; a.S = S; a.nvb = gl.nvb; a.nhb = gl.nhb; a.Lrow = gl.Lrow; a.LWs = gl.LWs;
  a.divVB = make_fastdiv((uint32_t)gl.nvb); a.divHB = make_fastdiv((uint32_t)gl.nhb);
  a.divRow = make_fastdiv((uint32_t)(gl.Lrow * ms.NW)); a.divLfw = make_fastdiv((uint32_t)(Lf * ms.NW));
  a.steps = steps;
  a.rng.seed_lo = 0x2026u; a.rng.seed_hi = 0x17u; a.rng.step = 5u; a.rng.seq_offset = 3u;
  a.debug = 0; a.nblocks = grid; a.stats_off = 0;
  emu::launch([&] { gibbs_body<C, true, false, GP>(a); }, dim3(grid), dim3(threads), (size_t)gl.lds_bytes);
  return o;
}

template <class C, int S, int LF, int TB, int NCHAINS, int GRID, bool WANT_CT>
int run_case(const char* name, int steps) {
  constexpr int M = C::M, NW = C::NW;
  const ModelShape ms = model_shape(C::K, C::M, C::DS, C::G, C::POOL);
  constexpr int LV = LF + M - 1, NVB = cdiv(LV, 4), LROW = 4 * cdiv(4 * NVB + M - 1 + 3, 4), LWS = (4 * NVB + 15) / 16 + 2;
  const GibbsLayout gl = gibbs_layout(ms, LF, S, true);
  if (gl.Lv != LV || gl.nvb != NVB || gl.nhb != LF || gl.Lrow != LROW || gl.LWs != LWS) { fprintf(stderr, "layout constants differ from gibbs_layout\n"); return 3; }
  // the model: N(0, 0.7^2) weights, hidden biases around -1.5 (a few per cent of the units set), visible biases of their own
  Lcg rng{0x9E3779B97F4A7C15ull + (uint64_t)C::K * 131 + M};
  std::vector<float> W((size_t)C::K * 4 * M), b((size_t)C::K), c(4);
  for (auto& w : W) w = 0.7f * rng.normalish();
  for (auto& x : b) x = -1.5f + 0.5f * rng.normalish();
  for (auto& x : c) x = 0.3f * rng.normalish();
  std::vector<float> tables((size_t)C::TABLES_ALL);
  emu::build_tables<C>(W.data(), b.data(), c.data(), tables.data());
  const size_t words = (size_t)NCHAINS * LF * NW;
  std::vector<uint32_t> hm0(words), hmp0(C::DS ? words : 0);
  auto fill = [&](std::vector<uint32_t>& m) {
    for (size_t i = 0; i < m.size(); ++i) {
      const int w = (int)(i % NW), nbits = std::min(32, C::K - 32 * w);
      uint32_t x = 0u;
      for (int k = 0; k < nbits; ++k) x |= (rng.uniform() < 0.06f ? 1u : 0u) << k;
      m[i] = x;
    }
  };
  fill(hm0);
  fill(hmp0);
  // the form the library would launch this shape in
  const GeoSpec spec = geo_spec(gl, TB, GRID, NCHAINS, NW, C::G);
  if (spec.on() != WANT_CT) { fprintf(stderr, "%s: geo_spec %s, expected the %s form\n", name, spec.on() ? "on" : "off", WANT_CT ? "compile-time" : "run-time"); return 4; }
  const Outputs rt = run<C, GeomRT>(tables, hm0, hmp0, NCHAINS, LF, S, TB, GRID, steps);
  Outputs other;
  if constexpr (WANT_CT) {
    constexpr bool ALIGNED = ((long)S * LF * NW) % 4 == 0;
    if (spec.aligned != ALIGNED || !spec.serves(gl, TB, GRID, NCHAINS)) { fprintf(stderr, "%s: geo_spec differs from the compiled constants\n", name); return 4; }
    using GP = GeomCT<S, LF, LV, LROW, LWS, NVB, LF, TB, NCHAINS, GRID, ALIGNED>;
    other = run<C, GP>(tables, hm0, hmp0, NCHAINS, LF, S, TB, GRID, steps);
  } else {
    other = run<C, GeomRT>(tables, hm0, hmp0, NCHAINS, LF, S, TB, GRID, steps);
  }
  auto same = [&](const std::vector<uint32_t>& x, const std::vector<uint32_t>& y, const char* what) {
    if (x.size() != y.size()) { fprintf(stderr, "%s: %s sizes differ\n", name, what); return false; }
    for (size_t i = 0; i < x.size(); ++i)
      if (x[i] != y[i]) { fprintf(stderr, "%s: %s differs at word %zu: %08x vs %08x\n", name, what, i, x[i], y[i]); return false; }
    return true;
  };
  if (!same(rt.hm, other.hm, "hm") || !same(rt.hmp, other.hmp, "hmp") || !same(rt.vout, other.vout, "letters") || !same(rt.ones, other.ones, "activity")) return 1;
  // the launch did something: the state moved, every activity slot was written, and the masks stay within K bits
  unsigned long long set = 0, moved = 0;
  for (size_t i = 0; i < rt.hm.size(); ++i) {
    set += (unsigned)__builtin_popcount(rt.hm[i]);
    moved += rt.hm[i] != hm0[i];
    const int nbits = std::min(32, C::K - 32 * (int)(i % NW));
    if (nbits < 32 && (rt.hm[i] >> nbits)) { fprintf(stderr, "%s: a bit beyond K\n", name); return 1; }
  }
  for (uint32_t x : rt.ones) if (x == 0xDEADBEEFu) { fprintf(stderr, "%s: an activity slot was not written\n", name); return 1; }
  for (uint32_t x : rt.vout) if (x == 0xDEADBEEFu) { fprintf(stderr, "%s: a letter word was not written\n", name); return 1; }
  if (!moved || !set) { fprintf(stderr, "%s: the chains did not move\n", name); return 1; }
  printf("GEOM OK %s %d form=%s set=%llu\n", name, steps, WANT_CT ? "ct" : "rt", set);
  return 0;
}
}  // namespace

int main(int argc, char** argv) {
  if (argc != 3) { fprintf(stderr, "usage: %s <case> <steps>\n", argv[0]); return 2; }
  const char* w = argv[1];
  const int steps = atoi(argv[2]);
  if (steps < 1 || steps > 8) { fprintf(stderr, "steps out of range\n"); return 2; }
  //                                                      model              S  Lf   TB  chains grid  compiled-in
  if (!strcmp(w, "ss_186_aligned")) return run_case<Cfg<10, 15, 0, 3>, 4, 186, 256, 8, 2, true>(w, steps);    // one tile per block
  if (!strcmp(w, "ss_185")) return run_case<Cfg<10, 15, 0, 3>, 4, 185, 256, 8, 2, true>(w, steps);
  if (!strcmp(w, "ss_185_word_path")) return run_case<Cfg<10, 15, 0, 3>, 2, 185, 128, 6, 3, true>(w, steps);  // 370 words per tile: 4-byte loads
  if (!strcmp(w, "ds_50")) return run_case<Cfg<10, 15, 1, 3>, 2, 50, 128, 6, 2, true>(w, steps);              // three tiles on two blocks: the tile loop
  if (!strcmp(w, "two_mask_words")) return run_case<Cfg<40, 6, 0, 2>, 4, 30, 128, 4, 1, true>(w, steps);
  // (the check of this case is that geo_spec refuses the shape; both of its runs are then GeomRT, so its word comparison
  //  is vacuous by construction -- on the GPU, tests/test_gpu_geometry.py reads the launch counter for the same shape)
  if (!strcmp(w, "ragged_falls_back")) return run_case<Cfg<10, 15, 0, 3>, 4, 186, 256, 9, 3, false>(w, steps);
  fprintf(stderr, "unknown case %s\n", w);
  return 2;
}
