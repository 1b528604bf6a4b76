// TEST INFRASTRUCTURE: a stand-alone program that runs the variant-effect kernels of crbm_amd/csrc/crbm_kernels.h
// (scan_encode_kernel, variant_effects_body, variant_combine_kernel) on CPU threads, all blocks of a grid at once, in
// the order of the driver (crbm_api.hip, variant_effects_any): contexts gathered by gather_contexts (crbm_sweep.h),
// encoded, scored, combined.  tests/test_emu_variants.py builds it with ASan + UBSan and runs it directly.
// usage: variants_main <in> <out>  |  variants_main plan <nvar> <M> <K> <budget> <budget_was_set>
// (the second form prints variant_plan's chunk, sets, bytes per variant, validity words and tiles)
//   <in>   int32 cfg, K, T, V, grid, threads; float32 W[K][4][M], b[K], c[4]; uint8 stream[T]; int64 pos[V]; uint8 alt[V].
//          K is the model's number of motifs: a multiple case runs Cfg as the slab model of a larger model,
//          blockIdx.y = slab, the last slab moved back to end at K (crbm_kernels.h, slab_k0).
//   <out>  32-bit words: GUARD, dfe [V], GUARD, per_motif [V][K], GUARD, windows [V], GUARD.
// Every buffer has exactly the size the driver gives it.
#define CRBM_DEFINE_MISC_KERNELS
#include "crbm_kernels.h"
#include "crbm_sweep.h"
#include "emu_launch.h"

#include <cstdio>
#include <cstdlib>
#include <cstring>

const bool emu::concurrent_blocks = true;

using namespace crbm;

static const uint32_t GUARD_WORD = 0xDEADBEEFu;
static const int GUARD = 8;

#define VAR_DISPATCH(id, ...)                                            \
  switch (id) {                                                          \
    case 0: { using C = Cfg<10, 15, 1, 3>; __VA_ARGS__; break; }         \
    case 1: { using C = Cfg<10, 5, 0, 2>; __VA_ARGS__; break; }          \
    case 2: { using C = Cfg<6, 1, 1, 1>; __VA_ARGS__; break; }           \
    case 3: { using C = Cfg<20, 15, 1, 2>; __VA_ARGS__; break; }         /* two groups of quads */ \
    case 4: { using C = Cfg<36, 6, 0, 2>; __VA_ARGS__; break; }          /* three */ \
    case 5: { using C = Cfg<5, 40, 1, 2>; __VA_ARGS__; break; }          /* a window of two 64-bit words */ \
    default: fprintf(stderr, "unknown configuration %d\n", id); return 2; \
  }

template <class C>
static int run(int K, long T, int V, int grid, int threads, const float* W, const float* b, const float* c,
               const unsigned char* codes, const int64_t* pos, const unsigned char* alt, std::vector<uint32_t>* out) {
  constexpr int M = C::M, CW = 2 * M - 1;
  const int nslab = (K + C::K - 1) / C::K;
  SlabPlan plan;
  plan.Ks = C::K; plan.K = K; plan.last_k0 = K - C::K;
  if (K < C::K) { fprintf(stderr, "K below the configuration's\n"); return 2; }
  std::vector<float> tables((size_t)nslab * C::TABLES_ALL);
  for (int y = 0; y < nslab; ++y) {
    const int k0 = (y + 1) * plan.Ks <= plan.K ? y * plan.Ks : plan.last_k0;
    emu::build_tables<C>(W + (size_t)k0 * 4 * C::M, b + k0, c, tables.data() + (size_t)y * C::TABLES_ALL);
  }
  const size_t o_dfe = GUARD, o_pm = o_dfe + V + GUARD, o_win = o_pm + (size_t)V * K + GUARD, total = o_win + V + GUARD;
  out->assign(total, GUARD_WORD);
  uint32_t* base = out->data();
  float* dfe = reinterpret_cast<float*>(base + o_dfe);
  float* pm = reinterpret_cast<float*>(base + o_pm);
  int32_t* windows = reinterpret_cast<int32_t*>(base + o_win);
  for (int i = 0; i < V; ++i)
    if (pos[i] < 0 || pos[i] >= T || alt[i] > 3) { fprintf(stderr, "a variant outside the stream, or no letter\n"); return 3; }
  if (V == 0) return 0;
  // the staging buffer of the driver: the contexts, rounded up to four bytes, then the alt bytes
  const size_t ctx_bytes = ((size_t)V * CW + 3) & ~(size_t)3;
  std::vector<uint32_t> staged((ctx_bytes + (size_t)V + 3) / 4);
  unsigned char* st = reinterpret_cast<unsigned char*>(staged.data());
  gather_contexts(codes, T, pos, V, M, st);
  std::memcpy(st + ctx_bytes, alt, (size_t)V);
  const long n = (long)V * CW;
  const ScanLayout l = scan_layout(n, V);
  std::vector<uint32_t> letters((size_t)l.letter_words, 0xDEADBEEFu);
  std::vector<unsigned long long> valid((size_t)l.valid_words, ~0ull);
  uint32_t flags = 0;
  ScanEncodeArgs e{st, letters.data(), valid.data(), &flags, n, l.valid_words};
  emu::launch([&] { scan_encode_kernel(e); }, dim3(2), dim3(64), 0);
  if (flags) { fprintf(stderr, "a code above 4\n"); return 3; }
  VariantArgs a{};
  a.tables = tables.data(); a.letters = letters.data(); a.valid = valid.data();
  a.starts = (int32_t)(n - M + 1); a.tiles = l.tiles; a.table_stride = C::TABLES_ALL; a.plan = plan;
  a.alt = st + ctx_bytes; a.per_motif = pm; a.windows = windows; a.cnt = V; a.pad_ = 0;
  emu::launch([&] { variant_effects_body<C>(a); }, dim3(grid, nslab), dim3(threads), (size_t)C::TAB * 4);
  VariantCombineArgs cb{pm, st, st + ctx_bytes, c, dfe, V, K, CW, M};
  emu::launch([&] { variant_combine_kernel(cb); }, dim3(2), dim3(64), 0);
  return 0;
}

int main(int argc, char** argv) {
  if (argc == 7 && !strcmp(argv[1], "plan")) {
    const VariantPlan p = variant_plan(atol(argv[2]), atoi(argv[3]), atoi(argv[4]), (size_t)atoll(argv[5]), atoi(argv[6]) != 0);
    printf("%d %d %zu %ld %d\n", p.chunk, p.nsets, p.per_variant, p.full.valid_words, p.full.tiles);
    return 0;
  }
  if (argc != 3) { fprintf(stderr, "usage: %s <in> <out>\n", argv[0]); return 2; }
  FILE* f = fopen(argv[1], "rb");
  if (!f) { perror(argv[1]); return 2; }
  int32_t hd[6];
  if (fread(hd, 4, 6, f) != 6) { fprintf(stderr, "short header\n"); return 2; }
  const int id = hd[0], K = hd[1], V = hd[3], grid = hd[4], threads = hd[5];
  const long T = hd[2];
  if (K < 1 || K > 4096 || T < 0 || T > (1 << 24) || V < 0 || V > (1 << 20) || grid < 1 || grid > 64 || threads < 64 ||
      threads > 1024 || threads % 64 != 0) { fprintf(stderr, "bad header\n"); return 2; }
  int M = 0;
  VAR_DISPATCH(id, (M = C::M));
  std::vector<float> W((size_t)K * 4 * M), b((size_t)K), c(4);
  std::vector<unsigned char> codes((size_t)T + 1), alt((size_t)V + 1);
  std::vector<int64_t> pos((size_t)V + 1);
  if (fread(W.data(), 4, W.size(), f) != W.size() || fread(b.data(), 4, b.size(), f) != b.size() || fread(c.data(), 4, 4, f) != 4 ||
      fread(codes.data(), 1, (size_t)T, f) != (size_t)T || fread(pos.data(), 8, (size_t)V, f) != (size_t)V ||
      fread(alt.data(), 1, (size_t)V, f) != (size_t)V) { fprintf(stderr, "short input\n"); return 2; }
  fclose(f);
  codes.resize((size_t)T); pos.resize((size_t)V); alt.resize((size_t)V);
  std::vector<uint32_t> out;
  int rc = 0;
  VAR_DISPATCH(id, (rc = run<C>(K, T, V, grid, threads, W.data(), b.data(), c.data(), codes.data(), pos.data(), alt.data(), &out)));
  if (rc) return rc;
  FILE* g = fopen(argv[2], "wb");
  if (!g || fwrite(out.data(), 4, out.size(), g) != out.size()) { perror(argv[2]); return 2; }
  fclose(g);
  return 0;
}
