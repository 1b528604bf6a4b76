// TEST INFRASTRUCTURE: a stand-alone program that runs the allele-effect kernels of crbm_amd/csrc/crbm_kernels.h
// (scan_encode_kernel, allele_effects_body, allele_combine_kernel) on CPU threads, all blocks of a grid at once, in the
// order of the driver (crbm_api.hip, allele_effects_any): haplotypes gathered by gather_haplotypes (crbm_sweep.h),
// encoded, scored, combined.  tests/test_emu_alleles.py builds it with ASan + UBSan and runs it directly.
// usage: alleles_main <in> <out>  |  alleles_main plan <M> <K> <budget> <budget_was_set> <lengths>
// (the second form reads int32 nvar, R[nvar], A[nvar] from <lengths> and prints allele_plan's sets, longest chunk, most
//  staged codes and validity words, then the cuts)
//   <in>   int32 cfg, K, T, V, grid, threads; float32 W[K][4][M], b[K], c[4]; uint8 stream[T]; int64 pos[V];
//          int32 ref_len[V]; int64 alt_off[V + 1]; uint8 alt_codes[alt_off[V]].
//          K is the model's number of motifs: a multiple case runs Cfg as the slab model of a larger model,
//          blockIdx.y = slab, the last slab moved back to end at K (crbm_kernels.h, slab_k0).
//   <out>  32-bit words: GUARD, dfe [V], GUARD, per_motif [V][K], GUARD, windows [V][2], GUARD.
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

#define ALLELE_DISPATCH(id, ...)                                         \
  switch (id) {                                                          \
    case 0: { using C = Cfg<10, 15, 1, 3>; __VA_ARGS__; break; }         \
    case 1: { using C = Cfg<10, 5, 0, 2>; __VA_ARGS__; break; }          \
    case 2: { using C = Cfg<6, 1, 1, 1>; __VA_ARGS__; break; }           /* M = 1: an insertion has no ref windows */ \
    case 3: { using C = Cfg<20, 15, 1, 2>; __VA_ARGS__; break; }         /* two groups of quads */ \
    case 4: { using C = Cfg<36, 6, 0, 2>; __VA_ARGS__; break; }          /* three */ \
    case 5: { using C = Cfg<5, 40, 1, 2>; __VA_ARGS__; break; }          /* a window of two 64-bit words */ \
    default: fprintf(stderr, "unknown configuration %d\n", id); return 2; \
  }

template <class C>
static int run(int K, long T, int V, int grid, int threads, const float* W, const float* b, const float* c,
               const unsigned char* codes, const int64_t* pos, const int32_t* ref_len, const int64_t* alt_off,
               const unsigned char* alt_codes, std::vector<uint32_t>* out) {
  constexpr int M = C::M;
  const int nslab = (K + C::K - 1) / C::K;
  SlabPlan plan;
  plan.Ks = C::K; plan.K = K; plan.last_k0 = K - C::K;
  if (K < C::K) { fprintf(stderr, "K below the configuration's\n"); return 2; }
  std::vector<float> tables((size_t)nslab * C::TABLES_ALL);
  for (int y = 0; y < nslab; ++y) {
    const int k0 = (y + 1) * plan.Ks <= plan.K ? y * plan.Ks : plan.last_k0;
    emu::build_tables<C>(W + (size_t)k0 * 4 * C::M, b + k0, c, tables.data() + (size_t)y * C::TABLES_ALL);
  }
  const size_t o_dfe = GUARD, o_pm = o_dfe + V + GUARD, o_win = o_pm + (size_t)V * K + GUARD, total = o_win + 2 * (size_t)V + GUARD;
  out->assign(total, GUARD_WORD);
  uint32_t* base = out->data();
  float* dfe = reinterpret_cast<float*>(base + o_dfe);
  float* pm = reinterpret_cast<float*>(base + o_pm);
  int32_t* windows = reinterpret_cast<int32_t*>(base + o_win);
  long n = 0;
  for (int i = 0; i < V; ++i) {
    const int64_t A = alt_off[i + 1] - alt_off[i];
    if (pos[i] < 0 || ref_len[i] < 0 || ref_len[i] > 65535 || A < 0 || A > 65535 || pos[i] + ref_len[i] > T) {
      fprintf(stderr, "a variant outside the stream, or a bad length\n");
      return 3;
    }
    n += allele_codes(ref_len[i], A, M);
  }
  for (int64_t i = 0; i < alt_off[V]; ++i)
    if (alt_codes[i] > 3) { fprintf(stderr, "an alt code that is no letter\n"); return 3; }
  if (V == 0) return 0;
  // the staging buffer of the driver: the haplotypes, rounded up to sixteen bytes, then the table
  const size_t code_bytes = ((size_t)n + 15) & ~(size_t)15;
  std::vector<uint32_t> staged((code_bytes + (size_t)V * sizeof(AlleleEntry)) / 4);
  unsigned char* st = reinterpret_cast<unsigned char*>(staged.data());
  AlleleEntry* table = reinterpret_cast<AlleleEntry*>(st + code_bytes);
  if (gather_haplotypes(codes, T, pos, ref_len, alt_off, alt_codes, V, M, st, table) != n) { fprintf(stderr, "gather_haplotypes: another length\n"); return 3; }
  const ScanLayout l = scan_layout(n, n);
  std::vector<uint32_t> letters((size_t)l.letter_words, 0xDEADBEEFu);
  std::vector<unsigned long long> valid((size_t)l.valid_words, ~0ull);
  uint32_t flags = 0;
  ScanEncodeArgs e{st, letters.data(), valid.data(), &flags, n, l.valid_words};
  emu::launch([&] { scan_encode_kernel(e); }, dim3(2), dim3(64), 0);
  if (flags) { fprintf(stderr, "a code above 4\n"); return 3; }
  AlleleArgs a{};
  a.tables = tables.data(); a.letters = letters.data(); a.valid = valid.data();
  a.starts = (int32_t)n; a.tiles = l.tiles; a.table_stride = C::TABLES_ALL; a.plan = plan;
  a.table = table; a.per_motif = pm; a.windows = windows; a.cnt = V; a.pad_ = 0;
  emu::launch([&] { allele_effects_body<C>(a); }, dim3(grid, nslab), dim3(threads), (size_t)C::TAB * 4);
  AlleleCombineArgs cb{pm, st, table, c, dfe, V, K, M, 0};
  emu::launch([&] { allele_combine_kernel(cb); }, dim3(2), dim3(64), 0);
  return 0;
}

static int plan_main(char** argv) {
  FILE* f = fopen(argv[6], "rb");
  if (!f) { perror(argv[6]); return 2; }
  int32_t nvar = 0;
  if (fread(&nvar, 4, 1, f) != 1 || nvar < 0 || nvar > (1 << 24)) { fprintf(stderr, "bad lengths file\n"); return 2; }
  std::vector<int32_t> R((size_t)nvar + 1), A((size_t)nvar + 1);
  if (fread(R.data(), 4, (size_t)nvar, f) != (size_t)nvar || fread(A.data(), 4, (size_t)nvar, f) != (size_t)nvar) { fprintf(stderr, "short lengths file\n"); return 2; }
  fclose(f);
  std::vector<int64_t> off((size_t)nvar + 1, 0);
  for (int i = 0; i < nvar; ++i) off[i + 1] = off[i] + A[i];
  const AllelePlan p = allele_plan(nvar, R.data(), off.data(), atoi(argv[2]), atoi(argv[3]), (size_t)atoll(argv[4]), atoi(argv[5]) != 0);
  printf("%d %d %ld %ld", p.nsets, p.max_cnt, p.max_codes, p.full.valid_words);
  for (int64_t c : p.cuts) printf(" %lld", (long long)c);
  printf("\n");
  return 0;
}

int main(int argc, char** argv) {
  if (argc == 7 && !strcmp(argv[1], "plan")) return plan_main(argv);
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
  ALLELE_DISPATCH(id, (M = C::M));
  std::vector<float> W((size_t)K * 4 * M), b((size_t)K), c(4);
  std::vector<unsigned char> codes((size_t)T + 1);
  std::vector<int64_t> pos((size_t)V + 1), alt_off((size_t)V + 1);
  std::vector<int32_t> ref_len((size_t)V + 1);
  if (fread(W.data(), 4, W.size(), f) != W.size() || fread(b.data(), 4, b.size(), f) != b.size() || fread(c.data(), 4, 4, f) != 4 ||
      fread(codes.data(), 1, (size_t)T, f) != (size_t)T || fread(pos.data(), 8, (size_t)V, f) != (size_t)V ||
      fread(ref_len.data(), 4, (size_t)V, f) != (size_t)V || fread(alt_off.data(), 8, (size_t)V + 1, f) != (size_t)V + 1) {
    fprintf(stderr, "short input\n");
    return 2;
  }
  if (alt_off[0] != 0 || alt_off[V] < 0 || alt_off[V] > (1 << 26)) { fprintf(stderr, "bad alt offsets\n"); return 2; }
  std::vector<unsigned char> alt_codes((size_t)alt_off[V] + 1);
  if (fread(alt_codes.data(), 1, (size_t)alt_off[V], f) != (size_t)alt_off[V]) { fprintf(stderr, "short input\n"); return 2; }
  fclose(f);
  codes.resize((size_t)T); pos.resize((size_t)V); ref_len.resize((size_t)V); alt_codes.resize((size_t)alt_off[V]);
  std::vector<uint32_t> out;
  int rc = 0;
  ALLELE_DISPATCH(id, (rc = run<C>(K, T, V, grid, threads, W.data(), b.data(), c.data(), codes.data(), pos.data(), ref_len.data(),
                                   alt_off.data(), alt_codes.data(), &out)));
  if (rc) return rc;
  FILE* g = fopen(argv[2], "wb");
  if (!g || fwrite(out.data(), 4, out.size(), g) != out.size()) { perror(argv[2]); return 2; }
  fclose(g);
  return 0;
}
