// TEST INFRASTRUCTURE: a stand-alone program that runs the score-histogram kernels of crbm_amd/csrc/crbm_kernels.h
// (scan_encode_kernel, scan_hist_body) on CPU threads, all blocks of a grid at once; tests/test_emu_hist.py builds it
// with ASan + UBSan and runs it directly.  usage: hist_main <in> <out>  |  hist_main plan <tab_bytes> <NQ> <S> <nbins> <copies>
// (the second form prints hist_plan's gq, copies and LDS bytes)
//   <in>   int32 cfg, K, T, nbins, grid, threads, variant, gq (0: hist_plan's); float32 lo, hi; float32 W[K][4][M], b[K],
//          c[4]; uint8 stream[T].  K is the model's number of motifs: a multiple case runs Cfg as the slab model of a
//          larger model, blockIdx.y = slab, the last slab moved back to end at K (crbm_kernels.h, slab_k0).
//   <out>  uint64 GUARD words, counts [K][S][nbins], the valid windows, GUARD words.
// Every buffer has exactly the size the driver gives it, the LDS exactly hist_plan's bytes.
#define CRBM_DEFINE_MISC_KERNELS
#include "crbm_kernels.h"
#include "emu_launch.h"

#include <cstdio>
#include <cstdlib>
#include <cstring>

const bool emu::concurrent_blocks = true;

using namespace crbm;

static const unsigned long long GUARD_WORD = 0xA5A5A5A5DEADBEEFull;
static const int GUARD = 8;

#define HIST_DISPATCH(id, ...)                                           \
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
static int run(int K, long T, int nbins, int grid, int threads, int variant, int gq, float lo, float hi, const float* W,
               const float* b, const float* c, const unsigned char* codes, std::vector<unsigned long long>* out) {
  constexpr int S = C::DS ? 2 : 1;
  const int nslab = (K + C::K - 1) / C::K;
  SlabPlan plan;
  plan.Ks = C::K; plan.K = K; plan.last_k0 = K - C::K;
  if (K < C::K) { fprintf(stderr, "K below the configuration's\n"); return 2; }
  std::vector<float> tables((size_t)nslab * C::TABLES_ALL);
  for (int y = 0; y < nslab; ++y) {
    const int k0 = (y + 1) * plan.Ks <= plan.K ? y * plan.Ks : plan.last_k0;
    emu::build_tables<C>(W + (size_t)k0 * 4 * C::M, b + k0, c, tables.data() + (size_t)y * C::TABLES_ALL);
  }
  const size_t cells = (size_t)K * S * nbins;
  out->assign(cells + 1 + 2 * GUARD, 0ull);
  for (int i = 0; i < GUARD; ++i) (*out)[i] = (*out)[GUARD + cells + 1 + i] = GUARD_WORD;
  if (T < C::M) return 0;
  const long starts = T - C::M + 1;
  const ScanLayout l = scan_layout(T, starts);
  std::vector<uint32_t> staged((size_t)(T + 3) / 4);
  std::memcpy(staged.data(), codes, (size_t)T);
  std::vector<uint32_t> letters((size_t)l.letter_words, 0xDEADBEEFu);
  std::vector<unsigned long long> valid((size_t)l.valid_words, ~0ull);
  uint32_t flags = 0;
  ScanEncodeArgs e{reinterpret_cast<const unsigned char*>(staged.data()), letters.data(), valid.data(), &flags, T, l.valid_words};
  emu::launch([&] { scan_encode_kernel(e); }, dim3(2), dim3(64), 0);
  if (flags) { fprintf(stderr, "a code above 4\n"); return 3; }
  HistPlan hp = hist_plan(C::TAB * 4, C::NQ, S, nbins, variant == 2 ? threads / 64 : 1);
  if (gq > 0) {                                     // a forced group size, one counter set
    hp.gq = gq; hp.copies = 1;
    hp.lds = (long)C::TAB * 4 + 16L * S * nbins * gq + 4;
  }
  if (hp.gq < 1 || hp.lds > 160L * 1024) { fprintf(stderr, "no room for the counters\n"); return 2; }
  ScanHistArgs a{ScanInput{tables.data(), letters.data(), valid.data(), (int)starts, l.tiles, C::TABLES_ALL, plan}};
  a.hist = out->data() + GUARD;
  a.nbins = nbins; a.gq = hp.gq; a.copies = hp.copies; a.rotate = variant == 1;
  a.lo = lo; a.inv_w = (float)nbins / (hi - lo);
  emu::launch([&] { scan_hist_body<C>(a); }, dim3(grid, nslab), dim3(threads), (size_t)hp.lds);
  return 0;
}

int main(int argc, char** argv) {
  if (argc == 7 && !strcmp(argv[1], "plan")) {     // hist_main plan tab_bytes NQ S nbins want_copies -> gq copies lds
    const HistPlan p = hist_plan(atoi(argv[2]), atoi(argv[3]), atoi(argv[4]), atoi(argv[5]), atoi(argv[6]));
    printf("%d %d %ld\n", p.gq, p.copies, p.lds);
    return 0;
  }
  if (argc != 3) { fprintf(stderr, "usage: %s <in> <out>\n", argv[0]); return 2; }
  FILE* f = fopen(argv[1], "rb");
  if (!f) { perror(argv[1]); return 2; }
  int32_t hd[8];
  float range[2];
  if (fread(hd, 4, 8, f) != 8 || fread(range, 4, 2, f) != 2) { fprintf(stderr, "short header\n"); return 2; }
  const int id = hd[0], K = hd[1], nbins = hd[3], grid = hd[4], threads = hd[5], variant = hd[6], gq = hd[7];
  const long T = hd[2];
  if (K < 1 || K > 4096 || T < 0 || T > (1 << 24) || nbins < 1 || nbins > 1024 || grid < 1 || grid > 64 || threads < 64 ||
      threads > 1024 || threads % 64 != 0) { fprintf(stderr, "bad header\n"); return 2; }
  int M = 0;
  HIST_DISPATCH(id, (M = C::M));
  std::vector<float> W((size_t)K * 4 * M), b((size_t)K), c(4);
  std::vector<unsigned char> codes((size_t)T + 1);
  if (fread(W.data(), 4, W.size(), f) != W.size() || fread(b.data(), 4, b.size(), f) != b.size() || fread(c.data(), 4, 4, f) != 4 ||
      fread(codes.data(), 1, (size_t)T, f) != (size_t)T) { fprintf(stderr, "short input\n"); return 2; }
  fclose(f);
  codes.resize((size_t)T);
  std::vector<unsigned long long> out;
  int rc = 0;
  HIST_DISPATCH(id, (rc = run<C>(K, T, nbins, grid, threads, variant, gq, range[0], range[1], W.data(), b.data(), c.data(), codes.data(), &out)));
  if (rc) return rc;
  FILE* g = fopen(argv[2], "wb");
  if (!g || fwrite(out.data(), 8, out.size(), g) != out.size()) { perror(argv[2]); return 2; }
  fclose(g);
  return 0;
}
