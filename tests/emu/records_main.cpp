// TEST INFRASTRUCTURE: a stand-alone program that runs the record-summary kernels of crbm_amd/csrc/crbm_kernels.h
// (scan_encode_kernel, scan_records_body) on CPU threads, all blocks of a grid at once, and the host's part of
// crbm_scan_records_codes (crbm_layout.h: records_unit_exp; crbm_sweep.h: records_check, records_x_max, records_finish);
// tests/test_emu_records.py builds it with ASan + UBSan and runs it directly.
// usage: records_main <in> <out>  |  records_main unit <x_max> <S>   (the second form prints records_unit_exp's e)
//   <in>   int32 cfg, K, T, nrec, grid, threads, seg (window starts per segment, 0: one segment), want (bit 0 counts,
//          1 free energy, 2 best site); float32 W[K][4][M], b[K], c[4]; uint8 stream[T]; int64 rec_start[nrec + 1].
//          K is the model's number of motifs: a multiple case runs Cfg as the slab model of a larger model,
//          blockIdx.y = slab, the last slab moved back to end at K (crbm_kernels.h, slab_k0).
//   <out>  int32 e; uint64 GUARD, sums [nrec][K], GUARD, keys [nrec][K], GUARD, counts [nrec][5], GUARD; then what
//          records_finish makes of them: int64 windows [nrec], letters [nrec][4]; float32 fe [nrec], per_motif [nrec][K];
//          int32 start, strand [nrec][K]; float32 prob [nrec][K].
// The stream goes through in segments exactly as the driver sends it: segment [start, start + cnt) of the window starts
// with its halo of M - 1 letters, every buffer at exactly the size the driver gives it, the accumulators shared.
#define CRBM_DEFINE_MISC_KERNELS
#include "crbm_kernels.h"
#include "crbm_sweep.h"
#include "emu_launch.h"

#include <cstdio>
#include <cstdlib>
#include <cstring>

const bool emu::concurrent_blocks = true;

using namespace crbm;

static const unsigned long long GUARD_WORD = 0xA5A5A5A5DEADBEEFull;
static const int GUARD = 8;

#define REC_DISPATCH(id, ...)                                            \
  switch (id) {                                                          \
    case 0: { using C = Cfg<10, 15, 1, 3>; __VA_ARGS__; break; }         \
    case 1: { using C = Cfg<10, 5, 0, 2>; __VA_ARGS__; break; }          \
    case 2: { using C = Cfg<6, 1, 1, 1>; __VA_ARGS__; break; }           \
    case 3: { using C = Cfg<20, 15, 1, 2>; __VA_ARGS__; break; }         /* two groups of quads */ \
    case 4: { using C = Cfg<36, 6, 0, 2>; __VA_ARGS__; break; }          /* three */ \
    case 5: { using C = Cfg<5, 40, 1, 2>; __VA_ARGS__; break; }          /* a window of two 64-bit words */ \
    default: fprintf(stderr, "unknown configuration %d\n", id); return 2; \
  }

struct Out {
  int e = 0;
  std::vector<unsigned long long> acc;             // guards, sums, guards, keys, guards, counts, guards
  size_t off_sums = 0, off_keys = 0, off_counts = 0;
};

template <class C>
static int run(int K, long T, long nrec, int grid, int threads, long seg, int want, const float* W, const float* b, const float* c,
               const unsigned char* codes, const int64_t* rec_start, Out* out) {
  constexpr int M = C::M, S = C::DS ? 2 : 1;
  const int nslab = (K + C::K - 1) / C::K;
  SlabPlan plan;
  plan.Ks = C::K; plan.K = K; plan.last_k0 = K - C::K;
  if (K < C::K) { fprintf(stderr, "K below the configuration's\n"); return 2; }
  if (const char* bad = records_check(codes, T, rec_start, nrec)) { fprintf(stderr, "%s\n", bad); return 4; }
  std::vector<float> tables((size_t)nslab * C::TABLES_ALL);
  for (int y = 0; y < nslab; ++y) {
    const int k0 = (y + 1) * plan.Ks <= plan.K ? y * plan.Ks : plan.last_k0;
    emu::build_tables<C>(W + (size_t)k0 * 4 * M, b + k0, c, tables.data() + (size_t)y * C::TABLES_ALL);
  }
  out->e = records_unit_exp(records_x_max(W, b, K, M), S);
  const size_t cells = (size_t)nrec * K;
  out->off_sums = GUARD; out->off_keys = out->off_sums + cells + GUARD; out->off_counts = out->off_keys + cells + GUARD;
  out->acc.assign(out->off_counts + (size_t)nrec * 5 + GUARD, 0ull);
  for (size_t base : {(size_t)0, out->off_keys - GUARD, out->off_counts - GUARD, out->off_counts + (size_t)nrec * 5})
    for (int i = 0; i < GUARD; ++i) out->acc[base + i] = GUARD_WORD;
  if (T < M) {                                      // the driver counts the letters of such a stream on the host
    for (long r = 0; r < nrec; ++r)
      for (int64_t i = rec_start[r]; i < rec_start[r + 1] - 1; ++i)
        if (codes[i] < 4) ++out->acc[out->off_counts + 5 * (size_t)r + 1 + codes[i]];
    return 0;
  }
  const long starts_all = T - M + 1;
  if (seg <= 0 || seg > starts_all) seg = starts_all;
  std::vector<long long> rs((size_t)nrec + 1);      // the device copy, at its exact size
  for (long r = 0; r <= nrec; ++r) rs[(size_t)r] = rec_start[r];
  for (long start = 0; start < starts_all; start += seg) {
    const long cnt = std::min(seg, starts_all - start), n = cnt + M - 1;
    const ScanLayout l = scan_layout(n, cnt);
    std::vector<uint32_t> staged((size_t)(n + 3) / 4);
    std::memcpy(staged.data(), codes + start, (size_t)n);
    std::vector<uint32_t> letters((size_t)l.letter_words, 0xDEADBEEFu);
    std::vector<unsigned long long> valid((size_t)l.valid_words, ~0ull);
    uint32_t flags = 0;
    ScanEncodeArgs e{reinterpret_cast<const unsigned char*>(staged.data()), letters.data(), valid.data(), &flags, n, l.valid_words};
    emu::launch([&] { scan_encode_kernel(e); }, dim3(2), dim3(64), 0);
    if (flags) { fprintf(stderr, "a code above 4\n"); return 3; }
    ScanRecordsArgs a{ScanInput{tables.data(), letters.data(), valid.data(), (int)cnt, l.tiles, C::TABLES_ALL, plan}};
    a.rec_start = rs.data();
    a.sums = (want & 2) ? out->acc.data() + out->off_sums : nullptr;
    a.best = (want & 4) ? out->acc.data() + out->off_keys : nullptr;
    a.counts = (want & 1) ? out->acc.data() + out->off_counts : nullptr;
    a.pos0 = start; a.nrec = (int32_t)nrec;
    a.own = (int32_t)(start + cnt == starts_all ? n : cnt);
    a.scale = ldexpf(1.f, out->e); a.pad_ = 0;
    emu::launch([&] { scan_records_body<C>(a); }, dim3(grid, nslab), dim3(threads), (size_t)C::TAB * 4);
  }
  return 0;
}

int main(int argc, char** argv) {
  if (argc == 4 && !strcmp(argv[1], "unit")) {     // records_main unit x_max S -> e, and whether the bound holds
    const double x_max = atof(argv[2]);
    const int S = atoi(argv[3]), e = records_unit_exp(x_max, S);
    const double per = S * ((x_max > 0 ? x_max : 0) + 0.6931471805599453);
    printf("%d %d %d\n", e, ldexp(per, 31 + e) < ldexp(1.0, 62) ? 1 : 0, e == 32 || ldexp(per, 32 + e) >= ldexp(1.0, 62) ? 1 : 0);
    return 0;
  }
  if (argc != 3) { fprintf(stderr, "usage: %s <in> <out>\n", argv[0]); return 2; }
  FILE* f = fopen(argv[1], "rb");
  if (!f) { perror(argv[1]); return 2; }
  int32_t hd[8];
  if (fread(hd, 4, 8, f) != 8) { fprintf(stderr, "short header\n"); return 2; }
  const int id = hd[0], K = hd[1], grid = hd[4], threads = hd[5], want = hd[7];
  const long T = hd[2], nrec = hd[3], seg = hd[6];
  if (K < 1 || K > 4096 || T < 0 || T > (1 << 24) || nrec < 1 || nrec > (1 << 24) || grid < 1 || grid > 64 || threads < 64 ||
      threads > 1024 || threads % 64 != 0) { fprintf(stderr, "bad header\n"); return 2; }
  int M = 0, DS = 0;
  REC_DISPATCH(id, (M = C::M, DS = C::DS));
  std::vector<float> W((size_t)K * 4 * M), b((size_t)K), c(4);
  std::vector<unsigned char> codes((size_t)T + 1);
  std::vector<int64_t> rec_start((size_t)nrec + 1);
  if (fread(W.data(), 4, W.size(), f) != W.size() || fread(b.data(), 4, b.size(), f) != b.size() || fread(c.data(), 4, 4, f) != 4 ||
      fread(codes.data(), 1, (size_t)T, f) != (size_t)T || fread(rec_start.data(), 8, rec_start.size(), f) != rec_start.size()) {
    fprintf(stderr, "short input\n");
    return 2;
  }
  fclose(f);
  codes.resize((size_t)T);
  Out out;
  int rc = 0;
  REC_DISPATCH(id, (rc = run<C>(K, T, nrec, grid, threads, seg, want, W.data(), b.data(), c.data(), codes.data(), rec_start.data(), &out)));
  if (rc) return rc;
  const size_t cells = (size_t)nrec * K;
  std::vector<int64_t> windows((size_t)nrec), letters((size_t)nrec * 4);
  std::vector<float> fe((size_t)nrec), pm(cells), prob(cells);
  std::vector<int32_t> start(cells), strand(cells);
  records_finish(nrec, K, DS, out.e, c.data(), out.acc.data() + out.off_sums, out.acc.data() + out.off_keys,
                 out.acc.data() + out.off_counts, windows.data(), letters.data(), fe.data(), pm.data(), start.data(), strand.data(),
                 prob.data());
  FILE* g = fopen(argv[2], "wb");
  const int32_t e32 = out.e;
  bool ok = g && fwrite(&e32, 4, 1, g) == 1 && fwrite(out.acc.data(), 8, out.acc.size(), g) == out.acc.size() &&
            fwrite(windows.data(), 8, windows.size(), g) == windows.size() && fwrite(letters.data(), 8, letters.size(), g) == letters.size() &&
            fwrite(fe.data(), 4, fe.size(), g) == fe.size() && fwrite(pm.data(), 4, cells, g) == cells &&
            fwrite(start.data(), 4, cells, g) == cells && fwrite(strand.data(), 4, cells, g) == cells && fwrite(prob.data(), 4, cells, g) == cells;
  if (!ok) { perror(argv[2]); return 2; }
  fclose(g);
  return 0;
}
