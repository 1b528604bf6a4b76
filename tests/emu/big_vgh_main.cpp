// TEST INFRASTRUCTURE: a stand-alone program that runs the chain v|h kernels of the generic path (crbm_kernels_generic.h:
// big_vgh_kernel for DNA, big_vgh_any_kernel for any other alphabet) on CPU threads with 64-thread blocks -- chunks of
// 512 and 64 visible positions -- so that the chunk loop (c0 > 0, sbase > 0) and the column slabs (JS < M) run under
// ASan + UBSan before they run on a GPU.  The LDS a block gets is what the host's own formula gives (crbm_plan.h,
// big_vgh_geom), to the byte.  tests/test_emu_big_vgh.py builds it, runs it directly and compares the letters with the oracle.
// usage: big_vgh_main <in> <out>
//   in:  13 int32 (A, K, M, ds, nchains, Lf, JS (0: the host's), threads, grid, seed_lo, seed_hi, step, seq_offset), then as
//        float32 W[K][A][M], c[A], then as uint32 the masks hm[nchains][Lf][NW] and, for ds, hmp
//   out: 3 int32 (LWs, JS, CH), then uint32 vout[nchains][LWs]
//   prints "BIG_VGH OK chunks=<n> col_slabs=<n> lds=<bytes>"
#define CRBM_DEFINE_MISC_KERNELS
#include "crbm_kernels.h"
#include "crbm_plan.h"
#include "emu_launch.h"

#include <cstdio>
#include <cstdlib>
#include <cstring>

// block after block: the letters are compared with the oracle's one by one
const bool emu::concurrent_blocks = false;

using namespace crbm;

namespace {
template <typename T>
bool read_n(FILE* f, std::vector<T>& v, size_t n) {
  v.resize(n);
  return n == 0 || fread(v.data(), sizeof(T), n, f) == n;
}
}  // namespace

int main(int argc, char** argv) {
  if (argc != 3) { fprintf(stderr, "usage: %s <in> <out>\n", argv[0]); return 2; }
  FILE* in = fopen(argv[1], "rb");
  if (!in) { perror(argv[1]); return 2; }
  std::vector<int32_t> hd;
  if (!read_n(in, hd, 13)) { fprintf(stderr, "short header\n"); return 2; }
  const int A = hd[0], K = hd[1], M = hd[2], ds = hd[3], nchains = hd[4], Lf = hd[5], threads = hd[7], grid = hd[8];
  if (A < 1 || A > 64 || K < 1 || M < 1 || nchains < 1 || Lf < 1 || threads < 64 || threads % 64 || grid < 1 || hd[6] < 0 || hd[6] > M) {
    fprintf(stderr, "bad header\n");
    return 2;
  }
  const int NW = (K + 31) / 32, Lv = Lf + M - 1, LWs = letter_words_any(A, Lv);
  std::vector<float> W, c;
  std::vector<uint32_t> hm, hmp;
  const size_t words = (size_t)nchains * Lf * NW;
  if (!read_n(in, W, (size_t)K * A * M) || !read_n(in, c, (size_t)A) || !read_n(in, hm, words) || !read_n(in, hmp, ds ? words : 0)) {
    fprintf(stderr, "short input\n");
    return 2;
  }
  fclose(in);
  const BigVghGeom g = big_vgh_geom(A, M, Lv, threads, hd[6]);
  std::vector<uint32_t> vout((size_t)nchains * LWs, 0xDEADBEEFu);      // every word must be written, the pad words with zero
  BigVghArgs v;
  v.m.W = W.data(); v.m.b = nullptr; v.m.c = c.data();
  v.m.K = K; v.m.M = M; v.m.ds = ds; v.m.NW = NW; v.m.A = A;
  v.hm = hm.data(); v.hmp = ds ? hmp.data() : nullptr; v.vout = vout.data();
  v.nchains = nchains; v.Lf = Lf; v.Lv = Lv; v.LWs = LWs; v.JS = g.JS;
  v.rng.seed_lo = (uint32_t)hd[9]; v.rng.seed_hi = (uint32_t)hd[10]; v.rng.step = (uint32_t)hd[11]; v.rng.seq_offset = (uint32_t)hd[12];
  if (A == 4) emu::launch([&] { big_vgh_kernel(v); }, dim3(grid), dim3(threads), g.lds);
  else emu::launch([&] { big_vgh_any_kernel(v); }, dim3(grid), dim3(threads), g.lds);
  FILE* out = fopen(argv[2], "wb");
  if (!out) { perror(argv[2]); return 2; }
  const int32_t oh[3] = {LWs, g.JS, g.CH};
  if (fwrite(oh, sizeof(int32_t), 3, out) != 3 || fwrite(vout.data(), sizeof(uint32_t), vout.size(), out) != vout.size()) {
    fprintf(stderr, "short write\n");
    return 2;
  }
  fclose(out);
  printf("BIG_VGH OK chunks=%d col_slabs=%d lds=%zu\n", (Lv + g.CH - 1) / g.CH, (M + g.JS - 1) / g.JS, g.lds);
  return 0;
}
