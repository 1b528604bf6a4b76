// TEST INFRASTRUCTURE: a stand-alone program that runs the dense v|h kernel of DNA models (crbm_kernels.h, vgh_dense_kernel)
// on CPU threads with 64-thread blocks and the LDS the host gives it (crbm_plan.h, vgh_dense_lds), and compares the
// activity with a plain double-precision loop over the same inputs: models of one slab and models whose filters pass
// through the LDS in several slabs (vgh_dense_ks), with a ragged last slab, rounds of positions with idle threads and
// several rows per tile.  tests/test_emu_vgh_dense.py builds it with ASan + UBSan and runs it directly.
// prints one line per model and "DENSE OK"
#define CRBM_DEFINE_MISC_KERNELS
#include "crbm_kernels.h"
#include "crbm_plan.h"
#include "emu_launch.h"
#include <cstdio>
#include <cmath>
const bool emu::concurrent_blocks = false;
using namespace crbm;
int run(int K, int M, int ds, int n, int Lh, int TS, int grid) {
  const int L = Lh + M - 1;
  std::vector<float> W((size_t)K*4*M), c(4), h((size_t)n*K*Lh), hp((size_t)n*K*Lh), act((size_t)n*4*L, -7.f), prob(act), smp(act);
  uint64_t s = 12345;
  auto rnd = [&]() { s = s*6364136223846793005ull+1442695040888963407ull; return (float)((s>>33)&0xFFFFFF)/16777216.f; };
  for (auto& w : W) w = rnd()-0.5f;
  for (auto& x : c) x = rnd()-0.5f;
  for (auto& x : h) x = rnd() < 0.05f ? 1.f : 0.f;
  for (auto& x : hp) x = rnd() < 0.05f ? 1.f : 0.f;
  VghArgs a;
  a.W = W.data(); a.c = c.data(); a.K = K; a.M = M; a.hid = h.data(); a.hidp = ds ? hp.data() : nullptr;
  a.n = n; a.Lh = Lh; a.L = L; a.TS = TS; a.divL = make_fastdiv((uint32_t)L);
  a.act = act.data(); a.prob = prob.data(); a.sample = smp.data();
  a.rng.seed_lo = 1; a.rng.seed_hi = 2; a.rng.step = 3; a.rng.seq_offset = 0; a.kind = KIND_API_V;
  emu::launch([&] { vgh_dense_kernel(a); }, dim3(grid), dim3(64), vgh_dense_lds(4, K, M));
  double worst = 0;
  for (int nn = 0; nn < n; ++nn) for (int p = 0; p < L; ++p) for (int al = 0; al < 4; ++al) {
    double y = c[al];
    for (int k = 0; k < K; ++k) for (int j = 0; j < M; ++j) { int sidx = p - j; if (sidx < 0 || sidx >= Lh) continue;
      y += (double)W[((size_t)k*4+al)*M+j]*h[((size_t)nn*K+k)*Lh+sidx];
      if (ds) y += (double)W[((size_t)k*4+(3-al))*M+(M-1-j)]*hp[((size_t)nn*K+k)*Lh+sidx]; }
    worst = std::fmax(worst, std::fabs(y - act[((size_t)nn*4+al)*L+p]));
  }
  double ps = 0, ss = 0; for (float x : prob) ps += x; for (float x : smp) ss += x;
  printf("K=%d M=%d ds=%d ks=%d slabs=%d worst=%g probsum=%g samplesum=%g (n*L=%d)\n", K, M, ds, vgh_dense_ks(K,M), (K+vgh_dense_ks(K,M)-1)/vgh_dense_ks(K,M), worst, ps, ss, n*L);
  return worst < 1e-4 && std::fabs(ps - n*L) < 1e-2 && ss == n*L ? 0 : 1;
}
int main() {
  int rc = 0;
  rc |= run(10, 15, 1, 3, 47, 2, 2);
  rc |= run(300, 40, 1, 2, 20, 1, 2);
  rc |= run(256, 64, 0, 2, 20, 4, 1);
  rc |= run(4099, 1, 0, 3, 30, 1, 2);
  rc |= run(9, 512, 1, 1, 5, 1, 1);
  printf(rc ? "FAIL\n" : "DENSE OK\n");
  return rc;
}
