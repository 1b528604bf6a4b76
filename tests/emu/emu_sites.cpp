// TEST INFRASTRUCTURE: runs the motif-site kernels of crbm_amd/csrc/crbm_kernels.h (motif_sites_body, the fused
// pass of the specialised models, and motif_sites_select_kernel, the generic models' pass over dense probabilities)
// on CPU threads under ASan/UBSan, like emu_main.cpp does for the other kernels.  Plain C entry points for
// tests/test_emu_sites.py (ctypes).
#define CRBM_DEFINE_MISC_KERNELS
#include "crbm_kernels.h"
#include "emu_launch.h"

// all blocks of the grid at once (the site kernels combine across blocks with atomics only)
const bool emu::concurrent_blocks = true;

using namespace crbm;

// the model configurations of the site cases (K, M, DS, G, POOL)
#define SITES_DISPATCH(id, ...)                                          \
  switch (id) {                                                          \
    case 0: { using C = Cfg<10, 15, 1, 3>; __VA_ARGS__; break; }         \
    case 1: { using C = Cfg<6, 7, 1, 2, 2>; __VA_ARGS__; break; }        \
    case 2: { using C = Cfg<10, 5, 0, 2>; __VA_ARGS__; break; }          \
    case 3: { using C = Cfg<20, 15, 1, 2>; __VA_ARGS__; break; }         \
    default: return -1;                                                  \
  }

extern "C" {

int emu_sites_info(int id, int* out) {   // K, M, DS, POOL, TABLES, HIT_NI
  SITES_DISPATCH(id, (out[0] = C::K, out[1] = C::M, out[2] = C::DS, out[3] = C::POOL, out[4] = C::TABLES_ALL,
                      out[5] = C::HIT_NI));
  return 0;
}

int emu_sites_letter_words(int L) { return letter_words(L); }

int emu_sites_encode(const float* v, uint32_t* letters, uint32_t* flags, int n, int L) {
  emu::encode_onehot(v, letters, flags, n, L);
  return 0;
}

int emu_sites_tables(int id, const float* W, const float* b, const float* c, float* out) {
  SITES_DISPATCH(id, emu::build_tables<C>(W, b, c, out));
  return 0;
}

// motif_sites_body over n rows; recs / best may be null.  Returns the number of position chunks (gridDim.y).
int emu_sites_run(int id, const float* tables, const uint32_t* letters, int n, int L, float threshold, SiteRec* recs,
                  unsigned long long capacity, unsigned long long* count, unsigned long long* best, int grid, int threads) {
  SitesArgs a;
  a.tables = tables; a.letters = letters; a.n = n; a.L = L; a.LW = letter_words(L);
  a.o.recs = recs; a.o.capacity = capacity; a.o.count = count; a.o.best = best; a.o.threshold = threshold;
  int chunks = 0;
  SITES_DISPATCH(id, (a.Lh = L - C::M + 1, chunks = (a.Lh + 64 * C::HIT_NI - 1) / (64 * C::HIT_NI),
                      emu::launch([&] { motif_sites_body<C>(a); }, dim3(grid, chunks), dim3(threads), (size_t)C::TAB * 4)));
  return chunks;
}

// motif_sites_select_kernel over dense (n,K,Lh) probabilities; p1 null: one strand
int emu_sites_select(const float* p0, const float* p1, int n, int K, int Lh, int ds, float threshold, SiteRec* recs,
                     unsigned long long capacity, unsigned long long* count, unsigned long long* best, int grid, int threads) {
  SitesSelectArgs a;
  a.p0 = p0; a.p1 = p1; a.n = n; a.K = K; a.Lh = Lh; a.ds = ds;
  a.o.recs = recs; a.o.capacity = capacity; a.o.count = count; a.o.best = best; a.o.threshold = threshold;
  emu::launch([&] { motif_sites_select_kernel(a); }, dim3(grid), dim3(threads), 0);
  return 0;
}

}  // extern "C"
