// TEST INFRASTRUCTURE: runs the mutagenesis kernels of crbm_amd/csrc (mutagenesis_body, the fused pass of the
// specialised models; mutagenesis_expand_kernel and mutagenesis_combine_kernel, the general path around the models'
// own free-energy pass, here free_energy_body) on CPU threads under ASan/UBSan, like emu_sites.cpp does for the
// motif-site kernels.  Plain C entry points for tests/test_emu_mutagenesis.py (ctypes).
#define CRBM_DEFINE_MISC_KERNELS
#include "crbm_kernels.h"

#include <thread>
#include <vector>

namespace emu {
thread_local dim3 t_threadIdx, t_blockIdx, t_blockDim, t_gridDim;
thread_local BlockCtx* t_ctx;

// all blocks of the grid at once, every thread an OS thread; the LDS at its exact size, so that ASan sees overruns
template <typename F>
void launch(F kernel, dim3 grid, dim3 block, size_t lds) {
  const unsigned nthr = block.x, nwaves = (block.x + 63) / 64, nblocks = grid.x * grid.y;
  std::vector<BlockCtx> ctx(nblocks);
  std::vector<std::vector<pthread_barrier_t>> wb(nblocks, std::vector<pthread_barrier_t>(nwaves));
  std::vector<std::vector<float>> scratch(nblocks, std::vector<float>(nwaves * 64));
  std::vector<std::vector<uint32_t>> frag(nblocks, std::vector<uint32_t>((size_t)nwaves * 64 * 8));
  std::vector<std::vector<float4>> smem(nblocks, std::vector<float4>((lds + 15) / 16 + 1));
  std::vector<std::thread> threads;
  threads.reserve((size_t)nblocks * nthr);
  for (unsigned b = 0; b < nblocks; ++b) {
    pthread_barrier_init(&ctx[b].bar, nullptr, nthr);
    for (unsigned w = 0; w < nwaves; ++w) pthread_barrier_init(&wb[b][w], nullptr, std::min(64u, nthr - w * 64));
    memset(smem[b].data(), 0xAB, smem[b].size() * 16);
    ctx[b].wave_bar = wb[b].data();
    ctx[b].wave_scratch = scratch[b].data();
    ctx[b].wave_frag = frag[b].data();
    ctx[b].smem = reinterpret_cast<unsigned char*>(smem[b].data());
    for (unsigned t = 0; t < nthr; ++t)
      threads.emplace_back([&, b, t]() {
        t_threadIdx = dim3(t, 0, 0);
        t_blockIdx = dim3(b % grid.x, b / grid.x, 0);
        t_blockDim = block;
        t_gridDim = grid;
        t_ctx = &ctx[b];
        kernel();
      });
  }
  for (auto& th : threads) th.join();
  for (unsigned b = 0; b < nblocks; ++b) {
    pthread_barrier_destroy(&ctx[b].bar);
    for (auto& w : wb[b]) pthread_barrier_destroy(&w);
  }
}
}  // namespace emu

using namespace crbm;

// the model configurations of the cases (K, M, DS, G, POOL)
#define MUT_DISPATCH(id, ...)                                            \
  switch (id) {                                                          \
    case 0: { using C = Cfg<10, 15, 1, 3>; __VA_ARGS__; break; }         \
    case 1: { using C = Cfg<10, 5, 0, 2>; __VA_ARGS__; break; }          \
    case 2: { using C = Cfg<5, 1, 1, 1>; __VA_ARGS__; break; }           \
    case 3: { using C = Cfg<20, 15, 1, 2>; __VA_ARGS__; break; }         \
    case 4: { using C = Cfg<6, 40, 1, 2>; __VA_ARGS__; break; }          \
    case 5: { using C = Cfg<6, 7, 1, 2, 2>; __VA_ARGS__; break; }        \
    default: return -1;                                                  \
  }

extern "C" {

int emu_mut_info(int id, int* out) {   // K, M, DS, POOL, TABLES, TAB
  MUT_DISPATCH(id, (out[0] = C::K, out[1] = C::M, out[2] = C::DS, out[3] = C::POOL, out[4] = C::TABLES_ALL, out[5] = C::TAB));
  return 0;
}

int emu_mut_letter_words(int A, int L) { return letter_words_any(A, L); }

int emu_mut_encode(const float* v, uint32_t* letters, uint32_t* flags, int n, int L) {
  EncodeArgs a{v, letters, flags, n, L, letter_words(L), 4};
  emu::launch([&] { encode_onehot_kernel(a); }, dim3(2), dim3(64), 0);
  return 0;
}

int emu_mut_tables(int id, const float* W, const float* b, const float* c, float* out) {
  TablesArgs a{W, b, c, out};
  MUT_DISPATCH(id, emu::launch([&] { build_tables_body<C>(a); }, dim3(2), dim3(64), 0));
  return 0;
}

// mutagenesis_body over n rows; dfe / pll may be null.  Returns the dynamic LDS bytes of the launch.
int emu_mut_run(int id, const float* tables, const uint32_t* letters, int n, int L, float* dfe, float* pll, int grid, int threads) {
  MutArgs a;
  a.tables = tables; a.letters = letters; a.n = n; a.L = L; a.LW = letter_words(L); a.dfe = dfe; a.pll = pll;
  int lds = 0;
  MUT_DISPATCH(id, (a.Lh = L - C::M + 1, lds = (C::TAB + (threads / 64) * 3 * mut_plane(L)) * 4,
                    emu::launch([&] { mutagenesis_body<C>(a); }, dim3(grid), dim3(threads), (size_t)lds)));
  return lds;
}

int emu_mut_expand(const uint32_t* rows, uint32_t* out, int n, int L, int A, int grid, int threads) {
  MutExpandArgs a{rows, out, n, L, letter_words_any(A, L), A};
  emu::launch([&] { mutagenesis_expand_kernel(a); }, dim3(grid), dim3(threads), 0);
  return 0;
}

// free_energy_body: the per-motif terms (n,K) of packed rows (what the general path runs between expand and combine)
int emu_mut_free_energy(int id, const float* tables, const uint32_t* letters, int n, int L, float* fem, int grid, int threads) {
  FeArgs a;
  a.tables = tables; a.letters = letters; a.n = n; a.L = L; a.LW = letter_words(L); a.fe = nullptr; a.fem = fem;
  MUT_DISPATCH(id, (a.Lh = L - C::M + 1, emu::launch([&] { free_energy_body<C>(a); }, dim3(grid), dim3(threads), (size_t)C::TAB * 4)));
  return 0;
}

int emu_mut_combine(const float* fem, const float* c, const uint32_t* rows, int n, int L, int A, int K, float* dfe, float* pll,
                    int grid, int threads) {
  MutCombineArgs a{fem, c, rows, n, L, letter_words_any(A, L), A, K, dfe, pll};
  emu::launch([&] { mutagenesis_combine_kernel(a); }, dim3(grid), dim3(threads), 0);
  return 0;
}

}  // extern "C"
