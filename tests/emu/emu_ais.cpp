// TEST INFRASTRUCTURE: runs the annealed-importance-sampling kernel of crbm_amd/csrc (ais_body) on CPU threads under
// ASan/UBSan, like emu_mutagenesis.cpp does for the mutagenesis kernels.  Plain C entry points for
// tests/test_emu_ais.py (ctypes).
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

// the model configurations of the cases (K, M, DS, G)
#define AIS_DISPATCH(id, ...)                                            \
  switch (id) {                                                          \
    case 0: { using C = Cfg<10, 15, 1, 3>; __VA_ARGS__; break; }         \
    case 1: { using C = Cfg<10, 5, 0, 2>; __VA_ARGS__; break; }          \
    case 2: { using C = Cfg<5, 1, 1, 1>; __VA_ARGS__; break; }           \
    case 3: { using C = Cfg<70, 3, 0, 2>; __VA_ARGS__; break; }          \
    case 4: { using C = Cfg<40, 4, 1, 2>; __VA_ARGS__; break; }          \
    case 5: { using C = Cfg<6, 40, 1, 2>; __VA_ARGS__; break; }          \
    default: return -1;                                                  \
  }

extern "C" {

int emu_ais_info(int id, int* out) {   // K, M, DS, TABLES_ALL
  AIS_DISPATCH(id, (out[0] = C::K, out[1] = C::M, out[2] = C::DS, out[3] = C::TABLES_ALL));
  return 0;
}

int emu_ais_tables(int id, const float* W, const float* b, const float* c, float* out) {
  TablesArgs a{W, b, c, out};
  AIS_DISPATCH(id, emu::launch([&] { build_tables_body<C>(a); }, dim3(2), dim3(64), 0));
  return 0;
}

// ais_body: steps [t0, t1) of `runs` runs.  Returns the dynamic LDS bytes of the launch.
int emu_ais_run(int id, const float* tables, const float* base_c, const float* betas, uint8_t* state, float* logw, int runs, int L,
                int t0, int t1, uint32_t run_offset, uint64_t seed, int grid, int threads) {
  AisArgs a;
  a.tables = tables; a.base_c = base_c; a.betas = betas; a.state = state; a.logw = logw;
  a.runs = runs; a.L = L; a.t0 = t0; a.t1 = t1;
  a.rng.seed_lo = (uint32_t)(seed & 0xffffffffu); a.rng.seed_hi = (uint32_t)(seed >> 32); a.rng.step = 0; a.rng.seq_offset = run_offset;
  long lds = 0;
  AIS_DISPATCH(id, {
    const ModelShape ms = model_shape(C::K, C::M, C::DS, C::G);
    const AisLayout al = ais_layout(ms, L);
    a.Lh = L - C::M + 1; a.nvb = al.nvb; a.Lrow = al.Lrow; a.LWs = al.LWs; a.run_words = al.run_words;
    lds = ais_lds_bytes(ms, al, threads / 64);
    emu::launch([&] { ais_body<C>(a); }, dim3(grid), dim3(threads), (size_t)lds);
  });
  return (int)lds;
}

}  // extern "C"
