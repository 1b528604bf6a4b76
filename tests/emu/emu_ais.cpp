// TEST INFRASTRUCTURE: runs the annealed-importance-sampling kernel of crbm_amd/csrc (ais_body) on CPU threads under
// ASan/UBSan, like emu_mutagenesis.cpp does for the mutagenesis kernels.  Plain C entry points for
// tests/test_emu_ais.py (ctypes).
#include "crbm_kernels.h"
#include "emu_launch.h"

// all blocks of the grid at once, every thread an OS thread
const bool emu::concurrent_blocks = true;

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
  AIS_DISPATCH(id, emu::build_tables<C>(W, b, c, out));
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
