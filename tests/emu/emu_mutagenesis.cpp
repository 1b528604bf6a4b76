// TEST INFRASTRUCTURE: runs the mutagenesis kernels of crbm_amd/csrc (mutagenesis_body, the fused pass of the
// specialised models; mutagenesis_expand_kernel and mutagenesis_combine_kernel, the general path around the models'
// own free-energy pass, here free_energy_body) on CPU threads under ASan/UBSan, like emu_sites.cpp does for the
// motif-site kernels.  Plain C entry points for tests/test_emu_mutagenesis.py (ctypes).
#define CRBM_DEFINE_MISC_KERNELS
#include "crbm_kernels.h"
#include "emu_launch.h"

// all blocks of the grid at once, every thread an OS thread
const bool emu::concurrent_blocks = true;

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
  emu::encode_onehot(v, letters, flags, n, L);
  return 0;
}

int emu_mut_tables(int id, const float* W, const float* b, const float* c, float* out) {
  MUT_DISPATCH(id, emu::build_tables<C>(W, b, c, out));
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
