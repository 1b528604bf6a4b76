// TEST INFRASTRUCTURE: what every emulation driver of this folder (emu_*.cpp) needs to run the kernels of
// crbm_amd/csrc/crbm_kernels.h on CPU threads under ASan/UBSan: the objects shim/hip/hip_runtime.h and crbm_kernels.h
// only declare, the launcher, and the entry-point bodies that are the same in every driver.  It defines objects, so
// each driver (one translation unit per library) includes it once; the driver defines emu::concurrent_blocks.
#pragma once
#include "crbm_kernels.h"

#include <deque>
#include <thread>
#include <vector>

// the one primitive of the motif-site kernels the shim does not have (blocks run as concurrent OS threads: a CAS loop);
// crbm_kernels.h declares it for every driver, whether its kernels call it or not
unsigned long long atomicMax(unsigned long long* p, unsigned long long v) {
  unsigned long long old = __atomic_load_n(p, __ATOMIC_RELAXED);
  while (old < v && !__atomic_compare_exchange_n(p, &old, v, false, __ATOMIC_RELAXED, __ATOMIC_RELAXED)) {}
  return old;
}

namespace emu {
thread_local dim3 t_threadIdx, t_blockIdx, t_blockDim, t_gridDim;
thread_local BlockCtx* t_ctx;

// The order of a launch, defined by each driver.  true: all blocks of the grid at once, which exposes what a kernel
// assumes about the order of its blocks (they may combine through atomics only).  false: block after block, for a
// driver whose results are compared bit for bit and whose grids are large.
extern const bool concurrent_blocks;

// One block of a launch: every GPU thread an OS thread, started by the constructor and joined by the destructor.
struct Block {
  BlockCtx ctx;
  std::vector<pthread_barrier_t> wave_bar;
  std::vector<float> scratch;
  std::vector<uint32_t> frag;
  std::vector<float4> smem;
  std::vector<std::thread> threads;

  template <typename F>
  Block(F& kernel, dim3 grid, dim3 block, unsigned b, size_t lds)
      : wave_bar((block.x + 63) / 64), scratch(wave_bar.size() * 64), frag(wave_bar.size() * 64 * 8),
        smem((lds + 15) / 16 + 1) {   // exact size (16-byte aligned base): out-of-bounds LDS accesses trip AddressSanitizer
    const unsigned nthr = block.x;
    pthread_barrier_init(&ctx.bar, nullptr, nthr);
    for (unsigned w = 0; w < wave_bar.size(); ++w) pthread_barrier_init(&wave_bar[w], nullptr, std::min(64u, nthr - w * 64));
    memset(smem.data(), 0xAB, smem.size() * 16);
    ctx.wave_bar = wave_bar.data();
    ctx.wave_scratch = scratch.data();
    ctx.wave_frag = frag.data();
    ctx.smem = reinterpret_cast<unsigned char*>(smem.data());
    threads.reserve(nthr);
    for (unsigned t = 0; t < nthr; ++t)
      threads.emplace_back([this, &kernel, grid, block, b, t]() {
        t_threadIdx = dim3(t, 0, 0);
        t_blockIdx = dim3(b % grid.x, b / grid.x, 0);
        t_blockDim = block;
        t_gridDim = grid;
        t_ctx = &ctx;
        kernel();
      });
  }
  ~Block() {
    for (auto& th : threads) th.join();
    pthread_barrier_destroy(&ctx.bar);
    for (auto& w : wave_bar) pthread_barrier_destroy(&w);
  }
  Block(const Block&) = delete;
  Block& operator=(const Block&) = delete;
};

template <typename F>
void launch(F kernel, dim3 grid, dim3 block, size_t lds) {
  std::deque<Block> running;   // (a deque constructs in place: a running block never moves)
  for (unsigned b = 0; b < grid.x * grid.y; ++b) {
    running.emplace_back(kernel, grid, block, b, lds);
    if (!concurrent_blocks) running.clear();
  }
}

// ---- entry-point bodies shared by the drivers ------------------------------------------------------------------------
template <class C>
void build_tables(const float* W, const float* b, const float* c, float* out, int grid = 2) {
  crbm::TablesArgs a{W, b, c, out};
  launch([&] { crbm::build_tables_body<C>(a); }, dim3(grid), dim3(64), 0);
}

#ifdef CRBM_DEFINE_MISC_KERNELS
inline void encode_onehot(const float* v, uint32_t* letters, uint32_t* flags, int n, int L, int grid = 2) {
  crbm::EncodeArgs a{v, letters, flags, n, L, crbm::letter_words(L), 4};
  launch([&] { crbm::encode_onehot_kernel(a); }, dim3(grid), dim3(64), 0);
}
#endif
}  // namespace emu
