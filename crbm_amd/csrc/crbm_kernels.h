// CDNA4 (gfx950) kernels of the CRBM hot path.  Wave64 throughout.
//
// The model-dependent kernels are templates over crbm::Cfg<K,M,DS,G> and are
// compiled per model by hiprtc when a handle is created (crbm_jit.h) -- the
// counterpart of the reference compiling its Theano graph at construction
// (convRBM.py:175, :453-515).  K, M, the strand count and the table grouping
// are therefore compile-time constants: every motif loop is unrolled into
// registers and every LDS table offset is an instruction immediate.
//
// Design (details in DESIGN.md):
//  * The visible layer is one-hot wherever the forward correlation is applied
//    (reference sequences.py:28-31, convRBM.py:304-310), so a sequence is kept
//    as 2-bit letters and x[k,s] = b[k] + sum_j W[k, letter[s+j], j] becomes a
//    gather-add.  Letters are taken G at a time: LDS holds pre-summed rows
//    T[g][letter-tuple][k], one ds_read_b128 feeds four motifs.
//  * The hidden layer is binary wherever the transposed convolution is applied
//    (convRBM.py:259-267), so chain state is a K-bit mask per hidden position.
//    For small K*M the top-down pass is a dense walk over pre-summed tables
//    indexed by 5-bit mask chunks; otherwise it adds W[k,:,j] per set bit.
//  * One workgroup owns whole chains and one thread owns 4 consecutive
//    positions, so a k-step Gibbs chain runs entirely in LDS/registers; HBM
//    sees the masks once in and once out per launch.
//  * The convolution and its transpose do not use MFMA: the transposed conv has
//    output width 4 and the forward has one-hot operands (BASELINE.json
//    north_star).  The gradient statistics -- a K x 4M output contracted over
//    all positions of the batch -- do (stats_mfma_*).
//  * The reverse-complement strand needs no table of its own: its activation is
//    the forward gather of the reverse-complemented letter window.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "crbm_layout.h"

namespace crbm {

template <int I>
struct IC {
  static constexpr int value = I;
};

// ---------------------------------------------------------------------------
// Philox-4x32-7 (Random123 constants; seven rounds is the fewest that its authors report as passing BigCrush --
// Salmon et al., SC'11, table 2 -- and what Random123 ships as philox4x32_R<7>); same counters and the same
// round count as oracle/crbm_oracle.py and its C port.  The stream is this library's own definition: the
// reference seeds Theano's MRG31k3p from the wall clock (convRBM.py:155), so there is no stream to match.
// ---------------------------------------------------------------------------
struct Philox4 {
  uint32_t v[4];
};

// ---------------------------------------------------------------------------
// The one place that depends on the compiler: hipcc / hiprtc (clang) get the
// gfx950 instructions, the CPU emulation build of the same header (g++,
// tests/emu) gets portable equivalents supplied by its shim.
// ---------------------------------------------------------------------------
struct HalfFrag {     // eight f16 = one A or B fragment of v_mfma_f32_16x16x32_f16
  uint32_t r[4];
};
#if defined(__clang__)
typedef float floatx4 __attribute__((ext_vector_type(4)));
// a ^ b ^ c in one instruction (v_bitop3_b32, truth table 0x96); the compiler does not fuse it itself
__device__ __forceinline__ uint32_t xor3(uint32_t a, uint32_t b, uint32_t c) { return __builtin_amdgcn_bitop3_b32(a, b, c, 0x96); }
__device__ __forceinline__ uint32_t bitrev32(uint32_t x) { return __builtin_bitreverse32(x); }   // v_bfrev_b32
// (x << SH) | acc in one instruction (v_lshl_or_b32): left to itself the compiler shifts two operands apart and joins
// them with a v_or3_b32, three instructions where two of these do
template <int SH>
__device__ __forceinline__ uint32_t shl_or(uint32_t x, uint32_t acc) {
#if defined(__HIP_DEVICE_COMPILE__)
  uint32_t r;
  asm("v_lshl_or_b32 %0, %1, %2, %3" : "=v"(r) : "v"(x), "n"(SH), "v"(acc));
  return r;
#else
  return (x << SH) | acc;
#endif
}
// a value that is the same in every lane of the wave, pinned to a scalar register at this point (no instruction): the
// compiler can neither fold it into the vector expression it feeds nor pull a constant out of it (it moves constants
// to the outermost xor of a chain, which turns scalar work back into vector work).  Only for wave-uniform values.
__device__ __forceinline__ uint32_t uniform_word(uint32_t x) {
#if defined(__HIP_DEVICE_COMPILE__)
  x = __builtin_amdgcn_readfirstlane(x);     // folds away where x already sits in a scalar register
  asm("" : "+s"(x));
#endif
  return x;
}
// max of four finite floats in two instructions (v_max3_f32, v_max_f32).  fmaxf puts a canonicalising v_max_f32 x, x
// in front of every operand the compiler cannot prove canonical (a value that may come straight from memory); no
// operand here is ever a NaN, and the result is the same number whatever the order (with zeros of both signs among
// the largest the sign of the result may differ: callers subtract it and take 2^x, which is 1 for either zero).
__device__ __forceinline__ float max4_finite(float a, float b, float c, float d) {
#if defined(__HIP_DEVICE_COMPILE__)
  float m, r;
  asm("v_max3_f32 %0, %1, %2, %3" : "=v"(m) : "v"(a), "v"(b), "v"(c));
  asm("v_max_f32 %0, %1, %2" : "=v"(r) : "v"(m), "v"(d));
  return r;
#else
  return fmaxf(fmaxf(a, b), fmaxf(c, d));
#endif
}
// 16-byte store that does not linger in the caches (the chain state is written once
// per launch and next read by another launch: measured 0.45 us per launch at config #2)
__device__ __forceinline__ void store4_streaming(uint32_t* dst, uint32_t x, uint32_t y, uint32_t z, uint32_t w) {
  typedef uint32_t u4v __attribute__((ext_vector_type(4)));
  const u4v val = {x, y, z, w};
  __builtin_nontemporal_store(val, reinterpret_cast<u4v*>(dst));
}
__device__ __forceinline__ void store1_streaming(uint32_t* dst, uint32_t x) { __builtin_nontemporal_store(x, dst); }
// all vector-memory operations of this wave have completed (gfx9 encoding: vmcnt = 0, expcnt and lgkmcnt untouched)
__device__ __forceinline__ void wait_vector_memory() { __builtin_amdgcn_s_waitcnt(0x0F70); }
// System-scope accesses for memory another process / another GPU reads and writes (the mapped sums buffers of the
// IPC all-reduce): loads and stores that bypass this GPU's caches, and the fence that orders them.
__device__ __forceinline__ float load_system(const float* p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM); }
__device__ __forceinline__ uint32_t load_system(const uint32_t* p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM); }
__device__ __forceinline__ void store_system(float* p, float v) { __hip_atomic_store(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM); }
__device__ __forceinline__ void store_system(uint32_t* p, uint32_t v) { __hip_atomic_store(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM); }
__device__ __forceinline__ void fence_system() { __threadfence_system(); }
// what a consumer needs after it has seen a producer's flag: later loads may not be served from lines cached before
__device__ __forceinline__ void fence_acquire_system() { __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, ""); }
// arrival counter of the blocks of one launch: the increment publishes the block's stores (release) and the block
// that draws the last ticket sees everybody's (acquire), at the scope of this GPU
__device__ __forceinline__ uint32_t ticket_add(uint32_t* p) { return __hip_atomic_fetch_add(p, 1u, __ATOMIC_ACQ_REL, __HIP_MEMORY_SCOPE_AGENT); }
__device__ __forceinline__ void short_sleep() { __builtin_amdgcn_s_sleep(8); }
// the GPU's constant-rate wall clock (s_memrealtime; hipDeviceAttributeWallClockRate ticks per millisecond): bounds
// the waits for another process in TIME, whatever the shader clock does
__device__ __forceinline__ uint64_t realtime_ticks() { return __builtin_amdgcn_s_memrealtime(); }
__device__ __forceinline__ uint64_t shader_cycles() { return __builtin_amdgcn_s_memtime(); }   // counts shader clocks
// x = hi + lo with both halves f16 (round to nearest): 22 significant bits, v_cvt_pk_f16_f32 +
// v_cvt_f32_f16 + v_pk_add_f32 per pair
__device__ __forceinline__ void split_f16(const float (&x)[8], HalfFrag& hi, HalfFrag& lo) {
  typedef _Float16 half8 __attribute__((ext_vector_type(8)));
  half8 h, l;
#pragma unroll
  for (int e = 0; e < 8; ++e) {
    h[e] = (_Float16)x[e];
    l[e] = (_Float16)(x[e] - (float)h[e]);
  }
  hi = __builtin_bit_cast(HalfFrag, h);
  lo = __builtin_bit_cast(HalfFrag, l);
}
// D = A (16 x 32) * B (32 x 16) + C on the matrix core.  Lane l holds A[row l&15][8(l>>4) .. +7],
// B[8(l>>4) .. +7][col l&15] and D[rows 4(l>>4) .. +3][col l&15] (checked with integer data on gfx950:
// tools/mfma_probe.hip)
__device__ __forceinline__ floatx4 mfma_16x16x32_f16(const HalfFrag& a, const HalfFrag& b, floatx4 c) {
  typedef _Float16 half8 __attribute__((ext_vector_type(8)));
  return __builtin_amdgcn_mfma_f32_16x16x32_f16(__builtin_bit_cast(half8, a), __builtin_bit_cast(half8, b), c, 0, 0, 0);
}
// two floats = one v_pk_*_f32 operand; a * b + c as one v_pk_fma_f32; `opaque` hides where a value came
// from (no instruction), so that float(field) + 1 stays a packed add instead of a second conversion
typedef float floatx2 __attribute__((vector_size(8)));
__device__ __forceinline__ floatx2 fma2(floatx2 a, floatx2 b, floatx2 c) { return __builtin_elementwise_fma(a, b, c); }
__device__ __forceinline__ floatx2 opaque(floatx2 v) { asm volatile("" : "+v"(v)); return v; }
// lanes of `mask` below this lane (v_mbcnt_lo / v_mbcnt_hi)
__device__ __forceinline__ uint32_t lanes_below(unsigned long long mask) {
  return __builtin_amdgcn_mbcnt_hi((uint32_t)(mask >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)mask, 0u));
}
#else   // CPU emulation build (tests/emu/shim/hip/hip_runtime.h implements the wave-wide parts)
typedef float floatx4 __attribute__((vector_size(16)));
typedef float floatx2 __attribute__((vector_size(8)));
__device__ __forceinline__ floatx2 fma2(floatx2 a, floatx2 b, floatx2 c) { return floatx2{fmaf(a[0], b[0], c[0]), fmaf(a[1], b[1], c[1])}; }
__device__ __forceinline__ floatx2 opaque(floatx2 v) { return v; }
__device__ __forceinline__ uint32_t xor3(uint32_t a, uint32_t b, uint32_t c) { return a ^ b ^ c; }
__device__ __forceinline__ float max4_finite(float a, float b, float c, float d) { return fmaxf(fmaxf(a, b), fmaxf(c, d)); }
__device__ __forceinline__ uint32_t uniform_word(uint32_t x) { return x; }
template <int SH> __device__ __forceinline__ uint32_t shl_or(uint32_t x, uint32_t acc) { return (x << SH) | acc; }
__device__ __forceinline__ uint32_t bitrev32(uint32_t x) {
  x = ((x >> 1) & 0x55555555u) | ((x & 0x55555555u) << 1);
  x = ((x >> 2) & 0x33333333u) | ((x & 0x33333333u) << 2);
  x = ((x >> 4) & 0x0F0F0F0Fu) | ((x & 0x0F0F0F0Fu) << 4);
  x = ((x >> 8) & 0x00FF00FFu) | ((x & 0x00FF00FFu) << 8);
  return (x >> 16) | (x << 16);
}
__device__ __forceinline__ void store4_streaming(uint32_t* dst, uint32_t x, uint32_t y, uint32_t z, uint32_t w) {
  *reinterpret_cast<uint4*>(dst) = make_uint4(x, y, z, w);
}
__device__ __forceinline__ void store1_streaming(uint32_t* dst, uint32_t x) { *dst = x; }
__device__ __forceinline__ void wait_vector_memory() {}
__device__ __forceinline__ float load_system(const float* p) { float v; __atomic_load(p, &v, __ATOMIC_RELAXED); return v; }
__device__ __forceinline__ uint32_t load_system(const uint32_t* p) { return __atomic_load_n(p, __ATOMIC_RELAXED); }
__device__ __forceinline__ void store_system(float* p, float v) { __atomic_store(p, &v, __ATOMIC_RELAXED); }
__device__ __forceinline__ void store_system(uint32_t* p, uint32_t v) { __atomic_store_n(p, v, __ATOMIC_RELAXED); }
__device__ __forceinline__ void fence_system() { __atomic_thread_fence(__ATOMIC_SEQ_CST); }
__device__ __forceinline__ void fence_acquire_system() { __atomic_thread_fence(__ATOMIC_ACQUIRE); }
__device__ __forceinline__ uint32_t ticket_add(uint32_t* p) { return __atomic_fetch_add(p, 1u, __ATOMIC_ACQ_REL); }
__device__ __forceinline__ void short_sleep() {}
__device__ __forceinline__ uint64_t realtime_ticks() { return emu::realtime_ticks(); }   // microseconds
__device__ __forceinline__ uint64_t shader_cycles() { return emu::realtime_ticks(); }
__device__ __forceinline__ void split_f16(const float (&x)[8], HalfFrag& hi, HalfFrag& lo) { emu::split_f16(x, hi.r, lo.r); }
__device__ __forceinline__ uint32_t lanes_below(unsigned long long mask) {
  return (uint32_t)__popcll(mask & ((1ull << (threadIdx.x & 63u)) - 1ull));
}
}  // namespace crbm
// supplied by the driver that runs the motif-site kernels (tests/emu/emu_sites.cpp); nothing else calls it
unsigned long long atomicMax(unsigned long long* p, unsigned long long v);
namespace crbm {
__device__ __forceinline__ floatx4 mfma_16x16x32_f16(const HalfFrag& a, const HalfFrag& b, floatx4 c) {
  float d[4] = {c[0], c[1], c[2], c[3]};
  emu::mfma_16x16x32_f16(a.r, b.r, d);
  return floatx4{d[0], d[1], d[2], d[3]};
}
#endif

#ifndef CRBM_PHILOX_ROUNDS
#define CRBM_PHILOX_ROUNDS 7      // anything else (CRBM_JIT_DEFINES) is a timing experiment: the oracle draws seven
#endif
// A/B knobs of the second instruction diet (CRBM_JIT_DEFINES=-DCRBM_DIET2_<part>=0 takes one part out alone; every
// part leaves every bit of every result as it is):
//   CRBM_DIET2_A   sample_hidden: the exact path reads the coarse fields behind `opaque` (no register-pair copies)
//   CRBM_DIET2_B   sample_hidden: coarse fields that do not straddle a word are converted where they sit
//   CRBM_DIET2_C1  philox4x32<true>: the wave-uniform words of rounds 1-2 are joined on the scalar unit.  Not in the chain
//                  kernel of models that defer their undecided units (gibbs_body, DEFER: double-stranded, unpooled):
//                  there it was measured to COST time (config #5: 125.6-126.2 us per launch with it, 124.8-125.0
//                  without, parent commit 126.2-126.9), so both call sites of that kernel take the plain form.
#ifndef CRBM_DIET2_A
#define CRBM_DIET2_A 1
#endif
#ifndef CRBM_DIET2_B
#define CRBM_DIET2_B 1
#endif
#ifndef CRBM_DIET2_C1
#define CRBM_DIET2_C1 1
#endif
// UNIFORM: c2, c3, k0 and k1 are the same in every lane of the wave (the counter word of a kind, the step, the seed:
// every call site of a sampling pass), c0 and c1 (sequence, position) are not.  A v_bitop3_b32 takes ONE scalar
// operand, so the three xors of rounds 1-2 that join two uniform words -- hi(M1 c2) ^ k0, c3 ^ k1 and, a round later,
// lo(M1 c2) ^ (k0 + golden) -- each cost a v_mov_b32 of a scalar in front of them, inside the item loops.  Written as
// x ^ uniform_word(u ^ u') the inner xor is scalar work and the outer one a v_xor_b32 with one scalar operand: the same
// value (xor is associative), three vector instructions fewer per call.
// CONTRACT of philox4x32<true>: c2, c3, k0 and k1 MUST be wave-uniform.  uniform_word reads them from the first active
// lane, so a lane-varying word would give every lane that lane's stream, silently.  A caller whose kind, strand,
// group, step or seed differs between the lanes of a wave takes philox4x32<false>.
template <bool UNIFORM = false>
__device__ __forceinline__ Philox4 philox4x32(uint32_t c0, uint32_t c1, uint32_t c2, uint32_t c3,
                                                 uint32_t k0, uint32_t k1) {
#pragma unroll
  for (int r = 0; r < CRBM_PHILOX_ROUNDS; ++r) {
    const uint64_t p0 = (uint64_t)0xD2511F53u * c0;
    const uint64_t p1 = (uint64_t)0xCD9E8D57u * c2;
    const bool split = UNIFORM && CRBM_DIET2_C1;
    const uint32_t n0 = split && r == 0 ? c1 ^ uniform_word((uint32_t)(p1 >> 32) ^ k0)
                      : split && r == 1 ? (uint32_t)(p1 >> 32) ^ uniform_word(c1 ^ k0)
                                        : xor3((uint32_t)(p1 >> 32), c1, k0);
    const uint32_t n2 = split && r == 0 ? (uint32_t)(p0 >> 32) ^ uniform_word(c3 ^ k1) : xor3((uint32_t)(p0 >> 32), c3, k1);
    c1 = (uint32_t)p1;
    c3 = (uint32_t)p0;
    c0 = n0;
    c2 = n2;
    k0 += 0x9E3779B9u;
    k1 += 0xBB67AE85u;
  }
  Philox4 o;
  o.v[0] = c0; o.v[1] = c1; o.v[2] = c2; o.v[3] = c3;
  return o;
}

// component i (0..3) without dynamic register indexing
__device__ __forceinline__ uint32_t philox_pick(const Philox4& r, int i) {
  const uint32_t lo = (i & 1) ? r.v[1] : r.v[0];
  const uint32_t hi = (i & 1) ? r.v[3] : r.v[2];
  return (i & 2) ? hi : lo;
}

// 12-bit field I (0..9) of the 128-bit little-endian value v0 | v1<<32 | ...
template <int I>
__device__ __forceinline__ uint32_t philox_field12(const Philox4& r) {
  constexpr int w = (12 * I) / 32, b = (12 * I) % 32;
  if (b <= 20) return (r.v[w] >> b) & 0xFFFu;
  return ((r.v[w] >> b) | (r.v[(w + 1) & 3] << ((32 - b) & 31))) & 0xFFFu;
}

// the same for a field index known only at run time (the rare exact path of the chain kernel)
__device__ __forceinline__ uint32_t philox_field12_dyn(const Philox4& r, int i) {
  const int b = 12 * i, w = b >> 5, sh = b & 31;
  uint32_t v = philox_pick(r, w) >> sh;
  if (sh > 20) v |= philox_pick(r, (w + 1) & 3) << (32 - sh);
  return v & 0xFFFu;
}

__device__ __forceinline__ float u01(uint32_t r) { return (float)(r >> 8) * 5.9604644775390625e-8f; }

// counter word 2: kind | strand | sub-stream (0 coarse, 1 fine) | group
__device__ __forceinline__ uint32_t rng_word2(uint32_t kind, uint32_t strand, uint32_t sub, uint32_t group) {
  return (kind << 28) | (strand << 24) | (sub << 16) | group;
}

__device__ __forceinline__ uint32_t fastdiv(uint32_t i, const FastDiv& f) {
  if (f.d <= 1) return i;
  uint32_t q = __umulhi(i, f.inv);
  if (f.fix && q * f.d > i) --q;   // long rows only (crbm_layout.h): the estimate is q or q + 1
  return q;
}
// The Gibbs kernel divides indices of one LDS-resident tile: dividend and divisor are both at most
// the tile's word count (<= 40 960: 160 KB), so n*d < 2^32 and the single mul_hi is always exact.
__device__ __forceinline__ uint32_t fastdiv_tile(uint32_t i, const FastDiv& f) {
  return f.d <= 1 ? i : __umulhi(i, f.inv);
}

// The MFMA statistics carry probabilities scaled by 2^14 (and a one-hot operand of 2^-14):
// the f16 halves of P then stay normal numbers down to P ~ 4e-9 instead of 6e-5.
constexpr float STATS_PSCALE_INV = 6.103515625e-05f;   // 2^-14
// z = -x*log2(e) (what conv_gather returns): exp(-x) = 2^z
__device__ __forceinline__ float exp_neg_x(float z) { return __builtin_amdgcn_exp2f(z); }
// v_rcp_f32 (1 ulp); __fdividef expands to a full division sequence under hiprtc
__device__ __forceinline__ float fast_rcp(float x) { return __builtin_amdgcn_rcpf(x); }
__device__ __forceinline__ float sigmoid_z(float z) { return fast_rcp(1.0f + exp_neg_x(z)); }
__device__ __forceinline__ float x_of_z(float z) { return -0.6931471805599453f * z; }

// sum over the 16 lanes that share lane & 3 (all lanes of the class get the total):
// two row rotations (DPP, VALU only) + two cross-row exchanges
__device__ __forceinline__ float class_sum(float v) {
  v += __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, v), 0x124, 0xf, 0xf, false));   // row_ror:4
  v += __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, v), 0x128, 0xf, 0xf, false));   // row_ror:8
  v += __shfl_xor(v, 16, 64);
  v += __shfl_xor(v, 32, 64);
  return v;
}

// Wave-wide reductions on the VALU (DPP): four row rotations give every lane its
// 16-lane row total, row_bcast15 / row_bcast31 fold the four rows into lane 63,
// one v_readlane hands the result to all lanes.  (The LDS-crossbar shuffles are
// an order of magnitude slower when dozens of values are reduced back to back.)
template <int CTRL, int ROW_MASK>
__device__ __forceinline__ float dpp_move(float v) {
  return __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, v), CTRL, ROW_MASK, 0xf, false));
}

__device__ __forceinline__ float wave_sum(float v) {
  v += dpp_move<0x121, 0xf>(v);   // row_ror:1
  v += dpp_move<0x122, 0xf>(v);   // row_ror:2
  v += dpp_move<0x124, 0xf>(v);   // row_ror:4
  v += dpp_move<0x128, 0xf>(v);   // row_ror:8
  v += dpp_move<0x142, 0xa>(v);   // row_bcast15 into rows 1 and 3
  v += dpp_move<0x143, 0xc>(v);   // row_bcast31 into rows 2 and 3
  return __builtin_bit_cast(float, __builtin_amdgcn_readlane(__builtin_bit_cast(int, v), 63));
}

// maximum of non-negative values (rows a DPP move does not reach contribute 0)
__device__ __forceinline__ float wave_max_nonneg(float v) {
  v = fmaxf(v, dpp_move<0x121, 0xf>(v));
  v = fmaxf(v, dpp_move<0x122, 0xf>(v));
  v = fmaxf(v, dpp_move<0x124, 0xf>(v));
  v = fmaxf(v, dpp_move<0x128, 0xf>(v));
  v = fmaxf(v, dpp_move<0x142, 0xa>(v));
  v = fmaxf(v, dpp_move<0x143, 0xc>(v));
  return __builtin_bit_cast(float, __builtin_amdgcn_readlane(__builtin_bit_cast(int, v), 63));
}

// maximum of unsigned integers, the same DPP moves (0 is the identity here too)
__device__ __forceinline__ uint32_t umax32(uint32_t a, uint32_t b) { return a > b ? a : b; }
__device__ __forceinline__ uint32_t wave_max_u32(uint32_t v) {
  auto move = [](uint32_t x, auto CTRL, auto ROW_MASK) {
    return (uint32_t)__builtin_amdgcn_update_dpp(0, (int)x, decltype(CTRL)::value, decltype(ROW_MASK)::value, 0xf, false);
  };
  v = umax32(v, move(v, IC<0x121>{}, IC<0xf>{}));
  v = umax32(v, move(v, IC<0x122>{}, IC<0xf>{}));
  v = umax32(v, move(v, IC<0x124>{}, IC<0xf>{}));
  v = umax32(v, move(v, IC<0x128>{}, IC<0xf>{}));
  v = umax32(v, move(v, IC<0x142>{}, IC<0xa>{}));
  v = umax32(v, move(v, IC<0x143>{}, IC<0xc>{}));
  return (uint32_t)__builtin_amdgcn_readlane((int)v, 63);
}

// ---------------------------------------------------------------------------
// Sampling K hidden units from z = -x*log2(e) of their activations x
// (convRBM.py:259-267: h = 1 if p > u).  The uniform of unit k is 24 bits wide, u = (coarse*4096 + fine) /
// 2^24, where coarse and fine are the (k % 10)-th 12-bit fields of two Philox
// calls shared by the 10 units of group k / 10.  Almost every decision is
// settled by the coarse field alone: with e = exp(-x),
//     (coarse + 1)(1 + e) <= 4096  =>  h = 1,      coarse (1 + e) > 4096  =>  h = 0,
// and the fine call is made only when some lane of the wave lands in between
// (2^-12 per unit).  Returns the K-bit mask; optionally the probabilities.
// ---------------------------------------------------------------------------
// WANT_P: 0 none, 1 p = sigma(x), 2 p = 2^14 * sigma(x) (the scale of the MFMA statistics, below)
//
// The two coarse tests are taken as sign bits: d1 = 4096 - coarse (1 + e) and d2 = 4096 - (coarse + 1)(1 + e)
// (one fused multiply-add each, two units per packed instruction); the sign of d2 is "not certainly 1",
// the sign of d1 "certainly 0".  Both are shifted into a word per group (v_alignbit_b32, units in
// descending order so that unit 0 ends in bit 0): two instructions per unit where compares, selects
// and ors took six.  e = inf (x < -88) gives d2 = -inf (h = 0, correct); d1 can then be NaN for
// coarse = 0, whose sign only decides whether the exact path below is taken -- it returns 0 as well.
__device__ __forceinline__ uint32_t shift_in_sign(uint32_t acc, float d) { return (acc << 1) | (__float_as_uint(d) >> 31); }

// The coarse field as the two tests take it (CRBM_DIET2_B).  Only the SIGNS of d1 and d2 are used, a fused multiply-add
// has the sign of its exact value, and an exact zero stays zero.  A field at bit b <= 20 of its word is converted
// where it sits: (float)(word & (0xFFF << b)) is coarse * 2^b exactly (12 significant bits, nothing to round), and with
// 4096 * 2^b and 2^b in place of 4096 and 1 the exact values of both forms are 2^b times those above -- the same signs
// (the scaled values lie below 2^33 or round to an infinity of the same sign; nothing here can underflow).  One
// mask and one conversion per field, no shift.
// e = inf: (coarse + 1) 2^b > 0 gives d2 = -inf as before; coarse = 0 is 0 in both forms (d1 = NaN for e = inf, see
// above; otherwise d1 = 4096 * 2^b > 0), and d2 = 2^b (4096 - (1 + e)) has the sign of 4096 - (1 + e).
// The two fields that straddle a word boundary (2 and 5) keep philox_field12 and the scale 1.
template <int I>
struct CoarseField {
  static constexpr int w = (12 * I) / 32, b = (12 * I) % 32;
  static constexpr bool IN_PLACE = CRBM_DIET2_B && b <= 20;
  static constexpr float SCALE = IN_PLACE ? (float)(1u << b) : 1.0f;
  static __device__ __forceinline__ float get(const Philox4& r) {
    if constexpr (IN_PLACE) return (float)(r.v[w] & (0xFFFu << b));
    else return (float)philox_field12<I>(r);
  }
};

// DEFER: the undecided units are not resolved here; their bits come back in pending[group] (mask has 0
// there) and the caller resolves them later (gibbs_body queues them per block).
// kind, strand, group0, step and rng's seed MUST be the same in every lane of the wave (philox4x32<true>'s contract,
// above); n and s are per lane.
template <class C, int WANT_P, bool DEFER = false>
__device__ __forceinline__ void sample_hidden(const float (&z)[C::KP], uint32_t n, uint32_t s, uint32_t kind,
                                              uint32_t strand, const RngView& rng, uint32_t step,
                                              uint32_t (&mask)[C::NW], float (&p)[C::KP],
                                              uint32_t* pending = nullptr, uint32_t group0 = 0) {   // group0: sampler group of unit 0 (a slab of a larger model: hgv_masks_body)
#pragma unroll
  for (int w = 0; w < C::NW; ++w) mask[w] = 0u;
#pragma unroll
  for (int g = 0; g < C::NGRP; ++g) {
    const Philox4 rc = philox4x32<!DEFER>(n, s, rng_word2(kind, strand, 0, group0 + (uint32_t)g), step, rng.seed_lo, rng.seed_hi);   // DEFER: see CRBM_DIET2_C1
    constexpr int kFull = 10;
    const int cnt = C::K - 10 * g < kFull ? C::K - 10 * g : kFull;   // units of this group
    uint32_t not_one = 0u, zero = 0u;     // bit i: unit 10g+i is not certainly 1 / is certainly 0
    // CRBM_DIET2_A: the converted fields as they stand behind `opaque`, for the exact path.  Converting them again there
    // looks free but is not: the compiler merges that conversion with the one in front of `opaque`, keeps both copies
    // of the pair alive and pays one v_mov_b64 per pair on the main path.
    // How A and B meet: `pair` keeps in cf[i] what the tests took, coarse * CoarseField<i>::SCALE.  `fix` needs the
    // unscaled field, so it reads cf[i] only where SCALE is 1 -- every slot without B, slots 2 and 5 (the fields that
    // straddle a word) with B -- and extracts the field again, behind the branch, everywhere else; the slots it does
    // not read cost nothing (dead stores of registers).  Without A, or under DEFER (no `fix`), cf is never written.
    float cf[10];
    auto pair = [&](auto I) {             // units i + 1 and i of the group (i even), in that order
      constexpr int i = decltype(I)::value;
      const int k = 10 * g + i;
      if (k < C::K) {
        const bool two = k + 1 < C::K;
        const floatx2 e = {exp_neg_x(z[k]), exp_neg_x(z[two ? k + 1 : k])};
        const floatx2 ope = e + 1.0f;
        using F0 = CoarseField<i>;
        using F1 = CoarseField<i + 1>;
        const floatx2 af = opaque(floatx2{F0::get(rc), F1::get(rc)});            // coarse * SCALE
        const floatx2 c4096 = {4096.0f * F0::SCALE, 4096.0f * F1::SCALE}, one = {F0::SCALE, F1::SCALE};
        const floatx2 d1 = fma2(-af, ope, c4096);             // >= 0: coarse (1 + e) <= 4096
        const floatx2 d2 = fma2(-(af + one), ope, c4096);     // >= 0: (coarse + 1)(1 + e) <= 4096, h = 1
        if (CRBM_DIET2_A && !DEFER) { cf[i] = af[0]; cf[i + 1] = af[1]; }
        if (two) {
          zero = shift_in_sign(zero, d1[1]);
          not_one = shift_in_sign(not_one, d2[1]);
        }
        zero = shift_in_sign(zero, d1[0]);
        not_one = shift_in_sign(not_one, d2[0]);
        if (WANT_P == 1) { p[k] = fast_rcp(ope[0]); if (two) p[k + 1] = fast_rcp(ope[1]); }
        if (WANT_P == 2) {
          const floatx2 os = ope * STATS_PSCALE_INV;
          p[k] = fast_rcp(os[0]);
          if (two) p[k + 1] = fast_rcp(os[1]);
        }
      }
    };
    pair(IC<8>{}); pair(IC<6>{}); pair(IC<4>{}); pair(IC<2>{}); pair(IC<0>{});
    uint32_t ones = ~not_one & ((1u << cnt) - 1u);
    const uint32_t amb = not_one & ~zero;   // units of this group that need the fine field
    if constexpr (DEFER) pending[g] = amb;
    if (!DEFER && __any(amb != 0u)) {
      const Philox4 rf = philox4x32<true>(n, s, rng_word2(kind, strand, 1, group0 + (uint32_t)g), step, rng.seed_lo, rng.seed_hi);
      auto fix = [&](auto I) {
        constexpr int i = decltype(I)::value;
        const int k = 10 * g + i;
        if (k < C::K) {
          if (amb & (1u << i)) {
            // P*4096 - coarse lies in [0,1) up to rounding; compare with fine/4096
            // (the unscaled field: the one kept by `pair` where its scale is 1, extracted again -- behind the
            //  branch, and not the value the main path converts -- where it is not)
            const float t = 4096.0f * fast_rcp(1.0f + exp_neg_x(z[k]));
            const float coarse = CRBM_DIET2_A && CoarseField<i>::SCALE == 1.0f ? cf[i] : (float)philox_field12<i>(rc);
            const float frac = t - coarse;
            ones |= (frac * 4096.0f > (float)philox_field12<i>(rf) ? 1u : 0u) << i;
          }
        }
      };
      fix(IC<0>{}); fix(IC<1>{}); fix(IC<2>{}); fix(IC<3>{}); fix(IC<4>{});
      fix(IC<5>{}); fix(IC<6>{}); fix(IC<7>{}); fix(IC<8>{}); fix(IC<9>{});
    }
    constexpr int kBitsPerWord = 32;
    const int w0 = (10 * g) / kBitsPerWord, sh = (10 * g) % kBitsPerWord;
    mask[w0] |= ones << sh;
    if (sh + cnt > kBitsPerWord) mask[w0 + 1] |= ones >> (kBitsPerWord - sh);
  }
}

// M letters (2 bits each) starting at position s of a packed row: one 64-bit word for M <= 32,
// a second one (letters 32..) for M <= 64 (MAX_MOTIF_LENGTH).
template <int M>
struct LetterWin {
  uint64_t lo, hi;   // hi is never touched for M <= 32
};

template <int M>
__device__ __forceinline__ LetterWin<M> letter_window(const uint32_t* w, int s) {
  static_assert(M <= MAX_MOTIF_LENGTH, "letter windows hold at most 64 letters");
  const int i = s >> 4;
  const int sh = (s & 15) * 2;
  LetterWin<M> out;
  out.hi = 0ull;
  const uint64_t lo = (uint64_t)w[i] | ((uint64_t)w[i + 1] << 32);
  if constexpr (M <= 32) {
    uint64_t win = lo >> sh;
    if (2 * M + 30 > 64) {
      if (sh > 0) win |= (uint64_t)w[i + 2] << (64 - sh);
    }
    if (M < 32) win &= (1ull << (2 * M)) - 1ull;
    out.lo = win;
  } else {
    // bits [sh, sh + 2M) of the five words from w[i] on (the row's two pad words cover the last window: crbm_layout.h)
    const uint64_t mid = (uint64_t)w[i + 2] | ((uint64_t)w[i + 3] << 32);
    const uint64_t top = (uint64_t)w[i + 4];
    out.lo = sh > 0 ? (lo >> sh) | (mid << (64 - sh)) : lo;
    out.hi = sh > 0 ? (mid >> sh) | (top << (64 - sh)) : mid;
    if (M < 64) out.hi &= (1ull << (2 * (M - 32))) - 1ull;
  }
  return out;
}

// bits [off, off + 8) of a window (off < 2 M; a group's letter tuple is at most 8 bits wide)
template <int M>
__device__ __forceinline__ uint32_t window_bits(const LetterWin<M>& win, int off) {
  if constexpr (M <= 32) return (uint32_t)(win.lo >> off);
  else {
    if (off >= 64) return (uint32_t)(win.hi >> (off - 64));
    return (uint32_t)(off > 0 ? (win.lo >> off) | (win.hi << (64 - off)) : win.lo);
  }
}

// The window of the reverse-complement strand: letter o of the result is the complement of letter M-1-o.
// The reference flips the FILTER for that strand (rc(W)[k,a,j] = W[k,3-a,M-1-j], convRBM.py:241); flipping the
// data instead gives the same activation -- sum_j W[k, 3 - l(s+j), M-1-j] = sum_j' W[k, rc_window[j'], j'] -- as
// the FORWARD gather of the one table Tf (bias and pad columns of group 0 included exactly once, as they
// should be: both strands share the bias, :242).  No second gather table exists anywhere.
__device__ __forceinline__ uint32_t revcomp_word(uint32_t x) {   // 16 letters: order reversed, each complemented
  x = bitrev32(x);                                                // reverses the two bits inside every letter as well ...
  x = ((x >> 1) & 0x55555555u) | ((x & 0x55555555u) << 1);        // ... swap them back
  return ~x;
}

template <int M>
__device__ __forceinline__ LetterWin<M> revcomp_window(const LetterWin<M>& w) {
  LetterWin<M> out;
  out.hi = 0ull;
  // reversing a 64-bit word of 32 letters: both halves reversed, then swapped
  const uint64_t rlo = ((uint64_t)revcomp_word((uint32_t)w.lo) << 32) | revcomp_word((uint32_t)(w.lo >> 32));
  if constexpr (M <= 32) {
    out.lo = M < 32 ? rlo >> (64 - 2 * M) : rlo;        // the M letters sit at the top (the complemented padding below them leaves)
  } else {
    const uint64_t rhi = ((uint64_t)revcomp_word((uint32_t)w.hi) << 32) | revcomp_word((uint32_t)(w.hi >> 32));
    constexpr int sh = 128 - 2 * M;                     // the 128-bit value rlo:rhi (rlo on top), shifted down
    out.lo = sh > 0 ? (rhi >> sh) | (rlo << (64 - sh)) : rhi;
    out.hi = sh > 0 ? rlo >> sh : rlo;
  }
  return out;
}

// z[k] (+)= sum over letter groups of T[g][tuple][k]  (z = -log2(e) * activation).  The sums are kept
// as pairs of floats: one v_pk_add_f32 per two motifs (the compiler leaves scalar adds otherwise).
template <class C, bool ACCUMULATE = false>
__device__ __forceinline__ void conv_gather(const float* T, const LetterWin<C::M>& win, float (&x)[C::KP]) {
  floatx2 acc[2 * C::NQ];
  if (ACCUMULATE) {
#pragma unroll
    for (int q = 0; q < 2 * C::NQ; ++q) acc[q] = floatx2{x[2 * q], x[2 * q + 1]};
  }
  auto group = [&](int g, auto FIRST) {
    constexpr bool first = decltype(FIRST)::value != 0;   // the first group of a fresh sum assigns (saves KP adds of 0)
    const uint32_t r = window_bits<C::M>(win, 2 * C::G * g) & (uint32_t)(C::ROWS - 1);
    const float4* row = reinterpret_cast<const float4*>(T + (size_t)g * C::ROWS * C::KP) + (size_t)r * C::NQ;
#pragma unroll
    for (int q = 0; q < C::NQ; ++q) {
      const float4 t = row[q];
      if (first) {
        acc[2 * q] = floatx2{t.x, t.y}; acc[2 * q + 1] = floatx2{t.z, t.w};
      } else {
        acc[2 * q] += floatx2{t.x, t.y}; acc[2 * q + 1] += floatx2{t.z, t.w};
      }
    }
  };
  if (ACCUMULATE) group(0, IC<0>{}); else group(0, IC<1>{});
  if constexpr (C::NG * C::NQ <= 48) {
#pragma unroll
    for (int g = 1; g < C::NG; ++g) group(g, IC<0>{});
  } else {
    // large models: a rolled loop keeps the in-flight LDS reads (and registers) bounded
#pragma unroll 1
    for (int g = 1; g < C::NG; ++g) group(g, IC<0>{});
  }
#pragma unroll
  for (int q = 0; q < 2 * C::NQ; ++q) { x[2 * q] = acc[q][0]; x[2 * q + 1] = acc[q][1]; }
}

// ---------------------------------------------------------------------------
// Pooling (convRBM.py:245-267; Cfg::POOL > 1): the hidden units of POOL consecutive
// positions compete, P_i = exp(x_i) / (POOL + sum_j exp(x_j)), and at most one of them
// fires: unit i is on iff cum_{i-1} <= u < cum_i for the one uniform of the group
// (that of its first position).  A lane owns one position and evaluates its whole
// group itself (POOL gathers, two passes: maximum, then sums) -- plain and without
// cross-lane traffic; the reference calls pooling "not relevant for cRBM" and every
// BASELINE configuration uses POOL = 1, whose code never sees any of this.
//   zfun(pos, z): z[k] = -log2(e) * activation of the units at hidden position pos
// Results for the lane's position s: p = P_s, cb = sum of P over the group's earlier
// positions, S = sum of P over the group (all in the overflow-free form).
// ---------------------------------------------------------------------------
template <int POOL, int KP, class ZFun>
__device__ __forceinline__ void pooled_probs(ZFun zfun, int s, float (&p)[KP], float (&cb)[KP], float (&S)[KP]) {
  const int g0 = s - s % POOL, me = s - g0;
  float zmin[KP], z[KP];
#pragma unroll
  for (int k = 0; k < KP; ++k) zmin[k] = 0.f;               // the "POOL" term is POOL * exp(0)
#pragma unroll 1
  for (int j = 0; j < POOL; ++j) {
    zfun(g0 + j, z);
#pragma unroll
    for (int k = 0; k < KP; ++k) zmin[k] = fminf(zmin[k], z[k]);
  }
  float den[KP];
#pragma unroll
  for (int k = 0; k < KP; ++k) { den[k] = (float)POOL * __builtin_amdgcn_exp2f(zmin[k]); cb[k] = 0.f; p[k] = 0.f; }
#pragma unroll 1
  for (int j = 0; j < POOL; ++j) {
    zfun(g0 + j, z);
#pragma unroll
    for (int k = 0; k < KP; ++k) {
      const float e = __builtin_amdgcn_exp2f(zmin[k] - z[k]);   // exp(x_j - max), <= 1
      den[k] += e;
      cb[k] += j < me ? e : 0.f;
      p[k] = j == me ? e : p[k];
    }
  }
#pragma unroll
  for (int k = 0; k < KP; ++k) {
    const float inv = 1.0f / den[k];
    S[k] = (den[k] - (float)POOL * __builtin_amdgcn_exp2f(zmin[k])) * inv;
    p[k] *= inv;
    cb[k] *= inv;
  }
}

// 24-bit uniforms of the K units at (sequence n, position s): both 12-bit fields of every sampler
// group (the pooled sampler compares against cumulative sums, so the lazy fine call of
// sample_hidden does not apply)
template <class C>
__device__ __forceinline__ void hidden_uniforms24(uint32_t n, uint32_t s, uint32_t kind, uint32_t strand, const RngView& rng,
                                                  uint32_t step, float (&u)[C::KP], uint32_t group0 = 0) {
#pragma unroll
  for (int g = 0; g < C::NGRP; ++g) {
    const Philox4 rc = philox4x32(n, s, rng_word2(kind, strand, 0, group0 + (uint32_t)g), step, rng.seed_lo, rng.seed_hi);
    const Philox4 rf = philox4x32(n, s, rng_word2(kind, strand, 1, group0 + (uint32_t)g), step, rng.seed_lo, rng.seed_hi);
    auto unit = [&](auto I) {
      constexpr int i = decltype(I)::value;
      const int k = 10 * g + i;
      if (k < C::K) u[k] = (float)(philox_field12<i>(rc) * 4096u + philox_field12<i>(rf)) * 5.9604644775390625e-8f;
    };
    unit(IC<0>{}); unit(IC<1>{}); unit(IC<2>{}); unit(IC<3>{}); unit(IC<4>{});
    unit(IC<5>{}); unit(IC<6>{}); unit(IC<7>{}); unit(IC<8>{}); unit(IC<9>{});
  }
}

// sum_k log(1 + sum_j exp(x_j)) of the group that starts at position g0, per unit into acc[] (free energy,
// convRBM.py:664-665): ln2 * (-zmin) + ln(exp(-max) + sum_j exp(x_j - max))
template <int POOL, int KP, class ZFun>
__device__ __forceinline__ void pooled_softplus(ZFun zfun, int g0, float (&acc)[KP], int nvalid) {
  float zmin[KP], z[KP], den[KP];
#pragma unroll
  for (int k = 0; k < KP; ++k) zmin[k] = 0.f;
#pragma unroll 1
  for (int j = 0; j < POOL; ++j) {
    zfun(g0 + j, z);
#pragma unroll
    for (int k = 0; k < KP; ++k) zmin[k] = fminf(zmin[k], z[k]);
  }
#pragma unroll
  for (int k = 0; k < KP; ++k) den[k] = __builtin_amdgcn_exp2f(zmin[k]);
#pragma unroll 1
  for (int j = 0; j < POOL; ++j) {
    zfun(g0 + j, z);
#pragma unroll
    for (int k = 0; k < KP; ++k) den[k] += __builtin_amdgcn_exp2f(zmin[k] - z[k]);
  }
#pragma unroll
  for (int k = 0; k < KP; ++k)
    if (k < nvalid) acc[k] += 0.6931471805599453f * (__builtin_amdgcn_logf(den[k]) - zmin[k]);
}

// K-bit mask of the pooled sample at the lane's position: on iff cb <= u < cb + p (first index whose
// cumulative probability exceeds the group's uniform, convRBM.py:259-267)
template <class C>
__device__ __forceinline__ void pooled_sample(const float (&p)[C::KP], const float (&cb)[C::KP], const float (&u)[C::KP],
                                              uint32_t (&mask)[C::NW]) {
#pragma unroll
  for (int w = 0; w < C::NW; ++w) mask[w] = 0u;
#pragma unroll
  for (int k = 0; k < C::K; ++k) {
    const uint32_t one = (cb[k] + p[k] > u[k] && cb[k] <= u[k]) ? 1u : 0u;
    mask[k >> 5] |= one << (k & 31);
  }
}

// global precomputed tables -> LDS (plain float4 copy, one load in flight per thread: with a run-time stride and trip
// count, batching the loads of a thread measured slower).  stride: the threads of the block.
template <int NFLOATS>
__device__ __forceinline__ void copy_tables(float* dst, const float* src, uint32_t stride) {
  static_assert(NFLOATS % 4 == 0, "tables are float4 granular");
  const float4* s4 = reinterpret_cast<const float4*>(src);
  float4* d4 = reinterpret_cast<float4*>(dst);
  for (uint32_t i = threadIdx.x; i < (uint32_t)(NFLOATS / 4); i += stride) d4[i] = s4[i];
}
template <int NFLOATS>
__device__ __forceinline__ void copy_tables(float* dst, const float* src) { copy_tables<NFLOATS>(dst, src, blockDim.x); }
// Two tables, for a block of TB threads known at compile time (GeomCT): a thread's loads are all issued before its
// first LDS store -- together with whatever loads the caller has in flight, one memory round trip instead of one per
// 16 bytes -- in batches of at most CAP loads (4 * CAP registers; config #2: 4 + 1 loads, one batch).
template <int NA, int NB, int TB>
__device__ __forceinline__ void copy_tables_batched(float* dstA, const float* srcA, float* dstB, const float* srcB) {
  static_assert(NA % 4 == 0 && NB % 4 == 0, "tables are float4 granular");
  constexpr int A4 = NA / 4, B4 = NB / 4, RA = (A4 + TB - 1) / TB, RB = (B4 + TB - 1) / TB, R = RA + RB, CAP = 8;
  const float4 *sA = reinterpret_cast<const float4*>(srcA), *sB = reinterpret_cast<const float4*>(srcB);
  float4 *dA = reinterpret_cast<float4*>(dstA), *dB = reinterpret_cast<float4*>(dstB);
  // round j of the two tables back to back: rounds [0, RA) are the first table's.  In a ragged last round the threads
  // past the end copy the table's last element once more (the same 16 bytes to the same place): no branch around a
  // load or a store, so nothing keeps the compiler from issuing every load first.
#pragma unroll
  for (int j0 = 0; j0 < R; j0 += CAP) {
    float4 v[CAP];
    int at[CAP];
#pragma unroll
    for (int c = 0; c < CAP; ++c) {
      const int j = j0 + c, r = j < RA ? j : j - RA, n4 = j < RA ? A4 : B4, i = r * TB + (int)threadIdx.x;
      at[c] = (r + 1) * TB <= n4 ? i : min(i, n4 - 1);
      if (j < R) v[c] = (j < RA ? sA : sB)[at[c]];
    }
#pragma unroll
    for (int c = 0; c < CAP; ++c)
      if (j0 + c < R) (j0 + c < RA ? dA : dB)[at[c]] = v[c];
  }
}

// ---------------------------------------------------------------------------
// Tables, rebuilt whenever W, b or c change (set_params / apply_update):
//  Tf[g][r][k]  = -log2(e) * ( sum_{t<G, j=gG+t<M} W[k][(r>>2t)&3][j]  (+ b[k] in group 0) )
//    (ONE table: the reverse-complement strand, rc(W) = W[k][3-a][M-1-j] of convRBM.py:241, gathers from it
//     with the reverse-complemented letter window -- revcomp_window)
//    The gather therefore yields z = -x*log2(e), so exp(-x) is one v_exp_f32
//    (2^z) with no multiply; kernels that need x itself use x = -ln(2)*z.
//    Pad columns k >= K get +1e30 in group 0: exp(-x) = inf, sigmoid -> 0.
//  Tv[jr][ch][pat] (float4 over letters) = log2(e) * sum_{bit in pat} W[5ch+bit][:][M-1-jr]
//  Tvr          = same for rc(W)                           (convRBM.py:279-287)
//  Ws[jr+4][k]  (float4 over letters) = log2(e) * W[k][:][M-1-jr] for 0 <= jr < M, else 0   (sparse top-down)
//  Wsr          = same for rc(W)
//  c            = log2(e) * c
//    The top-down images carry log2(e) so that the softmax over the four letters is four v_exp_f32
//    (2^(y - max)) without a multiply each (sample_letter); free_energy_body, which wants c itself, multiplies back.
// ---------------------------------------------------------------------------
constexpr float LOG2E = 1.4426950408889634f, LN2 = 0.6931471805599453f;
struct TablesArgs {
  const float* W;   // (K,4,M)
  const float* b;   // (K)
  const float* c;   // (4)
  float* out;       // Cfg::TABLES_ALL floats
};

// entries first, first + stride, ... of the table images
// LIMIT: entries [0, LIMIT) only (Cfg::TAB: the gather table alone)
template <class C, int LIMIT = C::TABLES_ALL>
__device__ void build_tables_range(const TablesArgs& a, int first, int stride) {
  constexpr int K = C::K, M = C::M;
  for (int idx = first; idx < LIMIT; idx += stride) {
    float val = 0.f;
    if (idx < C::TAB) {                                      // gather table
      const int t0 = idx;
      const int k = t0 % C::KP, r = (t0 / C::KP) % C::ROWS, g = t0 / (C::KP * C::ROWS);
      if (k < K) {
        for (int t = 0; t < C::G; ++t) {
          const int j = g * C::G + t;
          if (j < M) {
            const int al = (r >> (2 * t)) & 3;
            val += a.W[(k * 4 + al) * M + j];
          }
        }
        if (g == 0) val += a.b[k];
        val *= -LOG2E;
      } else if (g == 0) {
        val = 1e30f;
      }
    } else if (idx < C::OFF_C) {                             // dense top-down tables
      const bool rc = C::DS && idx >= C::OFF_TVR;
      const int t0 = idx - (rc ? C::OFF_TVR : C::OFF_TV);
      const int al = t0 & 3, pat = (t0 >> 2) & 31, ch = (t0 >> 7) % C::NCH, jr = (t0 >> 7) / C::NCH;
      for (int bit = 0; bit < 5; ++bit) {
        const int k = 5 * ch + bit;
        if (k < K && ((pat >> bit) & 1))
          val += rc ? a.W[(k * 4 + (3 - al)) * M + jr] : a.W[(k * 4 + al) * M + (M - 1 - jr)];
      }
      val *= LOG2E;
    } else if (idx < C::TABLES) {
      val = LOG2E * a.c[idx - C::OFF_C];
    } else if (idx < C::OFF_C2) {                            // sparse top-down tables, zero rows at both ends
      const bool rc = C::DS && idx >= C::OFF_WSR;
      const int t0 = idx - (rc ? C::OFF_WSR : C::OFF_WS);
      const int al = t0 & 3, k = (t0 >> 2) % K, jr = (t0 >> 2) / K - 4;
      if (jr >= 0 && jr < M) val = LOG2E * (rc ? a.W[(k * 4 + (3 - al)) * M + jr] : a.W[(k * 4 + al) * M + (M - 1 - jr)]);
    } else {
      val = LOG2E * a.c[idx - C::OFF_C2];
    }
    a.out[idx] = val;
  }
}

template <class C>
__device__ void build_tables_body(const TablesArgs& a) {
  build_tables_range<C>(a, (int)(blockIdx.x * blockDim.x + threadIdx.x), (int)(gridDim.x * blockDim.x));
}
// the gather table of another letter grouping (plain chain launches of small models take larger groups than the
// fused training launch, whose LDS is shared with the statistics: crbm_api.hip, solo_group)
template <class C>
__device__ void build_gather_table_body(const TablesArgs& a) {
  build_tables_range<C, C::TAB>(a, (int)(blockIdx.x * blockDim.x + threadIdx.x), (int)(gridDim.x * blockDim.x));
}

// ---------------------------------------------------------------------------
// h_given_v, dense outputs: _bottomUpActivity / _bottomUpProbability /
// _bottomUpSample (convRBM.py:238-275) and motifHitProbs (:507-514).
// mode 0: forward strand, 1: reverse-complement strand, 2: sigma(x + x').
// ---------------------------------------------------------------------------
struct HgvArgs {
  const float* tables;
  const uint32_t* letters;
  int32_t n, L, Lh, LW;
  int32_t TS;          // sequences per tile
  FastDiv divLh;
  int32_t mode;
  float* act;
  float* prob;
  float* sample;
  unsigned long long* ones;   // += number of sampled ones (may be null)
  RngView rng;
  uint32_t kind;
};

// The kernel's model as a SLAB of a larger one (crbm_api.hip, slab_launch_hgv: h|v of a chain on the generic path): the
// sampled units go, as bits [k0, k0 + K) and below Kfull, into the larger model's mask rows (OR: the rows start at zero and
// slabs may overlap); group0 = k0 / 10 keeps every unit on its own counter (units draw in groups of ten).  Units below
// kskip are not counted in `ones`.  (A struct of its own: HgvArgs, and with it crbm_hgv, stay what they were.)
struct HgvMasksArgs {
  HgvArgs g;                  // act, prob, sample unused
  uint32_t* masks;            // [n][Lh][NWfull]
  int32_t NWfull, k0, Kfull, kskip;
  uint32_t group0;
};

template <class C>
__device__ void hgv_body(const HgvArgs& a) {
  constexpr int KP = C::KP, K = C::K, M = C::M;
  HIP_DYNAMIC_SHARED(float, smem);
  float* T0 = smem;
  copy_tables<C::TAB>(T0, a.tables + C::OFF_TF);
  __syncthreads();
  const bool want_sample = (a.sample != nullptr) || (a.ones != nullptr);
  const uint32_t strand = a.mode == 1 ? 1u : 0u;
  unsigned long long cnt = 0;
  const int ntiles = (a.n + a.TS - 1) / a.TS;
  for (int tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
    const int n0 = tile * a.TS;
    const int ns = min(a.TS, a.n - n0);
    const uint32_t items = (uint32_t)ns * (uint32_t)a.Lh;
    for (uint32_t i = threadIdx.x; i < items; i += blockDim.x) {
      const uint32_t nl = fastdiv(i, a.divLh);
      const int s = (int)(i - nl * (uint32_t)a.Lh);
      const int nn = n0 + (int)nl;
      const uint32_t* lrow = a.letters + (size_t)nn * a.LW;
      auto zfun = [&](int pos, float (&z)[KP]) {
        const LetterWin<M> w = letter_window<M>(lrow, pos);
        conv_gather<C>(T0, a.mode == 1 ? revcomp_window<M>(w) : w, z);
        if (a.mode == 2) conv_gather<C, true>(T0, revcomp_window<M>(w), z);
      };
      float x[KP];
      zfun(s, x);
      uint32_t mask[C::NW];
      float p[KP];
      if constexpr (C::POOL > 1) {
        float cb[KP], S[KP];
        pooled_probs<C::POOL, KP>(zfun, s, p, cb, S);
        if (want_sample) {
          float u[KP];
          hidden_uniforms24<C>(a.rng.seq_offset + (uint32_t)nn, (uint32_t)(s - s % C::POOL), a.kind, strand, a.rng, a.rng.step, u);
          pooled_sample<C>(p, cb, u, mask);
        }
      } else if (want_sample) {
        sample_hidden<C, 1>(x, a.rng.seq_offset + (uint32_t)nn, (uint32_t)s, a.kind, strand, a.rng, a.rng.step,
                               mask, p);
      } else {
#pragma unroll
        for (int k = 0; k < K; ++k) p[k] = sigmoid_z(x[k]);
      }
#pragma unroll
      for (int k = 0; k < K; ++k) {
        const size_t idx = ((size_t)nn * K + k) * a.Lh + s;
        if (a.act) a.act[idx] = x_of_z(x[k]);
        if (a.prob) a.prob[idx] = p[k];
        if (want_sample) {
          const uint32_t hb = (mask[k >> 5] >> (k & 31)) & 1u;
          if (a.sample) a.sample[idx] = (float)hb;
          cnt += hb;
        }
      }
    }
  }
  if (a.ones && cnt) atomicAdd(a.ones, cnt);
}

// The same pass for a SLAB of a larger model's chain (HgvArgs::masks; crbm_api.hip, slab_launch_hgv): the sample only, as bits
// of the larger model's mask rows.  A kernel of its own so that crbm_hgv stays the code it was (its register and scratch
// budget at 256 motifs is tight); compiled for models of up to 64 motifs only (crbm_jit.h).
template <class C>
__device__ void hgv_masks_body(const HgvMasksArgs& ma) {
  const HgvArgs& a = ma.g;
  constexpr int KP = C::KP, K = C::K, M = C::M;
  HIP_DYNAMIC_SHARED(float, smem);
  float* T0 = smem;
  copy_tables<C::TAB>(T0, a.tables + C::OFF_TF);
  __syncthreads();
  const uint32_t strand = a.mode == 1 ? 1u : 0u;
  unsigned long long cnt = 0;
  const int ntiles = (a.n + a.TS - 1) / a.TS;
  const int w0 = ma.k0 >> 5, sh = ma.k0 & 31;
  const int kend = min(K, ma.Kfull - ma.k0);          // local units that exist in the larger model
  for (int tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
    const int n0 = tile * a.TS;
    const int ns = min(a.TS, a.n - n0);
    const uint32_t items = (uint32_t)ns * (uint32_t)a.Lh;
    for (uint32_t i = threadIdx.x; i < items; i += blockDim.x) {
      const uint32_t nl = fastdiv(i, a.divLh);
      const int s = (int)(i - nl * (uint32_t)a.Lh);
      const int nn = n0 + (int)nl;
      const uint32_t* lrow = a.letters + (size_t)nn * a.LW;
      auto zfun = [&](int pos, float (&z)[KP]) {
        const LetterWin<M> w = letter_window<M>(lrow, pos);
        conv_gather<C>(T0, a.mode == 1 ? revcomp_window<M>(w) : w, z);
      };
      float x[KP];
      zfun(s, x);
      uint32_t mask[C::NW];
      float p[KP];
      if constexpr (C::POOL > 1) {
        float cb[KP], S[KP], u[KP];
        pooled_probs<C::POOL, KP>(zfun, s, p, cb, S);
        hidden_uniforms24<C>(a.rng.seq_offset + (uint32_t)nn, (uint32_t)(s - s % C::POOL), a.kind, strand, a.rng, a.rng.step, u, ma.group0);
        pooled_sample<C>(p, cb, u, mask);
      } else {
        sample_hidden<C, 0>(x, a.rng.seq_offset + (uint32_t)nn, (uint32_t)s, a.kind, strand, a.rng, a.rng.step, mask, p, nullptr, ma.group0);
      }
      // bits [k0, k0 + K) of the row's NWfull words, cut at Kfull (the last slab of a model may reach past its end);
      // units below kskip belong to the neighbouring slab as well and are counted there
      uint32_t* wp = ma.masks + ((size_t)nn * a.Lh + s) * ma.NWfull;
#pragma unroll
      for (int w = 0; w < C::NW; ++w) {
        const int lo = min(32, max(0, ma.kskip - 32 * w)), hi = min(32, max(0, kend - 32 * w));
        const uint32_t keep = hi >= 32 ? 0xFFFFFFFFu : (1u << hi) - 1u;
        const uint32_t counted = keep & (lo >= 32 ? 0u : ~((1u << lo) - 1u));
        mask[w] &= keep;
        cnt += (unsigned)__popc(mask[w] & counted);
      }
#pragma unroll
      for (int w = 0; w <= C::NW; ++w) {
        const uint32_t cur = w < C::NW ? mask[w < C::NW ? w : 0] : 0u, prev = w > 0 ? mask[w - 1] : 0u;
        const uint32_t bits = sh ? (cur << sh) | (prev >> (32 - sh)) : cur;
        if (bits && w0 + w < ma.NWfull) atomicOr(&wp[w0 + w], bits);      // (the slabs of a launch share words: slab_hgv_body)
      }
    }
  }
  if (a.ones && cnt) atomicAdd(a.ones, cnt);
}

// ===========================================================================
// Gradient statistics on the matrix cores.
//
// VH[k,a,j] = sum_{n,s} P[n,k,s] * [letter(n, s+j) == a]   (convRBM.py:327-337)
// is a K x (4*M) output contracted over N*Lh positions: a GEMM whose one operand
// (the unfolded one-hot) is exact in any float format and whose other operand, P,
// is split into two f16 halves (22 significant bits, products exact in f32).  One
// v_mfma_f32_16x16x32_f16 contracts 32 consecutive hidden positions of a chain:
//   A (16 x 32): row i = filter column j = 16*jt + i of letter a, element (i, t) =
//                2^-14 * [letter(s0 + t + j) == a] -- eight consecutive bits of the
//                letter's bit plane, expanded to eight f16 by one 16-byte LUT read;
//   B (32 x 16): column i = motif 16*nt + i of one column kind (P of the forward
//                strand, P' of the rc strand, Q = P(1-P) for the sparsity gradient,
//                convRBM.py:440-451), element (t, i) = 2^14 * P[k, s0 + t], read
//                from an LDS image the h|v pass writes transposed ([column][position]).
// The accumulators (one 16x16 f32 tile per letter x column tile x motif tile) stay in
// registers for the whole kernel; waves of a block are combined through LDS at the
// end and the block writes one partial row.  Against the letter-bucketed LDS walk of
// round 1 (one LDS read and one VALU add per (k, j, position); 42.5 us per half at
// config #2) the parked probabilities are read once instead of M
// times and the adds run on the matrix pipe beside the VALU work of other waves.
// north_star's "no MFMA" is about the convolution and its transpose (4-wide output,
// one-hot operand: gathers); this contraction is the one dense product on the path.
// ===========================================================================
struct StatsGeom {
  int32_t GPC;                                   // groups per chain
  int32_t off_slices, slice, off_win, off_gw, off_pt;   // LDS layout (floats): first slice, slice size, offsets inside a slice
  int32_t lds_floats;                            // dynamic LDS of the launch (the end-of-kernel combine uses all of it)
  FastDiv divGPC;
  int32_t row, off_vh0, off_vh1, off_h0, off_h1, off_sw, off_sb, off_v;
  float* partials;                               // [blocks of the statistics grid][row]
};

// kinds, motif tiles per wave, roles; mirrors stats_mfma_layout()
template <class C, bool SP>
struct StatsRole {
  static constexpr int KINDS = 1 + C::DS + (SP ? 1 : 0);
  static constexpr int NTW = stats_ntw(C::NT, C::JT, KINDS);
  static constexpr int NR = C::NT / NTW;
  static constexpr int KW = 16 * NTW < C::K ? 16 * NTW : C::K;
  // The sparsity columns Q = P(1-P) are not parked: the wave that reads a P fragment derives the Q fragment from
  // it in registers (same formula, same bits), so the column image holds the strands' P only -- half the rows
  // of a single-stranded data half, a third fewer LDS instructions.  (Pooled units need the sum over their
  // pooling group for Q: those are parked.)
  static constexpr bool QDERIVE = SP && C::POOL == 1;
  static constexpr int PARKED = KINDS - (QDERIVE ? 1 : 0);
  static constexpr int ROWS = PARKED * KW + 1;
  // Column tiles of the accumulators.  A wave that holds all motifs (NR == 1, so KW == K) has the parked kinds
  // back to back in its image, rows kind * K + k: the tiles then cut that list every 16 rows regardless of
  // where a kind ends (PACKED) -- 20 motifs on two strands are 40 columns = 3 tiles instead of 2 x 2.  The
  // derived sparsity tiles follow; each comes from the P fragment of the same tile index (columns of that
  // fragment that belong to the other strand give garbage nobody reads).
  static constexpr int NPT_PACKED = cdiv(PARKED * C::K, 16);
#ifdef CRBM_STATS_UNPACKED     // A/B knob (CRBM_JIT_DEFINES): whole tiles per kind everywhere
  static constexpr bool PACKED = false;
#else
  static constexpr bool PACKED = NR == 1 && NPT_PACKED < PARKED * NTW;
#endif
  static constexpr int NPT = PACKED ? NPT_PACKED : PARKED * NTW;        // tiles read from the image
  static constexpr int NCT = NPT + (QDERIVE ? NTW : 0);                 // + derived ones
  static constexpr int NACC = C::NL * C::JT * NCT;
  // tile and lane-in-tile of column `col` of kind `kind` (kind == KINDS - 1 with QDERIVE: the derived tiles)
  static constexpr int tile_of(int kind, int col) {
    return (QDERIVE && kind == KINDS - 1) ? NPT + col / 16 : PACKED ? (kind * C::K + col) / 16 : kind * NTW + col / 16;
  }
  static constexpr int lane_of(int kind, int col) {
    return (QDERIVE && kind == KINDS - 1) ? col % 16 : PACKED ? (kind * C::K + col) % 16 : col % 16;
  }
  static constexpr int THREADS = stats_mfma_threads(NR);
  static constexpr int NQW = 4 * NTW;            // float4 quads of motifs a wave gathers
};

// A-fragment look-up tables: bit e of the index set -> f16 2^-14 (0x0400), else 0.
//   nibble form: 16 entries of 8 bytes (four f16), two reads per fragment -- 128 bytes, for the Gibbs
//                kernel whose LDS is spoken for;
//   byte form:   256 entries of 16 bytes (eight f16), one read per fragment -- 4 KB, stand-alone kernel.
template <bool BYTE_LUT>
__device__ __forceinline__ void stats_build_lut(uint32_t* lut) {
  constexpr int WORDS = BYTE_LUT ? 1024 : 32, PER = BYTE_LUT ? 4 : 2;
  for (int i = threadIdx.x; i < WORDS; i += blockDim.x) {
    const uint32_t n = (uint32_t)i / PER, q = (uint32_t)i % PER;
    lut[i] = ((n >> (2 * q)) & 1u ? 0x0400u : 0u) | ((n >> (2 * q + 1)) & 1u ? 0x04000000u : 0u);
  }
}

// bit t of the result = [letter t of the packed word == a], t = 0..15
__device__ __forceinline__ uint32_t letter_plane16(uint32_t word, uint32_t a) {
  uint32_t x = word ^ (a * 0x55555555u);          // 00 where the letter is a
  x = ~(x | (x >> 1)) & 0x55555555u;
  x = (x | (x >> 1)) & 0x33333333u;
  x = (x | (x >> 2)) & 0x0F0F0F0Fu;
  x = (x | (x >> 4)) & 0x00FF00FFu;
  return (x | (x >> 8)) & 0xFFFFu;
}

// The letter windows of a unit (2 groups x 4 letters x NPW 16-bit pieces: 64 bits for M <= 32, 128
// beyond) are built by 8 NPW lanes: lane t owns letter (t & 3), letter word (t >> 2) % NPW (16
// positions) of group slot t / (4 NPW) and stores its 16 plane bits straight into the window
// (win as 16-bit pieces: piece index (slot*4 + letter)*NPW + word).
// Returns the number of its positions that count for the letter statistics: a group owns its 32
// positions (words 0, 1), the last group of a chain also the tail up to L (words 2 ..).
template <int NPW>
__device__ __forceinline__ float stats_window_piece(unsigned short* win16, int t, uint32_t word, bool group_valid, int gi, int GPC, int L) {
  const int a = t & 3, w = (t >> 2) % NPW, slot = t / (4 * NPW);
  const uint32_t bits = group_valid ? letter_plane16(word, (uint32_t)a) : 0u;
  win16[(slot * 4 + a) * NPW + w] = (unsigned short)bits;
  const int p0 = 32 * gi + 16 * w;                              // first position of this piece
  const int limit = (w < 2 || gi == GPC - 1) ? L : 0;           // positions >= limit do not count
  const int nbits = limit - p0 < 0 ? 0 : (limit - p0 > 16 ? 16 : limit - p0);
  return (float)__popc(bits & ((1u << nbits) - 1u));
}

// z[] = the gather of motif quads [q0, q0 + NQW) (clamped to the model's NQ); z = -log2(e) * activation
// ACCUMULATE: z[] (+)= the gather instead, every group added in turn (conv_gather's order: the same sums to the bit)
template <class C, int NQW, bool ACCUMULATE = false>
__device__ __forceinline__ void conv_gather_quads(const float* T, const LetterWin<C::M>& win, int q0, float (&z)[4 * NQW]) {
  if (!ACCUMULATE) {
#pragma unroll
    for (int i = 0; i < 4 * NQW; ++i) z[i] = 0.f;   // quads beyond the model's NQ
  }
  auto group = [&](int g, auto FIRST) {
    constexpr bool first = decltype(FIRST)::value != 0;   // the first group assigns
    const uint32_t r = window_bits<C::M>(win, 2 * C::G * g) & (uint32_t)(C::ROWS - 1);
    const float4* row = reinterpret_cast<const float4*>(T + (size_t)g * C::ROWS * C::KP) + (size_t)r * C::NQ + q0;
#pragma unroll
    for (int q = 0; q < NQW; ++q)
      if (q0 + q < C::NQ) {        // wave-uniform
        const float4 t = row[q];
        if (first) {
          z[4 * q + 0] = t.x; z[4 * q + 1] = t.y; z[4 * q + 2] = t.z; z[4 * q + 3] = t.w;
        } else {
          z[4 * q + 0] += t.x; z[4 * q + 1] += t.y; z[4 * q + 2] += t.z; z[4 * q + 3] += t.w;
        }
      }
  };
  if (ACCUMULATE) group(0, IC<0>{}); else group(0, IC<1>{});
  if constexpr (C::NG * NQW <= 48) {
#pragma unroll
    for (int g = 1; g < C::NG; ++g) group(g, IC<0>{});
  } else {
#pragma unroll 1
    for (int g = 1; g < C::NG; ++g) group(g, IC<0>{});
  }
}
// THE WINDOW CORE: z[] of motifs [4 q0, 4 q0 + 4 NQW) for window `w` on `strand` (1: its reverse complement).
// Single-stranded models score sigma(x + x') (convRBM.py:511-514): the other orientation is added on top, one strand.
// motif_sites_body, scan_sites_body and scan_hist_body all score through this one function: the same bits.
template <class C, int NQW>
__device__ __forceinline__ void window_strand_z(const float* Tf, const LetterWin<C::M>& w, int q0, int strand, float (&z)[4 * NQW]) {
  conv_gather_quads<C, NQW>(Tf, strand ? revcomp_window<C::M>(w) : w, q0, z);
  if (!C::DS) conv_gather_quads<C, NQW, true>(Tf, revcomp_window<C::M>(w), q0, z);
}

// One 32-position group (slot 0 or 1 of the wave's unit): all accumulator tiles of the wave.
//   Pt  : the wave's column image (row kind*KW + i, stride STATS_RS, position slot*32 + t)
//   win : the group's four letter windows (NPW/2 words each)
//   R   : the wave's role (StatsRole): column tiles read from the image (per kind, or cut from the kinds back to
//         back: PACKED) and, with QDERIVE, the tiles of the last kind (Q = P(1-P), sparsity), which are not in the
//         image but derived from the fragments of kind 0
template <class C, class R, bool BYTE_LUT>
__device__ __forceinline__ void stats_mfma_group(const float* Pt, const uint32_t* win, const uint32_t* lut, int nt0, int slot,
                                                 floatx4 (&acc)[R::NACC]) {
  constexpr int NTW = R::NTW, NCT = R::NCT, NPT = R::NPT, KW = R::KW, ZROW = R::PARKED * KW;
  const int lane = threadIdx.x & 63, i16 = lane & 15, g = lane >> 4;
  HalfFrag bhi[NCT], blo[NCT];
#pragma unroll
  for (int c = 0; c < NPT; ++c) {
    int row;
    if constexpr (R::PACKED) {
      row = 16 * c + i16 < R::PARKED * C::K ? 16 * c + i16 : ZROW;               // the kinds back to back; behind them the all-zero row
    } else {
      const int kind = c / NTW, t = c - kind * NTW, kl = 16 * t + i16;
      row = (16 * (nt0 + t) + i16 < C::K) ? kind * KW + kl : ZROW;              // motifs beyond K: the all-zero row
    }
    const float4* src = reinterpret_cast<const float4*>(Pt + (size_t)row * STATS_RS + slot * 32 + 8 * g);
    const float4 x0 = src[0], x1 = src[1];
    const float x[8] = {x0.x, x0.y, x0.z, x0.w, x1.x, x1.y, x1.z, x1.w};
    split_f16(x, bhi[c], blo[c]);
    if (R::QDERIVE && c < NTW) {          // kind 0 fills the first tiles in either layout
      float q[8];
#pragma unroll
      for (int e = 0; e < 8; ++e) q[e] = fmaf(-x[e] * STATS_PSCALE_INV, x[e], x[e]);   // 2^14 * P(1-P) from 2^14 * P
      split_f16(q, bhi[NPT + c], blo[NPT + c]);
    }
  }
  // the spare row (filter column M of letter 0, NL == 3): all ones -> sum over positions of P, i.e. H (crbm_layout.h, NL)
  const uint32_t ones_row = (C::NL == 3 && i16 == C::M % 16) ? 0x04000400u : 0u;
#pragma unroll
  for (int a = 0; a < C::NL; ++a) {
    unsigned long long bits = 0ull;
    if constexpr (C::NPW == 4) {
      const uint2 w = reinterpret_cast<const uint2*>(win)[a];
      bits = (unsigned long long)w.x | ((unsigned long long)w.y << 32);
    }
#pragma unroll
    for (int jt = 0; jt < C::JT; ++jt) {
      uint32_t byte;
      if constexpr (C::NPW == 4) byte = (uint32_t)(bits >> (8 * g + i16 + 16 * jt));
      else {
        // 128-bit window: the two words around bit 8 g + i16 + 16 jt (<= 87: word index <= 2), funnel-shifted
        const int sa = 8 * g + i16 + 16 * jt;
        const uint32_t* w32 = win + a * (C::NPW / 2) + (sa >> 5);
        const unsigned long long two = (unsigned long long)w32[0] | ((unsigned long long)w32[1] << 32);
        byte = (uint32_t)(two >> (sa & 31));
      }
      HalfFrag af;
      if constexpr (BYTE_LUT) {
        const uint4 f = reinterpret_cast<const uint4*>(lut)[byte & 255u];
        af.r[0] = f.x; af.r[1] = f.y; af.r[2] = f.z; af.r[3] = f.w;
      } else {
        const uint2 f0 = reinterpret_cast<const uint2*>(lut)[byte & 15u], f1 = reinterpret_cast<const uint2*>(lut)[(byte >> 4) & 15u];
        af.r[0] = f0.x; af.r[1] = f0.y; af.r[2] = f1.x; af.r[3] = f1.y;
      }
      if (C::NL == 3 && a == 0 && jt == C::JT - 1) {
#pragma unroll
        for (int e = 0; e < 4; ++e) af.r[e] |= ones_row;
      }
#pragma unroll
      for (int c = 0; c < NCT; ++c) {
        floatx4& d = acc[(a * C::JT + jt) * NCT + c];
        d = mfma_16x16x32_f16(af, bhi[c], d);
        d = mfma_16x16x32_f16(af, blo[c], d);
      }
    }
  }
}

// Combines the waves of a block and writes the block's partial row: vh / vh' / sw blocks, the H
// and sparsity-bias sums (filter column 0 pairs every hidden position with exactly one letter:
// sum_s P[k,s] = sum_a VH[k,a,0]; with NL == 3 the all-ones row gives H directly and the fourth letter is
// derived from it: crbm_layout.h) and the letter counts.  Kind by kind, every wave parks its
// accumulator tiles of that kind in a buffer of its own (as many waves at a time as the LDS
// holds: normally all), then every thread sums the copies of its output elements in wave order
// -- a barrier pair per kind instead of one per wave, and the same result for every launch
// geometry of a block.
// Uses the LDS of the block from its base on (everything is dead by now); all threads call it.
template <class C, bool SP>
__device__ __forceinline__ void stats_mfma_finish(const StatsGeom& sg, float* lds, int nt0, int block_row,
                                                  const floatx4 (&acc)[StatsRole<C, SP>::NACC], float vcount) {
  using R = StatsRole<C, SP>;
  constexpr int K = C::K, M = C::M, KAM = K * 4 * M, KINDS = R::KINDS, NTW = R::NTW, NR = R::NR, KW = R::KW;
  constexpr int PW = KW * 4 * M;                  // floats a wave parks per kind: [letter][column][motif of the role]
  const int nthr = blockDim.x, lane = threadIdx.x & 63, wave = threadIdx.x >> 6, nwaves = nthr >> 6;
  const int i16 = lane & 15, g = lane >> 4;
  float* total = lds;                   // [KAM], one kind at a time
  float* xch = lds + KAM;               // [nwaves][4]
  float* wbuf = xch + 64;
  int cw = min(nwaves, (sg.lds_floats - KAM - 64) / PW);   // waves parked at a time: whole sets of roles
  cw = max(NR, cw / NR * NR);
  float* out = sg.partials + (size_t)block_row * sg.row;
  __syncthreads();
#pragma unroll
  for (int kind = 0; kind < KINDS; ++kind) {
    for (int w0 = 0; w0 < nwaves; w0 += cw) {
      if (wave >= w0 && wave < w0 + cw) {
        float* mine = wbuf + (size_t)(wave - w0) * PW;
#pragma unroll
        for (int a = 0; a < C::NL; ++a)
#pragma unroll
          for (int jt = 0; jt < C::JT; ++jt)
#pragma unroll
            for (int c = R::tile_of(kind, 0); c <= R::tile_of(kind, KW - 1); ++c) {   // the tiles that hold columns of this kind
              // this lane's column of the tile, as a motif of the kind (negative or >= KW: another kind's or padding)
              const int kl = 16 * (c - R::tile_of(kind, 0)) + i16 - R::lane_of(kind, 0);
              const floatx4 d = acc[(a * C::JT + jt) * R::NCT + c];
#pragma unroll
              for (int r = 0; r < 4; ++r) {
                const int j = 16 * jt + 4 * g + r;
                const bool mine_k = kl >= 0 && kl < KW && 16 * nt0 + kl < K;
                if (j < M && mine_k) mine[(a * M + j) * KW + kl] = d[r];   // motif fastest: lanes of a tile row hit consecutive banks
                // the all-ones row: H, parked in the (unused) slot of letter 3, column 0
                if (C::NL == 3 && a == 0 && j == M && mine_k) mine[(3 * M) * KW + kl] = d[r];
              }
            }
      }
      __syncthreads();
      for (int e = threadIdx.x; e < (C::NL == 3 ? (3 * M + 1) * K : KAM); e += nthr) {   // e = (letter*M + column)*K + motif
        const int aj = e / K, k = e - aj * K;
        const int role = (k >> 4) / NTW, kl = k - 16 * NTW * role;
        const int o = k * 4 * M + aj;                                     // its place in the (K,4,M) output block
        float t = w0 == 0 ? 0.f : total[o];
        for (int w = w0 + role; w < min(nwaves, w0 + cw); w += NR)       // the waves of this motif's role, in wave order
          t += wbuf[(size_t)(w - w0) * PW + aj * KW + kl];
        total[o] = t;
      }
      __syncthreads();
    }
    // kinds: 0 = P (vh, h), 1 = P' when doublestranded (vh', h'), last = Q when SP (sw, sb)
    const int off_w = kind == 0 ? sg.off_vh0 : (C::DS && kind == 1) ? sg.off_vh1 : sg.off_sw;
    const int off_k = kind == 0 ? sg.off_h0 : (C::DS && kind == 1) ? sg.off_h1 : sg.off_sb;
    if constexpr (C::NL == 3) {
      // letter 3 from H (in its column-0 slot) and the three contracted letters
      for (int i = threadIdx.x; i < KAM; i += nthr) {
        const int k = i / (4 * M), aj = i - k * 4 * M;
        const float* tk = total + k * 4 * M;
        out[off_w + i] = aj < 3 * M ? tk[aj] : tk[3 * M] - ((tk[aj - 3 * M] + tk[aj - 2 * M]) + tk[aj - M]);
      }
      for (int k = threadIdx.x; k < K; k += nthr) out[off_k + k] = total[k * 4 * M + 3 * M];
    } else {
      for (int i = threadIdx.x; i < KAM; i += nthr) out[off_w + i] = total[i];
      for (int k = threadIdx.x; k < K; k += nthr)
        out[off_k + k] = (total[(k * 4) * M] + total[(k * 4 + 1) * M]) + (total[(k * 4 + 2) * M] + total[(k * 4 + 3) * M]);
    }
    // (the next kind's first barrier orders these reads before `total` is rewritten)
  }
  // letter counts: lane l counted letter (l & 3); lanes of one class -> wave -> block, fixed order
  const float cls = class_sum(vcount);
  if (lane < 4) xch[wave * 4 + lane] = cls;
  __syncthreads();
  if (threadIdx.x < 4) {
    float t = 0.f;
    for (int w = 0; w < nwaves; ++w) t += xch[w * 4 + threadIdx.x];
    out[sg.off_v + threadIdx.x] = t;
  }
}

struct StatsMfmaArgs {
  const float* tables;
  const uint32_t* letters;
  int32_t n, L, Lh, LW;
  int32_t off_tab;      // gather tables inside LDS (floats), after the slices
  int32_t debug;        // profiling only (results are wrong when set): 1 skips the MFMA steps, 2 the h|v arithmetic, 4 the
                        // staging, 8 the combine + output, 16 the table copy, 32 the whole loop
  int32_t nblocks;      // blocks of the statistics grid (0: the whole launch)
  StatsGeom sg;
};

// Stand-alone statistics of (letters, n, L): the data half of a training step (SP: with the
// sparsity columns) and the model half of models whose accumulator set is too large to ride
// in the Gibbs kernel.  A wave loops over units of two groups: lanes 0-7 stage the groups'
// letter words (fetched one unit ahead) and build the letter windows, every lane computes P of
// one hidden position for the wave's motifs and parks it transposed, then the MFMA steps run.
template <class C, bool SP, bool BYTE_LUT = true>
__device__ void stats_mfma_body(const StatsMfmaArgs& a, int bid = -1) {   // bid: block of the statistics grid (default: blockIdx.x)
  using R = StatsRole<C, SP>;
  constexpr int K = C::K, M = C::M, NTW = R::NTW, NR = R::NR, KW = R::KW;
  HIP_DYNAMIC_SHARED(float, smem);
  const StatsGeom& sg = a.sg;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, nwaves = blockDim.x >> 6;
  uint32_t* lut = reinterpret_cast<uint32_t*>(smem);
  float* slice = smem + sg.off_slices + (size_t)wave * sg.slice;
  constexpr int NPW = C::NPW;
  uint32_t* win = reinterpret_cast<uint32_t*>(slice + sg.off_win);
  uint32_t* gw = reinterpret_cast<uint32_t*>(slice + sg.off_gw);
  float* Pt = slice + sg.off_pt;
  float* Tf = smem + a.off_tab;
  if (!(a.debug & 16)) {
    copy_tables<C::TAB>(Tf, a.tables + C::OFF_TF);
    stats_build_lut<BYTE_LUT>(lut);
    for (int i = lane; i < R::ROWS * STATS_RS; i += 64) Pt[i] = 0.f;   // the zero row (and the pad columns) stay zero
  }
  __syncthreads();

  const int role = wave % NR, wave_in_role = wave / NR, waves_per_role = nwaves / NR;
  const int nt0 = role * NTW;
  floatx4 acc[R::NACC];
#pragma unroll
  for (int t = 0; t < R::NACC; ++t) acc[t] = floatx4{0.f, 0.f, 0.f, 0.f};
  float vcount = 0.f;                                  // letter (lane & 3), lanes 0-7 of role-0 waves

  const int GPC = sg.GPC;
  const int ngroups = a.n * GPC;                       // the host keeps n * GPC below 2^31
  const int nunits = (ngroups + 1) / 2;
  if (bid < 0) bid = (int)blockIdx.x;
  const int nblk = a.nblocks > 0 ? a.nblocks : (int)gridDim.x;
  const int ustride = nblk * waves_per_role;
  // letter words of a unit: lane t < 8 NPW fetches word (t >> 2) % NPW of group slot t / (4 NPW) (four lanes,
  // one per letter, fetch the same word: one transaction) and later turns it into its window piece
  unsigned short* win16 = reinterpret_cast<unsigned short*>(win);
  auto fetch_word = [&](int u) -> uint32_t {
    if (lane >= 8 * NPW || u >= nunits) return 0u;
    const int G = 2 * u + lane / (4 * NPW);
    if (G >= ngroups) return 0u;
    const uint32_t chain = fastdiv((uint32_t)G, sg.divGPC);
    const int w = 2 * (G - (int)chain * GPC) + (lane >> 2) % NPW;
    return w < a.LW ? a.letters[(size_t)chain * a.LW + w] : 0u;
  };
  int u = bid * waves_per_role + wave_in_role;
  if (a.debug & 32) u = nunits;
  uint32_t pre = fetch_word(u);
  for (; u < nunits; u += ustride) {
    const int G0 = 2 * u;
    if (lane < 8 * NPW && !(a.debug & 4)) {
      const int G = G0 + lane / (4 * NPW);
      int gi = 0;
      if (G < ngroups) gi = G - (int)fastdiv((uint32_t)G, sg.divGPC) * GPC;
      if ((lane & 3) == 0) gw[lane >> 2] = pre;        // the packed words themselves feed the h|v gather below
      const float cnt = stats_window_piece<NPW>(win16, lane, pre, G < ngroups, gi, GPC, a.L);
      if (role == 0) vcount += cnt;
    }
    __builtin_amdgcn_wave_barrier();
    pre = fetch_word(u + ustride);                     // in flight during this unit
    // ---- P (and P', Q) of this lane's hidden position for the wave's motifs, parked transposed ----
    {
      const int slot = lane >> 5, e = lane & 31;
      const int G = G0 + slot;
      bool valid = G < ngroups && !(a.debug & 2);
      uint32_t chain = 0u;
      int s = 0;
      if (valid) {
        chain = fastdiv((uint32_t)G, sg.divGPC);
        s = 32 * (G - (int)chain * GPC) + e;
        valid = s < a.Lh;
      }
      float* col = Pt + lane;
      if constexpr (C::POOL > 1) {
        // pooled units: the lane evaluates its whole pooling group (it may reach back over the staged
        // window: letters come from the global row); Q = dP_group/dx_s = P_s (1 - sum of the group's P)
        if (valid) {
          const uint32_t* lrow = a.letters + (size_t)chain * a.LW;
          constexpr int NV = 4 * R::NQW;
          float p[NV], cb[NV], S[NV];
#pragma unroll
          for (int strand = 0; strand <= C::DS; ++strand) {
            auto zfun = [&](int pos, float (&z)[NV]) {
              const LetterWin<M> w = letter_window<M>(lrow, pos);
              conv_gather_quads<C, R::NQW>(Tf, strand ? revcomp_window<M>(w) : w, 4 * nt0, z);
            };
            pooled_probs<C::POOL, NV>(zfun, s, p, cb, S);
#pragma unroll
            for (int kl = 0; kl < KW; ++kl)
              if (16 * nt0 + kl < K) {
                const float ps = 16384.0f * p[kl];
                col[(size_t)(strand * KW + kl) * STATS_RS] = ps;
                if (SP && strand == 0) col[(size_t)((1 + C::DS) * KW + kl) * STATS_RS] = ps * (1.0f - S[kl]);
              }
          }
        } else {
#pragma unroll
          for (int r = 0; r < R::PARKED * KW; ++r) col[(size_t)r * STATS_RS] = 0.f;
        }
      } else
      if (valid) {
        const LetterWin<M> wl = letter_window<M>(gw + NPW * slot, e);
        float z[4 * R::NQW];
        conv_gather_quads<C, R::NQW>(Tf, wl, 4 * nt0, z);
#pragma unroll
        for (int kl = 0; kl < KW; ++kl)
          if (16 * nt0 + kl < K) {                     // wave-uniform
            const float ps = fast_rcp(fmaf(exp_neg_x(z[kl]), STATS_PSCALE_INV, STATS_PSCALE_INV));   // 2^14 * sigma(x)
            col[(size_t)kl * STATS_RS] = ps;
            if (SP && !R::QDERIVE) col[(size_t)((1 + C::DS) * KW + kl) * STATS_RS] = fmaf(-ps * STATS_PSCALE_INV, ps, ps);   // 2^14 * P(1-P)
          }
        if (C::DS) {
          conv_gather_quads<C, R::NQW>(Tf, revcomp_window<M>(wl), 4 * nt0, z);
#pragma unroll
          for (int kl = 0; kl < KW; ++kl)
            if (16 * nt0 + kl < K)
              col[(size_t)(KW + kl) * STATS_RS] = fast_rcp(fmaf(exp_neg_x(z[kl]), STATS_PSCALE_INV, STATS_PSCALE_INV));
        }
      } else {
#pragma unroll
        for (int r = 0; r < R::PARKED * KW; ++r) col[(size_t)r * STATS_RS] = 0.f;
      }
    }
    __builtin_amdgcn_wave_barrier();
    // ---- the MFMA steps of the unit ----
#pragma unroll
    for (int slot = 0; slot < 2; ++slot)
      if (G0 + slot < ngroups && !(a.debug & 1))
        stats_mfma_group<C, R, BYTE_LUT>(Pt, win + 2 * NPW * slot, lut, nt0, slot, acc);
    __builtin_amdgcn_wave_barrier();                   // the slice is rewritten by the next unit
  }
  if (a.debug & 8) return;
  stats_mfma_finish<C, SP>(sg, smem, nt0, bid, acc, vcount);
}

// ---------------------------------------------------------------------------
// The persistent-chain kernel: `steps` Gibbs steps
//   v ~ P(v|h,h')  (convRBM.py:317-325)   then   h,h' ~ P(h|v)  (:269-275)
// for every chain of a tile, entirely in LDS (convRBM.py:397-408).
// ---------------------------------------------------------------------------
struct GibbsArgs {
  const float* tables;    // the model's table images (crbm_layout.h)
  const float* tables_tf = nullptr;   // sparse variant: the gather table of THIS kernel's letter grouping when it is not the
  int32_t off_ws = 0;                 // model's (then the top-down tables start at tables + off_ws); null: tables, Cfg::OFF_WS
  uint32_t* hm;        // [nchains][Lf][NW] in/out
  uint32_t* hmp;       // reverse strand (ds) or null
  uint32_t* vout;      // [nchains][LWs] letters of the last visible sample
  int32_t nchains, Lf, Lv, S;
  int32_t nvb, nhb;    // items per chain: 4-position visible blocks, hidden positions
  int32_t Lrow;        // padded mask row (positions), multiple of 4
  int32_t LWs;         // letter words per chain row
  FastDiv divVB, divHB, divRow, divLfw;   // / nvb, / nhb, / (Lrow*NW), / (Lf*NW)
  int32_t steps;
  RngView rng;
  uint32_t* ones;      // [gridDim.x * waves per block] set bits of the final hidden state per wave (activity monitor), may be null
  unsigned long long* clock = nullptr;   // null, or {sum of wall ticks, sum of shader cycles, scratch, scratch}: block 0 adds the duration of
                               // this launch in both clocks (their ratio is the shader clock WHILE the kernel ran: crbm_time_gibbs)
  unsigned long long* timeline = nullptr;   // measurement aid: null, or two words: block 0's first and last wall-clock tick of this launch
  int32_t debug;       // profiling only: 1 skips the table copy, 2 the state load, 4 the state store
  // STATS variant only: the model half of the gradient statistics rides in the last h|v pass
  int32_t nblocks;     // blocks [0, nblocks) of the launch run the chain (0: the whole grid)
  int32_t stats_off;   // statistics region inside LDS (floats, 16-byte aligned), after the chain image
  StatsGeom sg;        // divGPC divides group indices of one tile
};

// The geometry of a chain launch as gibbs_body sees it.  GeomRT reads it from the arguments (FastDiv records for the
// index divisions), serves any launch and carries the profiling aids (debug, clock, timeline).  GeomCT has the geometry
// of ONE launch shape compiled in (crbm_jit.h, jit_geo_stub; the host picks it only for a launch of exactly this shape:
// crbm_plan.h, GeoSpec): divisions by constants, one state-load path, constant trip counts, a single tile per block
// where the grid covers every tile, and nothing of the profiling aids.  Every tile of a GeomCT launch is full
// (NCHAINS % S == 0).  Both forms compute the same bits: the geometry decides where a word lives, never its value.
struct GeomRT {
  static constexpr bool CT = false, PROF = true, ALIGNED = false, ONE = false, WHOLE_BYTES = false;
  static constexpr int TB = 0;                          // the block size is the launch's
  const GibbsArgs& a;
  __device__ __forceinline__ explicit GeomRT(const GibbsArgs& a_) : a(a_) {}
  __device__ __forceinline__ int S() const { return a.S; }
  __device__ __forceinline__ int Lf() const { return a.Lf; }
  __device__ __forceinline__ int Lv() const { return a.Lv; }
  __device__ __forceinline__ int Lrow() const { return a.Lrow; }
  __device__ __forceinline__ int LWs() const { return a.LWs; }
  __device__ __forceinline__ int nvb() const { return a.nvb; }
  __device__ __forceinline__ int nhb() const { return a.nhb; }
  __device__ __forceinline__ int nchains() const { return a.nchains; }
  __device__ __forceinline__ uint32_t threads() const { return blockDim.x; }
  __device__ __forceinline__ int nblk() const { return a.nblocks > 0 ? a.nblocks : (int)gridDim.x; }
  __device__ __forceinline__ uint32_t div_vb(uint32_t i) const { return fastdiv_tile(i, a.divVB); }
  __device__ __forceinline__ uint32_t div_hb(uint32_t i) const { return fastdiv_tile(i, a.divHB); }
  template <int NW> __device__ __forceinline__ uint32_t div_lfw(uint32_t i) const { return fastdiv_tile(i, a.divLfw); }
};
template <int S_, int LF_, int LV_, int LROW_, int LWS_, int NVB_, int NHB_, int TB_, int NCHAINS_, int GRID_, bool ALIGNED_>
struct GeomCT {
  static_assert(S_ >= 1 && NCHAINS_ % S_ == 0 && GRID_ >= 1 && GRID_ <= NCHAINS_ / S_ && TB_ % 64 == 0, "GeomCT: full tiles only");
  static constexpr bool CT = true, PROF = false, ALIGNED = ALIGNED_, ONE = GRID_ == NCHAINS_ / S_;
  static constexpr bool WHOLE_BYTES = LV_ % 4 == 0;     // every letter byte of a visible row holds four positions
  static constexpr int TB = TB_;
  __device__ __forceinline__ explicit GeomCT(const GibbsArgs&) {}
  __device__ __forceinline__ constexpr int S() const { return S_; }
  __device__ __forceinline__ constexpr int Lf() const { return LF_; }
  __device__ __forceinline__ constexpr int Lv() const { return LV_; }
  __device__ __forceinline__ constexpr int Lrow() const { return LROW_; }
  __device__ __forceinline__ constexpr int LWs() const { return LWS_; }
  __device__ __forceinline__ constexpr int nvb() const { return NVB_; }
  __device__ __forceinline__ constexpr int nhb() const { return NHB_; }
  __device__ __forceinline__ constexpr int nchains() const { return NCHAINS_; }
  __device__ __forceinline__ constexpr uint32_t threads() const { return TB_; }
  __device__ __forceinline__ constexpr int nblk() const { return GRID_; }
  __device__ __forceinline__ uint32_t div_vb(uint32_t i) const { return i / (uint32_t)NVB_; }
  __device__ __forceinline__ uint32_t div_hb(uint32_t i) const { return i / (uint32_t)NHB_; }
  template <int NW> __device__ __forceinline__ uint32_t div_lfw(uint32_t i) const { return i / (uint32_t)(LF_ * NW); }
};

// letter of one visible position from its 4 top-down activations, given in units of log 2 (the tables carry log2(e))
// The letter is (t >= a) + (t >= b) + (t >= c) with t = u * sum(e) and the thresholds a = e0, b = e0 + e1, c = b + e2.
// The thresholds ascend (every e >= 0, rounding is monotone), and t - x has exactly the sign of the comparison (a
// difference of two floats never rounds to zero; t == x gives +0, which counts as t >= x).  With sa, sb, sc the sign
// bits of t - a, t - b, t - c (sa => sb => sc), bit 1 of the letter is ~sb and bit 0 is ~(sa ^ sb ^ sc): one subtraction
// per threshold and one v_bitop3 where compares, selects and adds took eight instructions and their wait states.
// push_letter shifts the two bits INVERTED into acc (bit 1 first: v_alignbit, shift_in_sign), so that after the letters
// of positions 3, 2, 1, 0 the low byte of ~acc is the packed letter byte of the four positions.
// (The activations are finite sums of finite table entries: no NaN reaches a sign.)
__device__ __forceinline__ uint32_t push_letter(uint32_t acc, float y0, float y1, float y2, float y3, float u) {
  const float mx = max4_finite(y0, y1, y2, y3);
  const float e0 = __builtin_amdgcn_exp2f(y0 - mx), e1 = __builtin_amdgcn_exp2f(y1 - mx), e2 = __builtin_amdgcn_exp2f(y2 - mx),
              e3 = __builtin_amdgcn_exp2f(y3 - mx);
  const float t = u * ((e0 + e1) + (e2 + e3));
  const float da = t - e0, db = t - (e0 + e1), dc = t - ((e0 + e1) + e2);
  acc = shift_in_sign(acc, db);
  return (acc << 1) | (xor3(__float_as_uint(da), __float_as_uint(db), __float_as_uint(dc)) >> 31);
}
__device__ __forceinline__ uint32_t sample_letter(float y0, float y1, float y2, float y3, float u) {
  return ~push_letter(0u, y0, y1, y2, y3, u) & 3u;
}
// the letter byte of the four positions p0 .. p0+3 of a visible row of Lv positions (p0 < Lv; letters beyond the row are 0):
// `inv` holds their inverted bits as push_letter left them, position 3 pushed first.  FULL: Lv % 4 == 0, every byte is whole.
template <bool FULL>
__device__ __forceinline__ uint32_t letter_byte(uint32_t inv, int p0, int Lv) {
  if constexpr (FULL) return ~inv & 0xFFu;
  else return ~inv & (0xFFu >> (2 * max(0, 4 - (Lv - p0))));
}

// The first n of the masks m[T .. N) of K bits each join the two halves of a 64-bit window word, mask t at bit t*K,
// in 32-bit shift-ors (lo and hi start at 0).  A mask that straddles bit 32 gives its low part to one half and the
// rest to the other; it is the first piece of the upper half, as the mask at bit 32 is where none straddles.
template <int K, int T, int N>
__device__ __forceinline__ void pack_masks(const uint32_t* m, int n, uint32_t& lo, uint32_t& hi) {
  if constexpr (T < N) {
    constexpr int o = T * K;
    if (T < n) {
      if constexpr (o == 0) lo = m[T];
      else if constexpr (o < 32) lo = shl_or<o % 32>(m[T], lo);
      if constexpr (o < 32 && o + K > 32) hi = m[T] >> ((32 - o) % 32);
      else if constexpr (o == 32) hi = m[T];
      else if constexpr (o > 32) hi = shl_or<(o - 32) % 32>(m[T], hi);
    }
    pack_masks<K, T + 1, N>(m, n, lo, hi);
  }
}

// Adds the top-down contributions of every set bit of one window word to the 4
// visible positions of a thread.  Bit b of the word is hidden unit k of window slot
// q = q_base + ql (b = ql*K + k); visible position i sees it through filter column
// jr = q - i, i.e. table row (q - i + 4): address (q_base*K + b)*16 + (4 - i)*K*16,
// out-of-range columns hit the zero rows of the table.  The rows of the next bit are
// requested before those of the current one are added (the LDS latency of a set
// bit overlaps the adds of the previous one); a lane that runs out of bits points
// at the leading zero rows.
// unit_base: hidden unit of bit 0 (models with more than 64 motifs walk a mask in several words).
template <class C>
__device__ __forceinline__ void topdown_bits(unsigned long long w, const char* tab, int q_base, float (&y)[4][4], int unit_base = 0) {
  constexpr int K = C::K;
  const char* tab_q = tab + ((size_t)q_base * K + unit_base) * 16;
  const char* idle = tab - K * 16;                     // + (4-i)*K*16 = rows 3-i: all zero
  auto rows_of = [&](unsigned long long bits) { return bits ? tab_q + (__ffsll(bits) - 1) * 16 : idle; };
  auto fetch = [&](const char* p, float4 (&t)[4]) {
#pragma unroll
    for (int i = 0; i < 4; ++i) t[i] = *reinterpret_cast<const float4*>(p + (4 - i) * K * 16);
  };
  float4 cur[4];
  fetch(rows_of(w), cur);
  while (w) {
    w &= w - 1ull;
    float4 nxt[4];
    fetch(rows_of(w), nxt);
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      y[i][0] += cur[i].x; y[i][1] += cur[i].y; y[i][2] += cur[i].z; y[i][3] += cur[i].w;
      cur[i] = nxt[i];
    }
  }
}

// SPARSE selects the top-down variant (Cfg comment in crbm_layout.h); the LDS image
// differs accordingly.  The dense variant exists only for Cfg::DENSE models.
// STATS: the last h|v pass also produces the model half of the gradient statistics
// (convRBM.py:411-413: last-step probabilities, last-step visible sample): the pass runs
// in wave units of two 32-position groups, every lane parks the probabilities it has in
// registers anyway in the wave's LDS slice, and the wave contracts them with the visible
// sample (still in LDS) on the matrix cores -- no second read of v, no recomputation of P.
// GP: the geometry policy (GeomRT: any launch; GeomCT: one launch shape, compiled in).
template <class C, bool SPARSE, bool STATS = false, class GP = GeomRT>
__device__ void gibbs_body(const GibbsArgs& a, int bid = -1) {   // bid: block of the chain grid (default: blockIdx.x)
  const GP g(a);
  const int dbg = GP::PROF ? a.debug : 0;              // profiling only (GibbsArgs::debug)
  const uint32_t TB = g.threads();
  constexpr int KP = C::KP, M = C::M, NW = C::NW, NCH = C::NCH;
  static_assert(SPARSE || C::DENSE, "no dense top-down tables for this model");
  using SR = StatsRole<C, false>;
  static_assert(!STATS || SR::NR == 1, "the fused statistics need all motifs of a position in one wave");
  constexpr int LTAB = SPARSE ? C::SP_TABLES : C::TABLES;
  HIP_DYNAMIC_SHARED(float, smem);
  const float* Tf = smem;
  const float* cv = smem + (SPARSE ? C::SP_C : C::OFF_C);
  uint32_t* hm = reinterpret_cast<uint32_t*>(smem + LTAB);
  uint32_t* hmp = hm + (size_t)g.S() * g.Lrow() * NW;
  uint32_t* let = hmp + (C::DS ? (size_t)g.S() * g.Lrow() * NW : 0);
  uint32_t* fixq = let + (size_t)g.S() * g.LWs();   // [count][-][FIXQ_CAP entries]: undecided units of the running h|v pass
#ifdef CRBM_INLINE_EXACT_PATH                     // A/B knob (CRBM_JIT_DEFINES): every wave resolves its own undecided units
  constexpr bool DEFER = false;
#else
  // Measured: double-stranded models gain (config #5: 180 -> 155 us per step), single-stranded
  // ones lose to the extra barrier and the serial drain (config #2: 16.9 -> 17.5 us per step; with the
  // 1024-thread blocks of round 3 21.7 -> 22.1 us per one-step launch, config #4 2.273 -> 2.279 ms).  Pooled
  // models draw both fields for every group anyway.
  constexpr bool DEFER = C::POOL == 1 && C::DS;
#endif

  // The tables are copied while the state loads of the block's first tile are in flight (below).  GeomCT with one tile per
  // block: the table loads join them -- every global load of the prologue is issued before the thread's first wait and
  // first LDS store.
  bool tables_done = (dbg & 1) != 0;
  auto copy_all_tables = [&]() {
    if (SPARSE) {
      const float* tf = a.tables_tf ? a.tables_tf : a.tables;
      const float* ws = a.tables + (a.tables_tf ? a.off_ws : C::OFF_WS);
      // (only where a block has ONE tile -- the prologue is then paid per tile, per step in one-step launches: config #2
      //  14.74 against 15.03 us per step.  A block that loops over tiles copies its tables once for many tiles, and
      //  config #4 measured 7 % SLOWER with the batch, 2.12 against 1.98 ms per five-step launch: DESIGN 6)
      if constexpr (GP::CT && GP::ONE) {
        copy_tables_batched<C::TAB, C::WS * (1 + C::DS) + 4, GP::CT ? GP::TB : 64>(smem, tf, smem + C::SP_WS, ws);
      } else {
        copy_tables<C::TAB>(smem, tf, TB);
        copy_tables<C::WS * (1 + C::DS) + 4>(smem + C::SP_WS, ws, TB);
      }
    } else {
      copy_tables<C::TABLES>(smem, a.tables, TB);
    }
    tables_done = true;
  };

  const int rowW = g.Lrow() * NW;
  const uint32_t per = (uint32_t)(g.Lf() * NW);           // state words per chain
  const int ntiles = (g.nchains() + g.S() - 1) / g.S();
  if (bid < 0) bid = (int)blockIdx.x;
  if constexpr (GP::PROF) {
    if (a.clock && bid == 0 && threadIdx.x == 0) {      // both clocks at the start of the launch, parked in memory (no live registers)
      a.clock[2] = realtime_ticks();
      a.clock[3] = shader_cycles();
    }
    if (a.timeline && bid == 0 && threadIdx.x == 0) a.timeline[0] = realtime_ticks();
  }
  const int nblk = g.nblk();
  int nset = 0;
  // statistics state (STATS): the wave's LDS slice, accumulator tiles, letter counts
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, nwaves = TB >> 6;
  float* sreg = nullptr;
  uint32_t* swin = nullptr;
  float* sPt = nullptr;
  floatx4 sacc[STATS ? SR::NACC : 1];
  float vcount = 0.f;
  if constexpr (STATS) {
    sreg = smem + a.stats_off;
    float* sslice = sreg + a.sg.off_slices + (size_t)wave * a.sg.slice;
    swin = reinterpret_cast<uint32_t*>(sslice + a.sg.off_win);
    sPt = sslice + a.sg.off_pt;
#pragma unroll
    for (int t = 0; t < SR::NACC; ++t) sacc[t] = floatx4{0.f, 0.f, 0.f, 0.f};
    stats_build_lut<false>(reinterpret_cast<uint32_t*>(sreg));
    for (int i = lane; i < SR::ROWS * STATS_RS; i += 64) sPt[i] = 0.f;   // the zero row stays zero
  }
  if (threadIdx.x == 0) fixq[0] = 0u;
  // the pads of the mask rows (M-1 positions in front, the rest behind) stay zero for the whole kernel
  {
    const int padw = rowW - (int)per, front = (M - 1) * NW;
    for (int idx = threadIdx.x; idx < g.S() * padw; idx += TB) {
      const int nl = idx / padw, e = idx - nl * padw;
      const int d = nl * rowW + (e < front ? e : e + (int)per);
      hm[d] = 0u;
      if (C::DS) hmp[d] = 0u;
    }
  }
  // (GeomCT: every tile is full; where the grid covers all tiles the loop is one iteration without a test)
  for (int tile = bid; GP::ONE ? tile == bid : tile < ntiles; tile += nblk) {
    const int n0 = tile * g.S();
    const int ns = GP::CT ? g.S() : min(g.S(), g.nchains() - n0);
    __syncthreads();
    // chain state -> zero-padded LDS rows (hidden position s sits at s + M-1).  The
    // chains of a tile are one contiguous range of ns*per words in global memory:
    // all loads of a thread are issued before the first LDS store (one memory round
    // trip per tile), 16 bytes per lane where the alignment allows.
    if (!(dbg & 2)) {
      const uint32_t nwords = (uint32_t)ns * per;
      auto lds_index = [&](uint32_t i) {           // word i of the tile -> padded row position
        const uint32_t nl = g.template div_lfw<NW>(i);
        return nl * (uint32_t)rowW + (uint32_t)((M - 1) * NW) + (i - nl * per);
      };
      const size_t g0 = (size_t)n0 * per;
      if (GP::CT ? GP::ALIGNED : ((g0 | nwords) & 3u) == 0u) {
        constexpr int UN = 2;
        const uint4* src = reinterpret_cast<const uint4*>(a.hm + g0);
        const uint4* srcp = C::DS ? reinterpret_cast<const uint4*>(a.hmp + g0) : nullptr;
        for (uint32_t base0 = 0; base0 < nwords / 4; base0 += UN * TB) {   // the same rounds for every thread
          const uint32_t base = base0 + threadIdx.x;
          uint4 t[UN], tp[UN];
#pragma unroll
          for (int u = 0; u < UN; ++u) {
            const uint32_t i4 = base + u * TB;
            if (i4 < nwords / 4) {
              t[u] = src[i4];
              if (C::DS) tp[u] = srcp[i4];
            }
          }
          if (!tables_done) copy_all_tables();
#pragma unroll
          for (int u = 0; u < UN; ++u) {
            const uint32_t i4 = base + u * TB;
            if (i4 < nwords / 4) {
              const uint32_t e[4] = {t[u].x, t[u].y, t[u].z, t[u].w};
              const uint32_t ep[4] = {tp[u].x, tp[u].y, tp[u].z, tp[u].w};
#pragma unroll
              for (int c = 0; c < 4; ++c) {
                const uint32_t d = lds_index(4 * i4 + c);
                hm[d] = e[c];
                if (C::DS) hmp[d] = ep[c];
              }
            }
          }
        }
      } else {
        constexpr int UN = 8;
        for (uint32_t base0 = 0; base0 < nwords; base0 += UN * TB) {
          const uint32_t base = base0 + threadIdx.x;
          uint32_t t[UN], tp[UN];
#pragma unroll
          for (int u = 0; u < UN; ++u) {
            const uint32_t i = base + u * TB;
            if (i < nwords) {
              t[u] = a.hm[g0 + i];
              if (C::DS) tp[u] = a.hmp[g0 + i];
            }
          }
          if (!tables_done) copy_all_tables();
#pragma unroll
          for (int u = 0; u < UN; ++u) {
            const uint32_t i = base + u * TB;
            if (i < nwords) {
              const uint32_t d = lds_index(i);
              hm[d] = t[u];
              if (C::DS) hmp[d] = tp[u];
            }
          }
        }
      }
    }
    if (!tables_done) copy_all_tables();
    for (int idx = threadIdx.x; idx < ns * g.LWs(); idx += TB) let[idx] = 0u;
    // The exact path of the hidden sampler, block-wide (DEFER).  A unit whose coarse 12-bit field cannot
    // decide it (2^-12 of all units, but some lane of a wave in 14.5 % of all rounds at K = 10) is not
    // resolved by its wave -- that costs the whole wave a second Philox call and a pass over its ten
    // units -- but queued: (item, unit, strand) in one word.  After the pass the block drains the queue,
    // one entry per thread: activation of that one unit (same table rows, same order of additions),
    // both Philox calls, the exact comparison of sample_hidden, one atomic OR into the mask word.
    auto resolve = [&](uint32_t e, int st, bool last) -> uint32_t {
      const uint32_t it = e & 0xFFFFFu, k = (e >> 20) & 0x7FFu, strand = e >> 31;
      const uint32_t nl = g.div_hb(it);
      const int s = (int)(it - nl * (uint32_t)g.nhb());
      const uint32_t gn = a.rng.seq_offset + (uint32_t)(n0 + nl);
      LetterWin<M> win = letter_window<M>(let + nl * (uint32_t)g.LWs(), s);
      if (strand) win = revcomp_window<M>(win);
      const float* T = Tf + k;
      float z = 0.f;
#pragma unroll
      for (int g = 0; g < C::NG; ++g) {
        const uint32_t r = window_bits<C::M>(win, 2 * C::G * g) & (uint32_t)(C::ROWS - 1);
        const float t = T[((size_t)g * C::ROWS + r) * KP];
        z = g == 0 ? t : z + t;
      }
      const uint32_t g10 = k / 10u, i10 = k - 10u * g10, step = a.rng.step + (uint32_t)st;
      const Philox4 rc = philox4x32(gn, (uint32_t)s, rng_word2(KIND_CHAIN_H, strand, 0, g10), step, a.rng.seed_lo, a.rng.seed_hi);
      const Philox4 rf = philox4x32(gn, (uint32_t)s, rng_word2(KIND_CHAIN_H, strand, 1, g10), step, a.rng.seed_lo, a.rng.seed_hi);
      const float t = 4096.0f * fast_rcp(1.0f + exp_neg_x(z));
      const float frac = t - (float)philox_field12_dyn(rc, (int)i10);
      const uint32_t one = frac * 4096.0f > (float)philox_field12_dyn(rf, (int)i10) ? 1u : 0u;
      if (one) {
        const uint32_t bit = 1u << (k & 31u), w = k >> 5;
        if (last) { if (!(dbg & 4)) atomicOr((strand ? a.hmp : a.hm) + (size_t)n0 * per + it * (uint32_t)NW + w, bit); }
        else atomicOr((strand ? hmp : hm) + (nl * (uint32_t)(rowW - (int)per) + it * (uint32_t)NW + (uint32_t)((M - 1) * NW)) + w, bit);
      }
      return one;
    };
    // queue the undecided units of one item (rare; lanes without any do nothing)
    auto defer_units = [&](const uint32_t (&pending)[C::NGRP], uint32_t it, uint32_t strand, int st, bool last) -> uint32_t {
      uint32_t any = 0u, ones = 0u;
#pragma unroll
      for (int g = 0; g < C::NGRP; ++g) any |= pending[g];
      if (__any(any != 0u)) {
#pragma unroll
        for (int g = 0; g < C::NGRP; ++g) {
          uint32_t m = pending[g];
          while (m) {
            const uint32_t i = (uint32_t)__ffs(m) - 1u;
            m &= m - 1u;
            const uint32_t e = it | ((10u * (uint32_t)g + i) << 20) | (strand << 31);
            const uint32_t slot = atomicAdd(&fixq[0], 1u);
            if (slot < (uint32_t)FIXQ_CAP) fixq[2 + slot] = e;
            else ones += resolve(e, st, last);        // queue full (never at the sizes that run): resolve in place
          }
        }
      }
      return ones;
    };
    auto drain_queue = [&](int st, bool last) {
      // the last pass stored its mask words to global memory: they must have arrived before another
      // wave's atomic OR may touch them (s_waitcnt vmcnt(0); the barrier itself only waits for LDS)
      if (last) wait_vector_memory();
      __syncthreads();                                // every mask word of the pass is stored, every entry queued
      const uint32_t nq = min(fixq[0], (uint32_t)FIXQ_CAP);
      for (uint32_t e = threadIdx.x; e < nq; e += TB) {
        const uint32_t one = resolve(fixq[2 + e], st, last);
        if (last) nset += (int)one;
      }
    };
    for (int st = 0; st < a.steps; ++st) {
      __syncthreads();
      if (threadIdx.x == 0) fixq[0] = 0u;             // read by drain_queue before this barrier, filled again after the next
      // ---- v | h : y[a,p] = c[a] + sum_{k,j} W[k,a,j] h[k,p-j] (+ rc strand) ----
      for (uint32_t it = threadIdx.x; it < (uint32_t)(ns * g.nvb()); it += TB) {
        const uint32_t nl = g.div_vb(it);
        const int pb = (int)(it - nl * (uint32_t)g.nvb());
        const int p0 = 4 * pb;
        float y[4][4];
#pragma unroll
        for (int i = 0; i < 4; ++i) { y[i][0] = cv[0]; y[i][1] = cv[1]; y[i][2] = cv[2]; y[i][3] = cv[3]; }
        if constexpr (SPARSE) {
          // the copies of c are made here, once, as register pairs: left to itself the compiler makes them on both
          // sides of the first set-bit walk's entry test, twelve moves where six do
#pragma unroll
          for (int i = 1; i < 4; ++i)
#pragma unroll
            for (int h = 0; h < 2; ++h) {
              const floatx2 pr = opaque(floatx2{y[i][2 * h], y[i][2 * h + 1]});
              y[i][2 * h] = pr[0]; y[i][2 * h + 1] = pr[1];
            }
        }
        if constexpr (!SPARSE) {
          // masks p0 .. p0+M+2 (padded row), then one float4 table row per
          // (filter column, 5-bit chunk) of each mask
          constexpr int NMV = (M + 3 + 3) / 4;
#pragma unroll
          for (int strand = 0; strand <= C::DS; ++strand) {
            const uint4* mrow = reinterpret_cast<const uint4*>((strand ? hmp : hm) + (size_t)nl * g.Lrow() + p0);
            const char* Tv = reinterpret_cast<const char*>(smem + (strand ? C::OFF_TVR : C::OFF_TV));
            uint32_t off[4 * NMV][NCH];
#pragma unroll
            for (int v4 = 0; v4 < NMV; ++v4) {
              const uint4 mm = mrow[v4];
              const uint32_t m4[4] = {mm.x, mm.y, mm.z, mm.w};
#pragma unroll
              for (int e = 0; e < 4; ++e)
#pragma unroll
                for (int ch = 0; ch < NCH; ++ch)
                  off[4 * v4 + e][ch] = (5 * ch >= 4 ? (m4[e] >> (5 * ch - 4)) : (m4[e] << (4 - 5 * ch))) & 0x1F0u;
            }
#pragma unroll
            for (int jr = 0; jr < M; ++jr)
#pragma unroll
              for (int ch = 0; ch < NCH; ++ch)
#pragma unroll
                for (int i = 0; i < 4; ++i) {
                  const float4 t = *reinterpret_cast<const float4*>(Tv + (jr * NCH + ch) * 512 + off[i + jr][ch]);
                  y[i][0] += t.x; y[i][1] += t.y; y[i][2] += t.z; y[i][3] += t.w;
                }
          }
        } else {
          // window slots q = 0 .. M+2 are the masks at padded-row positions p0 .. p0+M+2;
          // their bits are packed into 64-bit words (as many whole masks as fit) and every
          // set bit adds one table row to each of the 4 positions
          constexpr int NSLOT = M + 3;
          constexpr int PPW = NW == 1 ? 64 / C::K : 1;         // masks per word
          constexpr int NWORD = (NSLOT + PPW - 1) / PPW;
#pragma unroll
          for (int strand = 0; strand <= C::DS; ++strand) {
            const uint32_t* mrow = (strand ? hmp : hm) + ((size_t)nl * g.Lrow() + p0) * NW;
            const char* tab = reinterpret_cast<const char*>(smem + (strand ? C::SP_WSR : C::SP_WS));
            if constexpr (NW == 1) {
              constexpr int NMV = (NSLOT + 3) / 4;
              uint32_t m[4 * NMV];
#pragma unroll
              for (int v4 = 0; v4 < NMV; ++v4) {
                const uint4 mm = reinterpret_cast<const uint4*>(mrow)[v4];
                m[4 * v4] = mm.x; m[4 * v4 + 1] = mm.y; m[4 * v4 + 2] = mm.z; m[4 * v4 + 3] = mm.w;
              }
#pragma unroll
              for (int wi = 0; wi < NWORD; ++wi) {
                // (the halves of the word apart: 32-bit shift-ors; bit t*K + k keeps its place)
                uint32_t lo = 0u, hi = 0u;
                pack_masks<C::K, 0, PPW>(m + wi * PPW, NSLOT - wi * PPW, lo, hi);
                const unsigned long long w = (unsigned long long)lo | ((unsigned long long)hi << 32);
                topdown_bits<C>(w, tab, wi * PPW, y);
              }
            } else {
#pragma unroll 1
              for (int q = 0; q < NSLOT; ++q) {
                if constexpr (NW == 2) {
                  const uint2 mm = *reinterpret_cast<const uint2*>(mrow + 2 * q);
                  topdown_bits<C>((unsigned long long)mm.x | ((unsigned long long)mm.y << 32), tab, q, y);
                } else {
                  // more than 64 motifs: 64 units at a time (a mask is NW words, 4-byte aligned only)
#pragma unroll
                  for (int w2 = 0; 2 * w2 < NW; ++w2) {
                    const uint32_t lo = mrow[NW * q + 2 * w2], hi = 2 * w2 + 1 < NW ? mrow[NW * q + 2 * w2 + 1] : 0u;
                    topdown_bits<C>((unsigned long long)lo | ((unsigned long long)hi << 32), tab, q, y, 64 * w2);
                  }
                }
              }
            }
          }
        }
        // one Philox call serves the 4 positions of the block (convRBM.py:301-315)
        const Philox4 r = philox4x32<!DEFER>(a.rng.seq_offset + (uint32_t)(n0 + nl), (uint32_t)pb,   // DEFER: see CRBM_DIET2_C1
                                              rng_word2(KIND_CHAIN_V, 0, 0, 0), a.rng.step + (uint32_t)st,
                                              a.rng.seed_lo, a.rng.seed_hi);
        uint32_t inv = 0u;
#pragma unroll
        for (int i = 3; i >= 0; --i) inv = push_letter(inv, y[i][0], y[i][1], y[i][2], y[i][3], u01(r.v[i]));
        const uint32_t byte = letter_byte<GP::WHOLE_BYTES>(inv, p0, g.Lv());
        reinterpret_cast<unsigned char*>(let + (size_t)nl * g.LWs())[pb] = (unsigned char)byte;
      }
      __syncthreads();
      bool fused_pass = false;
      if constexpr (STATS) if (st == a.steps - 1) {
        fused_pass = true;
        // ---- last h | v with the model statistics: wave units of two 32-position groups ----
        constexpr int KW = SR::KW;
        const int GPC = a.sg.GPC, ngl = ns * GPC;
        for (int u = wave; 2 * u < ngl; u += nwaves) {
          const int G0 = 2 * u;
          constexpr int NPW = C::NPW;
          if (lane < 8 * NPW) {                 // letter windows of the two groups (and the letter counts)
            const int G = G0 + lane / (4 * NPW), w = (lane >> 2) % NPW;
            int gi = 0;
            uint32_t word = 0u;
            if (G < ngl) {
              const uint32_t nl = fastdiv_tile((uint32_t)G, a.sg.divGPC);
              gi = G - (int)nl * GPC;
              if (2 * gi + w < g.LWs()) word = let[(size_t)nl * g.LWs() + 2 * gi + w];
            }
            vcount += stats_window_piece<NPW>(reinterpret_cast<unsigned short*>(swin), lane, word, G < ngl, gi, GPC, g.Lv());
          }
          __builtin_amdgcn_wave_barrier();
          {
            const int slot = lane >> 5, G = G0 + slot;
            bool valid = G < ngl;
            uint32_t nl = 0u;
            int s = 0;
            if (valid) {
              nl = fastdiv_tile((uint32_t)G, a.sg.divGPC);
              s = 32 * (G - (int)nl * GPC) + (lane & 31);
              valid = s < g.Lf();
            }
            float* col = sPt + lane;
            if (valid) {
              const uint32_t gn = a.rng.seq_offset + (uint32_t)(n0 + nl);
              const LetterWin<M> win = letter_window<M>(let + (size_t)nl * g.LWs(), s);
#pragma unroll
              for (int strand = 0; strand <= C::DS; ++strand) {
                float x[KP], p[KP];
                conv_gather<C>(Tf, strand ? revcomp_window<M>(win) : win, x);
                uint32_t mask[NW];
                uint32_t pend[C::NGRP];
                sample_hidden<C, 2, DEFER>(x, gn, (uint32_t)s, KIND_CHAIN_H, (uint32_t)strand, a.rng,
                                           a.rng.step + (uint32_t)st, mask, p, pend);
                // the last pass of the launch: the new state goes straight to global memory
                uint32_t* dst = (strand ? a.hmp : a.hm) + (size_t)(n0 + nl) * per + (size_t)s * NW;
#pragma unroll
                for (int w = 0; w < NW; ++w) {
                  if (!(dbg & 4)) store1_streaming(dst + w, mask[w]);
                  nset += __popc(mask[w]);
                }
                if constexpr (DEFER) nset += (int)defer_units(pend, nl * (uint32_t)g.nhb() + (uint32_t)s, (uint32_t)strand, st, true);
#pragma unroll
                for (int k = 0; k < C::K; ++k) col[(size_t)(strand * KW + k) * STATS_RS] = p[k];
              }
            } else {
#pragma unroll
              for (int r = 0; r < SR::KINDS * KW; ++r) col[(size_t)r * STATS_RS] = 0.f;
            }
          }
          __builtin_amdgcn_wave_barrier();
#pragma unroll
          for (int slot = 0; slot < 2; ++slot)
            if (G0 + slot < ngl)
              stats_mfma_group<C, SR, false>(sPt, swin + 2 * C::NPW * slot, reinterpret_cast<const uint32_t*>(sreg), 0, slot, sacc);
          __builtin_amdgcn_wave_barrier();       // the slice is rewritten by the next unit
        }
      }
      if (!fused_pass) {
      // ---- h | v : x[k,s] = b[k] + sum_j W[k, letter[s+j], j]; h = [sigma(x) > u] ----
      // one hidden position per item (nhb = Lf items per chain): the K units of a position
      // already give the instruction-level parallelism, and single positions spread evenly
      // over the waves of the block
      for (uint32_t it = threadIdx.x; it < (uint32_t)(ns * g.nhb()); it += TB) {
        const uint32_t nl = g.div_hb(it);
        const int s = (int)(it - nl * (uint32_t)g.nhb());
        const uint32_t gn = a.rng.seq_offset + (uint32_t)(n0 + nl);
        const uint32_t* lrow = let + nl * (uint32_t)g.LWs();        // LDS offsets: 32-bit arithmetic
        const LetterWin<M> win = letter_window<M>(lrow, s);
#pragma unroll
        for (int strand = 0; strand <= C::DS; ++strand) {
          float x[KP], p[KP];
          uint32_t mask[NW], pend[C::NGRP];
          if constexpr (C::POOL > 1) {
            auto zfun = [&](int pos, float (&z)[KP]) {
              const LetterWin<M> w = letter_window<M>(lrow, pos);
              conv_gather<C>(Tf, strand ? revcomp_window<M>(w) : w, z);
            };
            float cb[KP], S[KP], u[KP];
            pooled_probs<C::POOL, KP>(zfun, s, p, cb, S);
            hidden_uniforms24<C>(gn, (uint32_t)(s - s % C::POOL), KIND_CHAIN_H, (uint32_t)strand, a.rng, a.rng.step + (uint32_t)st, u);
            pooled_sample<C>(p, cb, u, mask);
          } else {
          conv_gather<C>(Tf, strand ? revcomp_window<M>(win) : win, x);
          sample_hidden<C, 0, DEFER>(x, gn, (uint32_t)s, KIND_CHAIN_H, (uint32_t)strand, a.rng,
                                     a.rng.step + (uint32_t)st, mask, p, pend);
          }
          if (st == a.steps - 1) {
            // the last pass of the launch: the new state goes straight to global memory (the stores
            // drain behind the remaining items instead of in a phase of their own after a barrier)
            // (item `it` of the tile is word it * NW of its contiguous state: nhb = Lf positions per chain)
            uint32_t* dst = (strand ? a.hmp : a.hm) + (size_t)n0 * per + it * (uint32_t)NW;
#pragma unroll
            for (int w = 0; w < NW; ++w) {
              if (!(dbg & 4)) store1_streaming(dst + w, mask[w]);
              nset += __popc(mask[w]);
            }
          } else {
            uint32_t* dst = (strand ? hmp : hm) + (nl * (uint32_t)(rowW - (int)per) + it * (uint32_t)NW + (uint32_t)((M - 1) * NW));
#pragma unroll
            for (int w = 0; w < NW; ++w) dst[w] = mask[w];
          }
          if constexpr (DEFER) {
            const uint32_t ones = defer_units(pend, it, (uint32_t)strand, st, st == a.steps - 1);
            if (st == a.steps - 1) nset += (int)ones;
          }
        }
      }
      }
      if constexpr (DEFER) drain_queue(st, st == a.steps - 1);
    }
    // LDS -> chain state (contiguous in global memory, 16-byte stores where aligned): only a launch
    // without steps (state round trip) still has the state in LDS here
    // (GeomCT launches always step: the host sends a launch without steps to the run-time form)
    const bool round_trip = !GP::CT && a.steps == 0;
    if (round_trip) __syncthreads();
    if (round_trip && !(dbg & 4)) {
      const uint32_t nwords = (uint32_t)ns * per;
      const size_t g0 = (size_t)n0 * per;
      auto lds_index = [&](uint32_t i) {
        const uint32_t nl = g.template div_lfw<NW>(i);
        return nl * (uint32_t)rowW + (uint32_t)((M - 1) * NW) + (i - nl * per);
      };
      if (((g0 | nwords) & 3u) == 0u) {
        for (uint32_t i4 = threadIdx.x; i4 < nwords / 4; i4 += TB) {
          const uint32_t d0 = lds_index(4 * i4), d1 = lds_index(4 * i4 + 1), d2 = lds_index(4 * i4 + 2), d3 = lds_index(4 * i4 + 3);
          store4_streaming(a.hm + g0 + 4 * (size_t)i4, hm[d0], hm[d1], hm[d2], hm[d3]);
          if (C::DS) store4_streaming(a.hmp + g0 + 4 * (size_t)i4, hmp[d0], hmp[d1], hmp[d2], hmp[d3]);
        }
      } else {
        for (uint32_t i = threadIdx.x; i < nwords; i += TB) {
          const uint32_t d = lds_index(i);
          a.hm[g0 + i] = hm[d];
          if (C::DS) a.hmp[g0 + i] = hmp[d];
        }
      }
    }
    if (a.vout && !(dbg & 4))
      for (int idx = threadIdx.x; idx < ns * g.LWs(); idx += TB)
        a.vout[(size_t)n0 * g.LWs() + idx] = let[idx];
  }
  if (a.ones) {   // one plain store per wave, summed by the host (counts stay far below 2^24: exact in float)
    const float tot = wave_sum((float)nset);
    if ((threadIdx.x & 63) == 0) a.ones[bid * (TB >> 6) + (threadIdx.x >> 6)] = (uint32_t)tot;
  }
  if constexpr (GP::PROF) {
    if (a.clock && bid == 0 && threadIdx.x == 0) {
      a.clock[0] += realtime_ticks() - a.clock[2];
      a.clock[1] += shader_cycles() - a.clock[3];
    }
    if (a.timeline && bid == 0 && threadIdx.x == 0) a.timeline[1] = realtime_ticks();
  }
  if constexpr (STATS) stats_mfma_finish<C, false>(a.sg, smem, 0, bid, sacc, vcount);
}

// A plain chain launch in a compiled-in geometry.  The timed launches still sample both clocks (GibbsArgs::clock,
// crbm_last_shader_clock), here around the body: one scalar test per wave, the reads on block 0's first thread alone.
template <class C, class GP>
__device__ void gibbs_geo_body(const GibbsArgs& a) {
  const bool timed = a.clock && blockIdx.x == 0 && threadIdx.x == 0;
  if (timed) {
    a.clock[2] = realtime_ticks();
    a.clock[3] = shader_cycles();
  }
  gibbs_body<C, true, false, GP>(a);
  if (timed) {
    a.clock[0] += realtime_ticks() - a.clock[2];
    a.clock[1] += shader_cycles() - a.clock[3];
  }
}

// The local phase of a training step in ONE launch (convRBM.py:373-413): g.nblocks blocks advance the
// persistent chains and leave the model half of the statistics (gibbs_body, STATS variant), d.nblocks
// blocks compute the data half (stats_mfma_body with the sparsity columns) -- the two halves are
// independent given (W, b, c).  Same block size, similar LDS footprint; the two kinds alternate in
// the grid, so every CU runs chain blocks (VALU and LDS gathers) beside statistics blocks (matrix
// pipe) from the first cycle, and there is no second launch floor and no idle tail between them.
struct TrainLocalArgs {
  GibbsArgs g;
  StatsMfmaArgs d;
};

template <class C, class GP = GeomRT>
__device__ void train_local_body(const TrainLocalArgs& a) {
  if constexpr (C::FUSE_STATS) {
    const int nG = a.g.nblocks, nD = a.d.nblocks, m = min(nG, nD), b = (int)blockIdx.x;
    const bool chain = b < 2 * m ? !(b & 1) : nG > nD;      // alternate while both kinds last, then the rest
    const int idx = b < 2 * m ? b >> 1 : b - m;
    if (chain) gibbs_body<C, true, true, GP>(a.g, idx);
    else stats_mfma_body<C, true, false>(a.d, idx);
  }
}

// ---------------------------------------------------------------------------
// Free energy (convRBM.py:657-697): one wave per sequence.
//   fe[n]    = ( -sum_{k,s} softplus(x) [- rc strand] - sum_p c[letter_p] ) / L
//   fem[n,k] =   -sum_s softplus(x[k]) [- rc strand] - sum_p c[letter_p]
// ---------------------------------------------------------------------------
struct FeArgs {
  const float* tables;
  const uint32_t* letters;
  int32_t n, L, Lh, LW;
  float* fe;
  float* fem;
};

// softplus(x) = max(x,0) + log1p(exp(-|x|)) from z = -x*log2(e), on the hardware
// exp2/log2: log1p by its series below 2^-5 (where 1+t would round t away), by
// log2(1+t) above; relative error of either branch < 3e-7.
__device__ __forceinline__ float softplus_of_z(float z) {
  const float t = __builtin_amdgcn_exp2f(-fabsf(z));
  const float series = t * (1.0f - t * (0.5f - t * (0.33333334f - 0.25f * t)));
  const float vialog = 0.6931471805599453f * __builtin_amdgcn_logf(1.0f + t);
  return fmaxf(x_of_z(z), 0.f) + (t < 0.03125f ? series : vialog);
}

template <class C>
__device__ void free_energy_body(const FeArgs& a) {
  constexpr int KP = C::KP, K = C::K, M = C::M;
  HIP_DYNAMIC_SHARED(float, smem);
  float* Tf = smem;
  copy_tables<C::TAB>(Tf, a.tables + C::OFF_TF);
  __syncthreads();
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, nwaves = blockDim.x >> 6;
  const float* cg = a.tables + C::OFF_C;          // log2(e) * c
  const float c0 = LN2 * cg[0], c1 = LN2 * cg[1], c2 = LN2 * cg[2], c3 = LN2 * cg[3];
  for (int nn = blockIdx.x * nwaves + wave; nn < a.n; nn += gridDim.x * nwaves) {
    const uint32_t* row = a.letters + (size_t)nn * a.LW;
    float acc[KP];
#pragma unroll
    for (int q = 0; q < KP; ++q) acc[q] = 0.f;
    if constexpr (C::POOL > 1) {
      // one term per pooling group, log(1 + sum_j exp(x_j)) (convRBM.py:664-665): a lane takes whole groups
      for (int g0 = lane * C::POOL; g0 < a.Lh; g0 += 64 * C::POOL)
#pragma unroll
        for (int strand = 0; strand <= C::DS; ++strand) {
          auto zfun = [&](int pos, float (&z)[KP]) {
            const LetterWin<M> w = letter_window<M>(row, pos);
            conv_gather<C>(Tf, strand ? revcomp_window<M>(w) : w, z);
          };
          pooled_softplus<C::POOL, KP>(zfun, g0, acc, K);
        }
    } else
    for (int s = lane; s < a.Lh; s += 64) {
      const LetterWin<M> win = letter_window<M>(row, s);
      float x[KP];
      conv_gather<C>(Tf, win, x);
#pragma unroll
      for (int q = 0; q < K; ++q) acc[q] += softplus_of_z(x[q]);
      if (C::DS) {
        conv_gather<C>(Tf, revcomp_window<M>(win), x);
#pragma unroll
        for (int q = 0; q < K; ++q) acc[q] += softplus_of_z(x[q]);
      }
    }
    float cs = 0.f;
    for (int p = lane; p < a.L; p += 64) {
      const uint32_t l = (row[p >> 4] >> (2 * (p & 15))) & 3u;
      cs += l == 0u ? c0 : l == 1u ? c1 : l == 2u ? c2 : c3;
    }
    cs = wave_sum(cs);
    float tot = 0.f;
#pragma unroll
    for (int q = 0; q < K; ++q) {
      const float v = wave_sum(acc[q]);
      tot += v;
      if (lane == 0 && a.fem) a.fem[(size_t)nn * K + q] = -v - cs;
    }
    if (lane == 0 && a.fe) a.fe[nn] = (-tot - cs) / (float)a.L;
  }
}

// ===========================================================================
// Motif-hit summaries for data-set scale sweeps.  The reference's
// analysis code only ever reduces motifHitProbs() (convRBM.py:507-514): the max
// and the mean over positions per (sequence, motif) (utils.py:154, :242-244,
// :305) and the mean over sequences per (motif, position) (utils.py:113-116).
// This kernel produces those three reductions directly, so the dense
// (n,K,1,Lh) tensor never exists.  One wave per sequence; a lane owns HIT_NI
// positions (stride 64) of the chunk blockIdx.y of 64*HIT_NI positions and keeps
// their sums over sequences in registers.  Whatever is combined across waves, blocks
// or chunks is combined in FIXED POINT (2^-30 units, 64-bit integer atomics): integer
// addition does not care about the order, so the sums are the same bits in every run
// (float atomics gave run-to-run differences in the last place).
// ===========================================================================
constexpr float HIT_FX = 1073741824.0f;          // 2^30 units per 1.0: probabilities are <= 1, sums stay far below 2^63
struct HitArgs {
  const float* tables;
  const uint32_t* letters;
  int32_t n, L, Lh, LW;
  float* hmax;      // (n,K) max over positions   (zero-initialised when gridDim.y > 1)
  float* hsum;      // (n,K) mean over positions, written directly when gridDim.y == 1
  unsigned long long* hsum_fx;   // (n,K) fixed-point sums over positions when gridDim.y > 1 (zero-initialised; hit_finalize_kernel)
  float inv_Lh;     // 1 / Lh
  unsigned long long* pos_fx;    // (K,Lh) fixed-point sums over sequences (zero-initialised), or null
};
__device__ __forceinline__ unsigned long long to_fx(float v) { return (unsigned long long)(v * HIT_FX); }

template <class C>
__device__ void hit_summary_body(const HitArgs& a) {
  constexpr int KP = C::KP, K = C::K, M = C::M, NI = C::HIT_NI, PC = 64 * NI;
  constexpr bool BOTH = !C::DS;   // single-stranded models report sigma(x + x'), convRBM.py:511-514
  HIP_DYNAMIC_SHARED(float, smem);
  float* Tf = smem;
  unsigned long long* acc = reinterpret_cast<unsigned long long*>(Tf + C::TAB);   // [PC][K], block total of the waves' register sums (TAB: a multiple of 4 floats)
  copy_tables<C::TAB>(Tf, a.tables + C::OFF_TF);
  const int s0 = blockIdx.y * PC;
  if (a.pos_fx)
    for (int i = threadIdx.x; i < PC * K; i += blockDim.x) acc[i] = 0ull;
  __syncthreads();
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, nwaves = blockDim.x >> 6;
  float pacc[NI][K];
#pragma unroll
  for (int i = 0; i < NI; ++i)
#pragma unroll
    for (int q = 0; q < K; ++q) pacc[i][q] = 0.f;
  for (int nn = blockIdx.x * nwaves + wave; nn < a.n; nn += gridDim.x * nwaves) {
    const uint32_t* row = a.letters + (size_t)nn * a.LW;
    float mx[K], sm[K];
#pragma unroll
    for (int q = 0; q < K; ++q) { mx[q] = 0.f; sm[q] = 0.f; }
#pragma unroll
    for (int i = 0; i < NI; ++i) {
      const int s = s0 + lane + 64 * i;
      if (s < a.Lh) {
        auto zfun = [&](int pos, float (&zz)[KP]) {
          const LetterWin<M> w = letter_window<M>(row, pos);
          conv_gather<C>(Tf, w, zz);
          if (BOTH) conv_gather<C, true>(Tf, revcomp_window<M>(w), zz);
        };
        float z[KP], pp[KP];
        if constexpr (C::POOL > 1) {
          float cb[KP], S[KP];
          pooled_probs<C::POOL, KP>(zfun, s, pp, cb, S);
        } else {
          zfun(s, z);
#pragma unroll
          for (int q = 0; q < K; ++q) pp[q] = sigmoid_z(z[q]);
        }
#pragma unroll
        for (int q = 0; q < K; ++q) {
          const float p = pp[q];
          mx[q] = fmaxf(mx[q], p);
          sm[q] += p;
          pacc[i][q] += p;
        }
      }
    }
#pragma unroll
    for (int q = 0; q < K; ++q) {
      const float m = wave_max_nonneg(mx[q]);
      const float t = wave_sum(sm[q]);
      if (lane == 0) {
        const size_t idx = (size_t)nn * K + q;
        if (gridDim.y == 1) {
          if (a.hmax) a.hmax[idx] = m;
          if (a.hsum) a.hsum[idx] = t * a.inv_Lh;
        } else {   // probabilities are >= 0: their bit patterns order like unsigned integers
          if (a.hmax) atomicMax(reinterpret_cast<unsigned int*>(a.hmax) + idx, __float_as_uint(m));
          if (a.hsum_fx) atomicAdd(a.hsum_fx + idx, to_fx(t));
        }
      }
    }
  }
  if (a.pos_fx) {
#pragma unroll
    for (int i = 0; i < NI; ++i)
#pragma unroll
      for (int q = 0; q < K; ++q) atomicAdd(&acc[(lane + 64 * i) * K + q], to_fx(pacc[i][q]));
    __syncthreads();
    const int npos = min(PC, a.Lh - s0);
    for (int i = threadIdx.x; i < npos * K; i += blockDim.x) {
      const int sl = i / K, q = i - sl * K;
      if (acc[i]) atomicAdd(a.pos_fx + (size_t)q * a.Lh + s0 + sl, acc[i]);
    }
  }
}

// ===========================================================================
// Motif sites (crbm_motif_sites*): every (sequence, motif, position, strand) whose pooled probability reaches a
// threshold, as a compact list of records, and the best site of every (sequence, motif) -- without the dense
// (n,K,1,Lh) tensor of motifHitProbs() (convRBM.py:507-514).  Scores: single-stranded models sigma-pool(x + x')
// (what motifHitProbs reports, strand 0), double-stranded ones the forward strand (+1, what motifHitProbs reports)
// and the reverse-complemented filter (-1, the forward gather of the reverse-complemented window: revcomp_window).
//   records: a wave reserves the slots of its hits with ONE 64-bit atomicAdd on the slab's counter (per sequence and
//            position chunk in the fused pass, per step in the select pass) and every lane writes its hits at base +
//            (hits of earlier motifs) + (hits of lower lanes); records land only below `capacity`, the counter keeps
//            counting past it.  Their order is the order of the atomics: the
//            host sorts them (crbm_api.hip, motif_sites_any).
//   best:    one 64-bit key per (sequence, motif), prob bits on top (probabilities are >= 0: their bits order like
//            integers) and ~(2 start + strand_bit) below, so that the largest key is the largest probability, then
//            the smaller start, then + before -.  Reduced per wave, stored directly when the positions of a sequence
//            are one chunk, atomicMax (zero-initialised keys; a real key is never 0) across chunks.
// No float is ever combined across threads: every number is a per-position probability, the same bits in every run.
// ===========================================================================
struct SiteRec {      // crbm_site of include/crbm_amd.h
  int32_t seq, motif, start, strand;
  float prob;
};
struct SitesOut {
  SiteRec* recs;                 // records, or null (no list)
  unsigned long long capacity;   // records `recs` holds
  unsigned long long* count;     // the slab's counter (zero-initialised), exact past capacity
  unsigned long long* best;      // (n,K) keys, or null
  float threshold;
};
struct SitesArgs {
  const float* tables;
  const uint32_t* letters;
  int32_t n, L, Lh, LW;
  SitesOut o;
};
__device__ __forceinline__ unsigned long long site_key(float p, int start, int strand_bit) {
  return ((unsigned long long)__float_as_uint(p) << 32) | (unsigned long long)(0xFFFFFFFFu - (uint32_t)(2 * start + strand_bit));
}
// the larger key of the wave (all lanes call it; every lane gets it)
__device__ __forceinline__ unsigned long long wave_max_key(unsigned long long key) {
  const uint32_t hi = wave_max_u32((uint32_t)(key >> 32));
  const uint32_t lo = wave_max_u32((uint32_t)(key >> 32) == hi ? (uint32_t)key : 0u);
  return ((unsigned long long)hi << 32) | lo;
}
// hits of NS candidates per lane over the wave (all lanes call it)
template <int NS>
__device__ __forceinline__ uint32_t count_sites(const bool (&hit)[NS]) {
  uint32_t tot = 0;
#pragma unroll
  for (int j = 0; j < NS; ++j) tot += (uint32_t)__popcll(__ballot(hit[j]));
  return tot;
}
// `tot` slots of the slab's record list for the wave: one atomicAdd (lane 0), the base handed to every lane
__device__ __forceinline__ unsigned long long reserve_sites(const SitesOut& o, uint32_t tot) {
  unsigned long long base = 0;
  if ((threadIdx.x & 63) == 0) base = atomicAdd(o.count, (unsigned long long)tot);
  return ((unsigned long long)(uint32_t)__builtin_amdgcn_readlane((int)(base >> 32), 0) << 32) |
         (uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)base, 0);
}
// Records of NS candidates per lane into reserved slots from `base` on (all lanes of the wave call it with the same
// NS); hit[j] says whether this lane's candidate j is a site, rec(j) makes its record.  Slot order: candidate j, then
// lane.  `base` moves past the wave's hits.
template <int NS, class RecFun>
__device__ __forceinline__ void write_sites(const SitesOut& o, const bool (&hit)[NS], RecFun rec, unsigned long long& base) {
  unsigned long long m[NS];
#pragma unroll
  for (int j = 0; j < NS; ++j) m[j] = __ballot(hit[j]);
#pragma unroll
  for (int j = 0; j < NS; ++j) {
    const unsigned long long idx = base + lanes_below(m[j]);
    if (hit[j] && idx < o.capacity) {
      const SiteRec r = rec(j);
      SiteRec* d = o.recs + idx;
      d->seq = r.seq; d->motif = r.motif; d->start = r.start; d->strand = r.strand; d->prob = r.prob;
    }
    base += (unsigned long long)__popcll(m[j]);
  }
}
// reserve_sites + write_sites for one step
template <int NS, class RecFun>
__device__ __forceinline__ void emit_sites(const SitesOut& o, const bool (&hit)[NS], RecFun rec) {
  const uint32_t tot = count_sites<NS>(hit);
  if (tot == 0) return;                                      // wave-uniform
  unsigned long long base = reserve_sites(o, tot);
  write_sites<NS>(o, hit, rec, base);
}

// The fused pass of the specialised models: hit_summary_body's geometry (one wave per sequence, a lane owns HIT_NI
// positions of the chunk blockIdx.y of 64*HIT_NI positions), the motifs in groups of NQW quads (registers stay bounded
// at any K: no float[KP] per lane), per group the positions, per position the strands.  With a record list the wave
// walks its sequence twice: it counts its hits, reserves their slots with ONE atomicAdd, then writes them (one atomic
// per step on the one counter serialised the kernel: 58 ms instead of 2 at 10^6 x 200 bp and ~1 site per motif).
template <class C>
__device__ void motif_sites_body(const SitesArgs& a) {
  constexpr int K = C::K, M = C::M, NI = C::HIT_NI, PC = 64 * NI;
  constexpr int NQW = C::NQ < 4 ? C::NQ : 4, NV = 4 * NQW;
  constexpr int S = C::DS ? 2 : 1;
  HIP_DYNAMIC_SHARED(float, smem);
  float* Tf = smem;
  copy_tables<C::TAB>(Tf, a.tables + C::OFF_TF);
  __syncthreads();
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, nwaves = blockDim.x >> 6;
  const int s0 = blockIdx.y * PC;
  const bool want_recs = a.o.recs != nullptr, want_best = a.o.best != nullptr;
  const float thr = a.o.threshold;
  for (int nn = blockIdx.x * nwaves + wave; nn < a.n; nn += gridDim.x * nwaves) {
    const uint32_t* row = a.letters + (size_t)nn * a.LW;
    // p[] = the scores of motifs [4 q0, 4 q0 + NV) at position s on `strand` (0 where s is past the sequence)
    auto scores = [&](int q0, int s, int strand, float (&p)[NV]) {
#pragma unroll
      for (int j = 0; j < NV; ++j) p[j] = 0.f;
      if (s >= a.Lh) return;
      auto zfun = [&](int pos, float (&zz)[NV]) { window_strand_z<C, NQW>(Tf, letter_window<M>(row, pos), q0, strand, zz); };
      if constexpr (C::POOL > 1) {
        float cb[NV], Sg[NV];
        pooled_probs<C::POOL, NV>(zfun, s, p, cb, Sg);
      } else {
        float z[NV];
        zfun(s, z);
#pragma unroll
        for (int j = 0; j < NV; ++j) p[j] = sigmoid_z(z[j]);
      }
    };
    auto hits = [&](int q0, int s, const float (&p)[NV], bool (&hit)[NV]) {
#pragma unroll
      for (int j = 0; j < NV; ++j) hit[j] = s < a.Lh && 4 * q0 + j < K && p[j] >= thr;
    };
    unsigned long long base = 0;
    if (want_recs) {
      uint32_t tot = 0;
#pragma unroll 1
      for (int q0 = 0; q0 < C::NQ; q0 += NQW)
#pragma unroll 1
        for (int i = 0; i < NI; ++i)
#pragma unroll 1
          for (int strand = 0; strand < S; ++strand) {
            float p[NV];
            bool hit[NV];
            scores(q0, s0 + lane + 64 * i, strand, p);
            hits(q0, s0 + lane + 64 * i, p, hit);
            tot += count_sites<NV>(hit);
          }
      if (tot == 0 && !want_best) continue;                // wave-uniform
      if (tot) base = reserve_sites(a.o, tot);
    }
#pragma unroll 1
    for (int q0 = 0; q0 < C::NQ; q0 += NQW) {
      unsigned long long key[NV];
#pragma unroll
      for (int j = 0; j < NV; ++j) key[j] = 0ull;
#pragma unroll 1
      for (int i = 0; i < NI; ++i) {
        const int s = s0 + lane + 64 * i;
#pragma unroll 1
        for (int strand = 0; strand < S; ++strand) {
          float p[NV];
          scores(q0, s, strand, p);
          if (want_recs) {
            const int sign = C::DS ? (strand ? -1 : 1) : 0;
            bool hit[NV];
            hits(q0, s, p, hit);
            write_sites<NV>(a.o, hit, [&](int j) { return SiteRec{nn, 4 * q0 + j, s, sign, p[j]}; }, base);
          }
          if (want_best && s < a.Lh) {
#pragma unroll
            for (int j = 0; j < NV; ++j) {
              const unsigned long long k = site_key(p[j], s, strand);
              key[j] = k > key[j] ? k : key[j];
            }
          }
        }
      }
      if (want_best) {
#pragma unroll
        for (int j = 0; j < NV; ++j) {
          if (4 * q0 + j >= K) continue;                        // wave-uniform
          const unsigned long long k = wave_max_key(key[j]);
          if (lane == 0) {
            unsigned long long* dst = a.o.best + (size_t)nn * K + 4 * q0 + j;
            if (gridDim.y == 1) *dst = k;
            else atomicMax(dst, k);
          }
        }
      }
    }
  }
}

// ===========================================================================
// In-silico mutagenesis (crbm_mutagenesis*): dF[n,p,a] = F(v_n with letter p replaced by a) - F(v_n), F the
// unnormalised free energy L * freeEnergy (convRBM.py:657-676), and the pseudo-log-likelihood
// pll[n] = sum_p -log sum_a exp(-dF[n,p,a]) = sum_p log P(v_p | v_-p).  A substitution at p changes the M windows
// s in [p-M+1, p] and the visible bias; everything else cancels.  This is the fused pass of the specialised models
// with POOL == 1: one wave per sequence; a lane owns hidden position s of a 64-position chunk, gathers its activations
// once per strand and motif-quad group, and for every offset m < M and every x in {1,2,3} forms the activations of the
// window with letter s+m replaced by (letter ^ x) from ONE other table row, T[g][r ^ (x << 2t)] - T[g][r] (g, t: the
// group and slot of the letter in this strand's window; the reverse-complemented window holds the complement at the
// mirrored offset, and complementing commutes with ^ x: the same x names the same forward letter on both strands).
// The differences go into the wave's accumulator in LDS, acc[x-1][p]: in one step the lanes hold distinct s, hence
// distinct p = s + m, at consecutive addresses (ds_read_b32 / ds_write_b32: no bank conflict), and the steps follow
// each other in a fixed order -- no atomics, the same bits in every run.  Indexing by x instead of by the letter
// keeps the plane wave-uniform; the epilogue turns x into the letter.
// ===========================================================================
struct MutArgs {
  const float* tables;
  const uint32_t* letters;
  int32_t n, L, Lh, LW;
  float* dfe;   // (n, L, 4), or null
  float* pll;   // (n), or null
};

// running form of -log sum_a exp(-d_a), overflow-free: mn = the smallest d so far, s = sum exp(-(d - mn))
__device__ __forceinline__ void pll_push(float d, float& mn, float& s) {
  if (d < mn) {
    s = s * __builtin_amdgcn_exp2f(LOG2E * (d - mn)) + 1.0f;
    mn = d;
  } else {
    s += __builtin_amdgcn_exp2f(LOG2E * (mn - d));
  }
}
__device__ __forceinline__ float pll_term(float mn, float s) { return mn - LN2 * __builtin_amdgcn_logf(s); }

template <class C>
__device__ void mutagenesis_body(const MutArgs& a) {
  if constexpr (C::POOL == 1) {       // pooled models take the general path (crbm_api.hip): no body
    constexpr int K = C::K, M = C::M, G = C::G;
    constexpr int NQW = C::NQ < 4 ? C::NQ : 4, NV = 4 * NQW;
    HIP_DYNAMIC_SHARED(float, smem);
    float* Tf = smem;
    copy_tables<C::TAB>(Tf, a.tables + C::OFF_TF);
    __syncthreads();
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, nwaves = blockDim.x >> 6;
    const int LP = mut_plane(a.L);
    float* acc = smem + C::TAB + (size_t)wave * 3 * LP;      // acc[(x - 1) * LP + p]
    const float* cg = a.tables + C::OFF_C;                   // log2(e) * c
    const float c0 = LN2 * cg[0], c1 = LN2 * cg[1], c2 = LN2 * cg[2], c3 = LN2 * cg[3];
    // entry i of four values by its two bits (v_cndmask; an indexed array would live in scratch)
    auto pick = [](uint32_t i, float v0, float v1, float v2, float v3) {
      const float lo = (i & 1u) ? v1 : v0, hi = (i & 1u) ? v3 : v2;
      return (i & 2u) ? hi : lo;
    };
    for (int nn = blockIdx.x * nwaves + wave; nn < a.n; nn += gridDim.x * nwaves) {
      const uint32_t* row = a.letters + (size_t)nn * a.LW;
      for (int i = lane; i < 3 * LP; i += 64) acc[i] = 0.f;
      __builtin_amdgcn_wave_barrier();
      for (int s0 = 0; s0 < a.Lh; s0 += 64) {
        const int s = s0 + lane;
        const bool valid = s < a.Lh;
        const LetterWin<M> fwd = letter_window<M>(row, valid ? s : a.Lh - 1);
#pragma unroll 1
        for (int strand = 0; strand <= C::DS; ++strand) {
          const LetterWin<M> win = strand ? revcomp_window<M>(fwd) : fwd;
#pragma unroll 1
          for (int q0 = 0; q0 < C::NQ; q0 += NQW) {
            float z[NV], sp[NV];
            conv_gather_quads<C, NQW>(Tf, win, q0, z);
#pragma unroll
            for (int j = 0; j < NV; ++j) sp[j] = 4 * q0 + j < K ? softplus_of_z(z[j]) : 0.f;
#pragma unroll 1
            for (int m = 0; m < M; ++m) {
              const int o = strand ? M - 1 - m : m;          // the letter's offset in this strand's window
              const int g = o / G, t = o - g * G;
              const uint32_t r = window_bits<M>(win, 2 * G * g) & (uint32_t)(C::ROWS - 1);
              const float4* tab = reinterpret_cast<const float4*>(Tf + (size_t)g * C::ROWS * C::KP) + q0;
              float cur[NV];
#pragma unroll
              for (int q = 0; q < NQW; ++q)
                if (q0 + q < C::NQ) {                        // wave-uniform
                  const float4 v = tab[(size_t)r * C::NQ + q];
                  cur[4 * q] = v.x; cur[4 * q + 1] = v.y; cur[4 * q + 2] = v.z; cur[4 * q + 3] = v.w;
                }
#pragma unroll
              for (int x = 1; x < 4; ++x) {
                const uint32_t r2 = r ^ ((uint32_t)x << (2 * t));
                float d = 0.f;
#pragma unroll
                for (int q = 0; q < NQW; ++q)
                  if (q0 + q < C::NQ) {
                    const float4 v = tab[(size_t)r2 * C::NQ + q];
                    const float alt[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
                    for (int e = 0; e < 4; ++e)
                      if (4 * (q0 + q) + e < K) d += softplus_of_z(z[4 * q + e] + (alt[e] - cur[4 * q + e])) - sp[4 * q + e];
                  }
                if (valid) acc[(x - 1) * LP + s + m] -= d;   // F carries -softplus
              }
              __builtin_amdgcn_wave_barrier();               // the next step's lanes read what this step's neighbours wrote
            }
          }
        }
      }
      // x -> letter, the visible bias -(c[a] - c[v_p]), the position's term of the pseudo-log-likelihood
      float lsum = 0.f;
      for (int p0 = 0; p0 < a.L; p0 += 64) {
        const int p = p0 + lane;
        if (p < a.L) {
          const uint32_t l = (row[p >> 4] >> (2 * (p & 15))) & 3u;
          const float cl = pick(l, c0, c1, c2, c3);
          const float d1 = acc[p] - (pick(l ^ 1u, c0, c1, c2, c3) - cl), d2 = acc[LP + p] - (pick(l ^ 2u, c0, c1, c2, c3) - cl),
                      d3 = acc[2 * LP + p] - (pick(l ^ 3u, c0, c1, c2, c3) - cl);
          if (a.dfe) {
            float4 o4;                                       // letter a holds the difference of x = a ^ l
            o4.x = pick(l, 0.f, d1, d2, d3); o4.y = pick(l ^ 1u, 0.f, d1, d2, d3);
            o4.z = pick(l ^ 2u, 0.f, d1, d2, d3); o4.w = pick(l ^ 3u, 0.f, d1, d2, d3);
            reinterpret_cast<float4*>(a.dfe)[(size_t)nn * a.L + p] = o4;
          }
          float mn = 0.f, sm = 1.f;                          // the sequence's own letter: dF = 0
          pll_push(d1, mn, sm); pll_push(d2, mn, sm); pll_push(d3, mn, sm);
          lsum += pll_term(mn, sm);
        }
      }
      lsum = wave_sum(lsum);
      if (lane == 0 && a.pll) a.pll[nn] = lsum;
      __builtin_amdgcn_wave_barrier();                       // the accumulator is cleared for the wave's next sequence
    }
  }
}

// ===========================================================================
// Annealed importance sampling (Neal 2001; Salakhutdinov & Murray 2008): steps [t0, t1) of the ladder betas[] for
// `runs` independent runs, POOL == 1.  With x, x' the bottom-up activations of the two strands,
//   log p*_beta(v) = sum softplus(beta x(v)) + sum_p (beta c[v_p] + (1 - beta) cA[v_p]),
// step t adds log p*_{betas[t+1]}(v_t) - log p*_{betas[t]}(v_t) to the run's log weight and then takes one Gibbs step
// of the model tempered to betas[t+1]: h ~ sigma(beta x(v_t)), v_{t+1} ~ softmax(beta (c + W^T h + ..) + (1 - beta) cA).
// One wave owns a run; its letter row and mask rows stay in the LDS for all steps of the launch (AisLayout), so
// nothing but wave barriers separates the passes.  The tables are the chain kernel's (built for beta = 1): the
// gathered z = -log2(e) x is multiplied by beta, the top-down image (in units of log 2) enters through one fma per
// letter.  The two softplus terms of a unit share its gather and are differenced per unit; a lane adds its units in
// program order, the wave total comes from wave_sum and is added to the float32 log weight once per step -- the bits
// depend on nothing but (run, ladder), not on the launch geometry or on where the ladder is cut into launches (what
// crosses a cut is the letters and the float32 log weight, nothing else).
// Uniforms: kinds KIND_AIS_V / KIND_AIS_H with the chain's counter layout, sequence word run_offset + run, step word
// 0 for the base-rate draw and t + 1 for step t.
// ===========================================================================
struct AisArgs {
  const float* tables;
  const float* base_c;   // (4) visible bias cA of the base-rate model
  const float* betas;    // the ladder
  uint8_t* state;        // (runs, L) letter codes: read when t0 > 0, written at the end; may be null when t0 == 0
  float* logw;           // (runs): read when t0 > 0, written at the end
  int32_t runs, L, Lh, t0, t1;
  int32_t nvb, Lrow, LWs, run_words;   // AisLayout
  RngView rng;           // seed of the call; seq_offset = global index of run 0
};

template <class C>
__device__ void ais_body(const AisArgs& a) {
  if constexpr (C::POOL == 1) {       // crbm_ais refuses pooled models: no body
    constexpr int K = C::K, KP = C::KP, M = C::M, NW = C::NW;
    HIP_DYNAMIC_SHARED(float, smem);
    copy_tables<C::TAB>(smem, a.tables + C::OFF_TF);
    copy_tables<C::WS * (1 + C::DS) + 4>(smem + C::SP_WS, a.tables + C::OFF_WS);
    __syncthreads();
    const float* Tf = smem;
    const float* cv = smem + C::SP_C;                       // log2(e) * c
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, nwaves = blockDim.x >> 6;
    const int rowW = a.Lrow * NW;
    uint32_t* hm = reinterpret_cast<uint32_t*>(smem + C::SP_TABLES) + (size_t)wave * a.run_words;
    uint32_t* hmp = hm + rowW;
    uint32_t* let = hm + (1 + C::DS) * rowW;
    const float m0 = cv[0], m1 = cv[1], m2 = cv[2], m3 = cv[3];
    // the base-rate bias in the units of the top-down images, and c - cA per letter (exactly 0 where cA is c)
    const float a0 = LOG2E * a.base_c[0], a1 = LOG2E * a.base_c[1], a2 = LOG2E * a.base_c[2], a3 = LOG2E * a.base_c[3];
    const float d0 = LN2 * (m0 - a0), d1 = LN2 * (m1 - a1), d2 = LN2 * (m2 - a2), d3 = LN2 * (m3 - a3);
    auto pick = [](uint32_t i, float v0, float v1, float v2, float v3) {
      const float lo = (i & 1u) ? v1 : v0, hi = (i & 1u) ? v3 : v2;
      return (i & 2u) ? hi : lo;
    };
    for (int run = blockIdx.x * nwaves + wave; run < a.runs; run += gridDim.x * nwaves) {
      const uint32_t gn = a.rng.seq_offset + (uint32_t)run;
      for (int i = lane; i < a.run_words; i += 64) hm[i] = 0u;   // mask pads and letter pads stay zero
      __builtin_amdgcn_wave_barrier();
      float logw = 0.f;
      if (a.t0 == 0) {
        // v_0 ~ softmax(cA), four positions per Philox call like every visible draw
        for (int pb = lane; pb < a.nvb; pb += 64) {
          const Philox4 r = philox4x32(gn, (uint32_t)pb, rng_word2(KIND_AIS_V, 0, 0, 0), 0u, a.rng.seed_lo, a.rng.seed_hi);
          uint32_t byte = 0u;
#pragma unroll
          for (int i = 0; i < 4; ++i) byte |= (4 * pb + i < a.L ? sample_letter(a0, a1, a2, a3, u01(r.v[i])) : 0u) << (2 * i);
          reinterpret_cast<unsigned char*>(let)[pb] = (unsigned char)byte;
        }
      } else {
        logw = a.logw[run];
        const uint8_t* src = a.state + (size_t)run * a.L;
        for (int pb = lane; pb < a.nvb; pb += 64) {
          uint32_t byte = 0u;
#pragma unroll
          for (int i = 0; i < 4; ++i) byte |= (4 * pb + i < a.L ? (uint32_t)src[4 * pb + i] & 3u : 0u) << (2 * i);
          reinterpret_cast<unsigned char*>(let)[pb] = (unsigned char)byte;
        }
      }
      __builtin_amdgcn_wave_barrier();
#pragma unroll 1
      for (int t = a.t0; t < a.t1; ++t) {
        const float b0 = a.betas[t], b1 = a.betas[t + 1];
        // ---- weight of the step and h | v_t at betas[t+1], one hidden position per lane and round ----
        float acc = 0.f;
        for (int s = lane; s < a.Lh; s += 64) {
          const LetterWin<M> win = letter_window<M>(let, s);
#pragma unroll
          for (int strand = 0; strand <= C::DS; ++strand) {
            float z[KP], p[KP];
            conv_gather<C>(Tf, strand ? revcomp_window<M>(win) : win, z);
#pragma unroll
            for (int k = 0; k < KP; ++k) {
              const float zb = b1 * z[k];
              if (k < K) acc += softplus_of_z(zb) - softplus_of_z(b0 * z[k]);
              z[k] = zb;
            }
            uint32_t mask[NW];
            sample_hidden<C, 0>(z, gn, (uint32_t)s, KIND_AIS_H, (uint32_t)strand, a.rng, (uint32_t)(t + 1), mask, p);
            uint32_t* dst = (strand ? hmp : hm) + (size_t)(s + M - 1) * NW;
#pragma unroll
            for (int w = 0; w < NW; ++w) dst[w] = mask[w];
          }
        }
        float vs = 0.f;                                     // sum_p (c - cA)[v_p]
        for (int p = lane; p < a.L; p += 64) vs += pick((let[p >> 4] >> (2 * (p & 15))) & 3u, d0, d1, d2, d3);
        acc += (b1 - b0) * vs;
        logw += wave_sum(acc);
        __builtin_amdgcn_wave_barrier();                    // every mask of the step is stored
        // ---- v_{t+1} | h: the set-bit walk of the chain kernel over the run's mask rows ----
        const float omb = 1.0f - b1;
        const float e0 = omb * a0, e1 = omb * a1, e2 = omb * a2, e3 = omb * a3;
        for (int pb = lane; pb < a.nvb; pb += 64) {
          const int p0 = 4 * pb;
          float y[4][4];
#pragma unroll
          for (int i = 0; i < 4; ++i) { y[i][0] = m0; y[i][1] = m1; y[i][2] = m2; y[i][3] = m3; }
          constexpr int NSLOT = M + 3;
          constexpr int PPW = NW == 1 ? 64 / K : 1;         // masks per 64-bit word
          constexpr int NWORD = (NSLOT + PPW - 1) / PPW;
#pragma unroll
          for (int strand = 0; strand <= C::DS; ++strand) {
            const uint32_t* mrow = (strand ? hmp : hm) + (size_t)p0 * NW;
            const char* tab = reinterpret_cast<const char*>(smem + (strand ? C::SP_WSR : C::SP_WS));
            if constexpr (NW == 1) {
              constexpr int NMV = (NSLOT + 3) / 4;
              uint32_t m[4 * NMV];
#pragma unroll
              for (int v4 = 0; v4 < NMV; ++v4) {
                const uint4 mm = reinterpret_cast<const uint4*>(mrow)[v4];
                m[4 * v4] = mm.x; m[4 * v4 + 1] = mm.y; m[4 * v4 + 2] = mm.z; m[4 * v4 + 3] = mm.w;
              }
#pragma unroll
              for (int wi = 0; wi < NWORD; ++wi) {
                unsigned long long w = 0ull;
#pragma unroll
                for (int q = 0; q < PPW; ++q)
                  if (wi * PPW + q < NSLOT) w |= (unsigned long long)m[wi * PPW + q] << (q * K);
                topdown_bits<C>(w, tab, wi * PPW, y);
              }
            } else {
#pragma unroll 1
              for (int q = 0; q < NSLOT; ++q) {
#pragma unroll
                for (int w2 = 0; 2 * w2 < NW; ++w2) {
                  const uint32_t lo = mrow[NW * q + 2 * w2], hi = 2 * w2 + 1 < NW ? mrow[NW * q + 2 * w2 + 1] : 0u;
                  topdown_bits<C>((unsigned long long)lo | ((unsigned long long)hi << 32), tab, q, y, 64 * w2);
                }
              }
            }
          }
          const Philox4 r = philox4x32(gn, (uint32_t)pb, rng_word2(KIND_AIS_V, 0, 0, 0), (uint32_t)(t + 1), a.rng.seed_lo, a.rng.seed_hi);
          uint32_t byte = 0u;
#pragma unroll
          for (int i = 0; i < 4; ++i) {
            const uint32_t l = sample_letter(fmaf(b1, y[i][0], e0), fmaf(b1, y[i][1], e1), fmaf(b1, y[i][2], e2), fmaf(b1, y[i][3], e3),
                                             u01(r.v[i]));
            byte |= (p0 + i < a.L ? l : 0u) << (2 * i);
          }
          reinterpret_cast<unsigned char*>(let)[pb] = (unsigned char)byte;
        }
        __builtin_amdgcn_wave_barrier();                    // the next step gathers from the new letters
      }
      if (lane == 0) a.logw[run] = logw;
      if (a.state) {
        uint8_t* dst = a.state + (size_t)run * a.L;
        for (int p = lane; p < a.L; p += 64) dst[p] = (uint8_t)((let[p >> 4] >> (2 * (p & 15))) & 3u);
      }
      __builtin_amdgcn_wave_barrier();                      // the slice is cleared for the wave's next run
    }
  }
}

// ---------------------------------------------------------------------------
// Normalise the (all-reduced) raw sums and apply the SGD+momentum update
// (convRBM.py:358-371, :415-436, :440-451).
// ---------------------------------------------------------------------------
struct UpdateArgs {
  const float* sums;
  const float *W, *b, *c, *vW, *vb, *vc;      // parameters and velocities before the step
  float *oW, *ob, *oc, *ovW, *ovb, *ovc;      // ... after it (the same buffers when a single block updates in place)
  int32_t K, M, ds;
  int32_t L_data, Lf;
  int32_t data_off, n_d, model_off, n_m;   // offsets into sums
  float lr, momentum, rho, lambda_rate;
  int32_t A;                                  // letters (big_update_kernel; the specialised update is compiled for 4)
};

// `nw`: when not null, the new W, b, c are also left there ([KAM][K][4], LDS of the caller);
// `store`: whether this block writes the new parameters and velocities to global memory.
// NE: filter weights a thread may have to take (a compile-time bound on ceil(KAM / blockDim), 0 = run-time loop).
// The kernel is a chain of memory round trips (sums, parameters, velocities -> a few hundred numbers): with
// NE known the loads of all of a thread's weights are issued before the first is used -- a run-time loop
// paid one round trip per iteration (three at config #2 with 256 threads: 7.3 us for the launch).
// Sums: how element i of the packed sums is read -- PlainSums: from a.sums; RankSums (update_tables_ipc_body): the
// ranks' published copies added in rank order.
struct PlainSums {
  const float* p;
  __device__ __forceinline__ float operator()(int i) const { return p[i]; }
};
template <int NE = 0, class Sums = PlainSums>
__device__ __forceinline__ void apply_update_body(const UpdateArgs& a, float* nw, bool store, const Sums& S) {
  const int K = a.K, M = a.M, KAM = K * 4 * M;
  const float n_d = S(a.n_d), n_m = S(a.n_m);
  const float cnt_d = n_d * (float)(a.L_data - M + 1);
  const float cnt_m = n_m * (float)a.Lf;
  // offsets into the packed sums: data half [vh][vh'][h][h'][sw][sb][v], model half [vh][vh'][h][h'][v]
  const int d_vh = a.data_off, d_vhp = d_vh + KAM, d_h = d_vh + 2 * KAM, d_hp = d_h + K;
  const int d_sw = d_vh + 2 * KAM + 2 * K, d_sb = d_sw + KAM, d_v = d_sb + K;
  const int m_vh = a.model_off, m_vhp = m_vh + KAM, m_h = m_vh + 2 * KAM, m_hp = m_h + K, m_v = m_hp + K;
  const float q = a.rho;
  struct WeightIn { float dvh, mvh, dvhp, mvhp, dh, dsw, vw, w; };
  auto load_weight = [&](int idx) {
    const int k = idx / (4 * M), al = (idx / M) & 3, j = idx % M;
    const int ridx = (k * 4 + (3 - al)) * M + (M - 1 - j);
    WeightIn in;
    in.dvh = S(d_vh + idx); in.mvh = S(m_vh + idx);
    in.dvhp = a.ds ? S(d_vhp + ridx) : 0.f; in.mvhp = a.ds ? S(m_vhp + ridx) : 0.f;
    in.dh = S(d_h + k); in.dsw = S(d_sw + idx); in.vw = a.vW[idx]; in.w = a.W[idx];
    return in;
  };
  auto finish_weight = [&](int idx, const WeightIn& in) {
    float gd = in.dvh / cnt_d, gm = in.mvh / cnt_m;
    if (a.ds) {
      gd = 0.5f * (gd + in.dvhp / cnt_d);
      gm = 0.5f * (gm + in.mvhp / cnt_m);
    }
    const float p = in.dh / cnt_d;
    const float g = (q / p - (1.f - q) / (1.f - p)) / (float)K;
    const float reg = -g * in.dsw / cnt_d;
    const float v = a.momentum * in.vw + a.lr * (gd - gm - a.lambda_rate * reg);
    const float w = in.w + v;
    if (store) { a.ovW[idx] = v; a.oW[idx] = w; }
    if (nw) nw[idx] = w;
  };
  if constexpr (NE > 0) {
    WeightIn in[NE];
#pragma unroll
    for (int e = 0; e < NE; ++e) {
      const int idx = (int)threadIdx.x + e * (int)blockDim.x;
      if (idx < KAM) in[e] = load_weight(idx);
    }
#pragma unroll
    for (int e = 0; e < NE; ++e) {
      const int idx = (int)threadIdx.x + e * (int)blockDim.x;
      if (idx < KAM) finish_weight(idx, in[e]);
    }
    for (int idx = (int)threadIdx.x + NE * (int)blockDim.x; idx < KAM; idx += blockDim.x) finish_weight(idx, load_weight(idx));   // smaller blocks than assumed
  } else {
    for (int idx = threadIdx.x; idx < KAM; idx += blockDim.x) finish_weight(idx, load_weight(idx));
  }
  for (int k = threadIdx.x; k < K; k += blockDim.x) {
    const float dh = S(d_h + k);
    float gd = dh / cnt_d, gm = S(m_h + k) / cnt_m;
    if (a.ds) {
      gd = 0.5f * (gd + S(d_hp + k) / cnt_d);
      gm = 0.5f * (gm + S(m_hp + k) / cnt_m);
    }
    const float p = dh / cnt_d;
    const float g = (q / p - (1.f - q) / (1.f - p)) / (float)K;
    const float reg = -g * S(d_sb + k) / cnt_d;
    const float v = a.momentum * a.vb[k] + a.lr * (gd - gm - a.lambda_rate * reg);
    const float bn = a.b[k] + v;
    if (store) { a.ovb[k] = v; a.ob[k] = bn; }
    if (nw) nw[KAM + k] = bn;
  }
  if (threadIdx.x < 4) {
    const int al = threadIdx.x;
    const float nd = n_d * (float)a.L_data, nm = n_m * (float)(a.Lf + M - 1);
    const float gd = S(d_v + al) / nd + S(d_v + 3 - al) / nd;     // a += a[::-1]  (:345)
    const float gm = S(m_v + al) / nm + S(m_v + 3 - al) / nm;
    const float v = a.momentum * a.vc[al] + a.lr * (gd - gm);
    const float cn = a.c[al] + v;
    if (store) { a.ovc[al] = v; a.oc[al] = cn; }
    if (nw) nw[KAM + K + al] = cn;
  }
}

// The end of a training step in one launch: the update, then the LDS table images of the new
// parameters for the next step's kernels.  Every block of the grid forms the complete update for
// itself (a few hundred numbers from the packed sums) into its LDS and builds its share of the
// tables from there; block 0 also stores the new parameters and velocities -- into the OTHER set of
// buffers (the host swaps the two sets after the launch), because the remaining blocks may still be
// reading the old ones.
constexpr int UPDATE_THREADS = 1024;   // block size of the update launches of the product (the emulator uses smaller ones)
struct UpdateTablesArgs {
  UpdateArgs u;
  float* tables;     // Cfg::TABLES_ALL floats
};

template <class C>
__device__ void update_tables_body(const UpdateTablesArgs& a) {
  HIP_DYNAMIC_SHARED(float, smem);
  constexpr int KAM = C::K * 4 * C::M;
  apply_update_body<cdiv(KAM, UPDATE_THREADS) <= 8 ? cdiv(KAM, UPDATE_THREADS) : 0>(a.u, smem, blockIdx.x == 0, PlainSums{a.u.sums});
  __syncthreads();
  TablesArgs t;
  t.W = smem; t.b = smem + KAM; t.c = smem + KAM + C::K; t.out = a.tables;
  build_tables_body<C>(t);
}

// ---------------------------------------------------------------------------
// The all-reduce of a data-parallel training step WITHOUT a collective launch (an alternative to
// ncclAllReduce for the few-KB sums buffer, whose cost is pure latency).  Every rank owns a buffer that all
// ranks of the node have mapped (hipIpcOpenMemHandle): per step parity one slot of sums and one flag word per
// SOURCE rank.  A rank PUSHES: the column reduction of its step writes its packed sums into its slot of every
// rank's buffer (its own included) and then raises its flag there to the step number
// (reduce_publish_pair_kernel; publish_sums_kernel where the sums were formed in d_sums).  The update launch of
// every rank waits for the R flags in ITS OWN buffer, adds the R slots IN RANK ORDER (so every rank forms the
// bit-identical sum, and with it the bit-identical update) and goes on as update_tables_body does: no
// collective launch, no extra kernel boundary, and nothing on the critical path reads remote memory -- a
// step's traffic over xGMI is one posted copy of the sums per peer (a few KB), where pulling would have every
// block of every rank's update fetch every peer's sums and poll remote flags.
// Buffer reuse: a rank writes parity p of a peer's buffer only after its own update of the step before, which
// waited for that peer's flag of that step -- raised after the peer's update two steps back had read parity p.
// The wait is bounded in TIME (the GPU's constant-rate clock, `timeout_ticks`; the host sets it from
// CRBM_IPC_TIMEOUT_MS, default 30 s): a peer that died must not hang this GPU, and ordinary skew between the ranks'
// hosts -- a rank that uploads or evaluates while the others already wait -- must not trip it (crbm_amd.crbm.fit
// also puts a host barrier in front of every epoch's first launch).  A wait that runs out raises `status[0]`,
// which is sticky: the launch that saw it and every later one apply NO update (parameters and velocities are
// carried over unchanged, the tables stay), and the host turns the status word into an error at its next
// synchronisation point (CRBM_ERR_IPC_TIMEOUT) -- the run fails with the last consistent model instead of going on
// with sums that never arrived.
// ---------------------------------------------------------------------------
constexpr int IPC_MAX_RANKS = 8;
struct IpcArgs {
  const float* sums[IPC_MAX_RANKS];       // the slots of this step's parity in THIS rank's buffer, one per source rank
  const uint32_t* flags[IPC_MAX_RANKS];   // ... and their flag words: == expect once a source's sums are complete
  uint32_t* status;                       // [0] != 0: a wait timed out (sticky)
  uint32_t expect;
  int32_t nranks, count;
  unsigned long long timeout_ticks;       // of realtime_ticks()
};
struct UpdateIpcArgs {
  UpdateTablesArgs ut;
  IpcArgs ipc;
};

// element i of the all-reduced sums: the R published copies added IN RANK ORDER (every rank forms the same fp32
// sum); all loads of an element are in flight together, nothing is staged in LDS
struct RankSums {
  const IpcArgs* ipc;
  __device__ __forceinline__ float operator()(int i) const {
    float v[IPC_MAX_RANKS];
#pragma unroll
    for (int r = 0; r < IPC_MAX_RANKS; ++r) v[r] = r < ipc->nranks ? load_system(ipc->sums[r] + i) : 0.f;
    float t = v[0];
#pragma unroll
    for (int r = 1; r < IPC_MAX_RANKS; ++r) t += v[r];          // the zeros of absent ranks change nothing
    return t;
  }
};

template <class C>
__device__ void update_tables_ipc_body(const UpdateIpcArgs& a) {
  HIP_DYNAMIC_SHARED(float, smem);
  constexpr int KAM = C::K * 4 * C::M;
  const IpcArgs& ipc = a.ipc;
  float* nw = smem;                                                       // the new W, b, c
  uint32_t* gave_up = reinterpret_cast<uint32_t*>(smem + KAM + C::K + 4);   // this block does not apply the step
  if (threadIdx.x == 0) *gave_up = load_system(ipc.status);              // an earlier launch timed out: sticky
  __syncthreads();
  if ((int)threadIdx.x < ipc.nranks && *gave_up == 0u) {
    const uint32_t* f = ipc.flags[threadIdx.x];
    const uint64_t t0 = realtime_ticks();
    while ((int32_t)(load_system(f) - ipc.expect) < 0) {                  // flags only grow (step numbers)
      if (realtime_ticks() - t0 > ipc.timeout_ticks) {
        store_system(ipc.status, 1u);
        atomicOr(gave_up, 1u);
        break;
      }
      short_sleep();
    }
    fence_acquire_system();                                               // the sums behind the flag, not an older copy
  }
  __syncthreads();
  const UpdateArgs& u = a.ut.u;
  if (*gave_up != 0u) {
    // the host has already made the other buffer set the current one: carry the state over unchanged
    if (blockIdx.x == 0) {
      for (int i = threadIdx.x; i < KAM; i += blockDim.x) { u.oW[i] = u.W[i]; u.ovW[i] = u.vW[i]; }
      for (int i = threadIdx.x; i < C::K; i += blockDim.x) { u.ob[i] = u.b[i]; u.ovb[i] = u.vb[i]; }
      if (threadIdx.x < 4) { u.oc[threadIdx.x] = u.c[threadIdx.x]; u.ovc[threadIdx.x] = u.vc[threadIdx.x]; }
    }
    return;
  }
  apply_update_body<cdiv(KAM, UPDATE_THREADS) <= 8 ? cdiv(KAM, UPDATE_THREADS) : 0>(u, nw, blockIdx.x == 0, RankSums{&ipc});
  __syncthreads();
  TablesArgs t;
  t.W = nw; t.b = nw + KAM; t.c = nw + KAM + C::K; t.out = a.ut.tables;
  build_tables_body<C>(t);
}

// sums[dst(r)] = sum over partial rows of column r in a fixed order.  Block =
// 32 columns x (blockDim / 32) row groups: each thread adds the rows of its group (128-byte
// segments per row), the 32 groups are combined through LDS.  The partial
// buffer is never cleared: the kernel knows which column classes a statistics
// launch wrote and yields 0 for the classes that launch did not compute.
struct ReduceArgs {
  const float* partials;
  float* sums;
  int32_t nrows, row;
  int32_t K, KAM, ds, want_sparsity;
  int32_t skip_begin, skip_len;   // columns [skip_begin, skip_begin+skip_len) are dropped
  float n_value;                  // written after the last kept column
};

// Where a pushing rank's sums go: the same offset in its slot of every rank's buffer (byte distances from the
// rank's own buffer, which ReduceArgs::sums points into; own = 0)
struct PushTargets {
  int32_t n;
  long long delta[8];
};
__device__ __forceinline__ void push_store(float* own, const PushTargets& t, float v) {
#pragma unroll
  for (int r = 0; r < 8; ++r)
    if (r < t.n) store_system(reinterpret_cast<float*>(reinterpret_cast<char*>(own) + t.delta[r]), v);
}

// SYSTEM: the sums go out with system-scope stores into the buffers the ranks of a node have mapped
// (reduce_publish_pair_kernel)
template <bool SYSTEM = false>
__device__ __forceinline__ void reduce_partials_body(const ReduceArgs& a, const PushTargets* push = nullptr) {
  __shared__ float part[32][33];
  const int col = threadIdx.x & 31, grp = threadIdx.x >> 5;
  const int ngrp = (int)(blockDim.x >> 5);          // 32 row groups in the 1024-thread launches of the product
  const int r = blockIdx.x * 32 + col;
  float tsum = 0.f;
  if (r < a.row) {
    // column classes of a partial row: [vh KAM][vh' KAM][h K][h' K][sw KAM][sb K][v 4]
    const int K = a.K, KAM = a.KAM;
    bool valid;
    if (r < KAM) valid = true;
    else if (r < 2 * KAM) valid = a.ds != 0;
    else if (r < 2 * KAM + K) valid = true;
    else if (r < 2 * KAM + 2 * K) valid = a.ds != 0;
    else if (r < 3 * KAM + 3 * K) valid = a.want_sparsity != 0;
    else valid = true;
    if (valid) {
      // eight rows in flight per thread (the kernel is a chain of memory round trips: ~2 000 rows of a few KB;
      // sixteen in flight measured slower, 5.1 -> 5.7 us); fixed order
      float t0 = 0.f, t1 = 0.f, t2 = 0.f, t3 = 0.f, t4 = 0.f, t5 = 0.f, t6 = 0.f, t7 = 0.f;
      int i = grp;
      for (; i + 7 * ngrp < a.nrows; i += 8 * ngrp) {
        const float v0 = a.partials[(size_t)i * a.row + r], v1 = a.partials[(size_t)(i + ngrp) * a.row + r];
        const float v2 = a.partials[(size_t)(i + 2 * ngrp) * a.row + r], v3 = a.partials[(size_t)(i + 3 * ngrp) * a.row + r];
        const float v4 = a.partials[(size_t)(i + 4 * ngrp) * a.row + r], v5 = a.partials[(size_t)(i + 5 * ngrp) * a.row + r];
        const float v6 = a.partials[(size_t)(i + 6 * ngrp) * a.row + r], v7 = a.partials[(size_t)(i + 7 * ngrp) * a.row + r];
        t0 += v0; t1 += v1; t2 += v2; t3 += v3; t4 += v4; t5 += v5; t6 += v6; t7 += v7;
      }
      for (; i < a.nrows; i += ngrp) t0 += a.partials[(size_t)i * a.row + r];
      tsum = ((t0 + t1) + (t2 + t3)) + ((t4 + t5) + (t6 + t7));
    }
  }
  part[grp][col] = tsum;
  __syncthreads();
  if (grp == 0 && r < a.row) {
    const bool skipped = r >= a.skip_begin && r < a.skip_begin + a.skip_len;
    if (!skipped) {
      float s = 0.f;
      for (int g = 0; g < ngrp; ++g) s += part[g][col];
      float* dst = a.sums + (r < a.skip_begin ? r : r - a.skip_len);
      if (SYSTEM) push_store(dst, *push, s); else *dst = s;
    }
  }
  if (blockIdx.x == 0 && threadIdx.x == 0) {
    if (SYSTEM) push_store(a.sums + (a.row - a.skip_len), *push, a.n_value); else a.sums[a.row - a.skip_len] = a.n_value;
  }
}


// both halves of a training step in one launch (blockIdx.y = 0: data, 1: model)
struct ReducePair {
  ReduceArgs half[2];
};

// ===========================================================================
// A model as a row of SLABS of the kernels' model (crbm_api.hip: slab_launch_stats, slab_launch_hgv -- generic DNA
// models take their statistics and the h|v of their chains from the specialised kernels, Ks motifs at a time).  One launch
// serves all slabs: blockIdx.y is the slab, whose table image, partial rows and first motif follow from it; the bodies
// above run unchanged (they look at blockIdx.x only).
// ===========================================================================
struct SlabPlan {
  int32_t Ks, K, last_k0;     // motifs per slab, motifs of the model, first motif of the last slab (it may overlap its neighbour)
};
__device__ __forceinline__ int slab_k0(const SlabPlan& p, int y) { return (y + 1) * p.Ks <= p.K ? y * p.Ks : p.last_k0; }
// Slab y owns motifs [k0 + kskip, k0 + kend) of the model, [kskip, kend) of its kernel: those below kskip belong to the
// neighbouring slab as well and are reported there; those from kend on lie past the model.
struct SlabSpan {
  int k0, kskip, kend;
};
template <class C>
__device__ __forceinline__ SlabSpan slab_span(const SlabPlan& p, int y) {
  SlabSpan s;
  s.k0 = slab_k0(p, y);
  s.kskip = y > 0 ? max(0, slab_k0(p, y - 1) + p.Ks - s.k0) : 0;
  s.kend = min(C::K, p.K - s.k0);      // (C::K == p.Ks)
  return s;
}
// What every stream kernel reads (scan_sites_body, scan_hist_body): one segment of a stream as scan_encode_kernel left
// it (crbm_layout.h, scan_layout) and the model's slabs.  Filled in one place per driver (crbm_api.hip, StreamSweep);
// 48 bytes, no padding: it travels by value as the base of the kernels' argument structs.
struct ScanInput {
  const float* tables;                 // the first slab's image
  const uint32_t* letters;
  const unsigned long long* valid;
  int32_t starts, tiles;               // window starts of the segment, tiles of 64 of them
  int32_t table_stride;                // floats
  SlabPlan plan;
};
static_assert(sizeof(ScanInput) == 48, "ScanInput has no padding");
// all M validity bits from window start s on (the plane has two zero words behind: s >> 6 and the next one are inside)
template <int M>
__device__ __forceinline__ bool window_valid(const unsigned long long* valid, int s) {
  const int sh = s & 63;
  const unsigned long long v0 = valid[s >> 6], v1 = valid[(s >> 6) + 1];
  const unsigned long long v = sh ? (v0 >> sh) | (v1 << (64 - sh)) : v0;
  const unsigned long long need = M < 64 ? (1ull << M) - 1ull : ~0ull;
  return (v & need) == need;
}

struct SlabTablesArgs {
  TablesArgs t;               // W, b of the whole model; out: the first slab's image
  SlabPlan plan;
  int32_t stride;             // floats between the images of consecutive slabs
};
template <class C>
__device__ void slab_tables_body(const SlabTablesArgs& s) {
  TablesArgs a = s.t;
  const int k0 = slab_k0(s.plan, (int)blockIdx.y);
  a.W += (size_t)k0 * 4 * C::M;
  a.b += k0;
  a.out += (size_t)blockIdx.y * s.stride;
  build_tables_body<C>(a);
}

struct SlabStatsArgs {
  StatsMfmaArgs a;            // tables, partial rows: the first slab's
  int32_t table_stride;       // floats
  int32_t pad_;
  long long partial_stride;   // floats between the partial rows of consecutive slabs
};
template <class C, bool SP, bool BYTE_LUT>
__device__ void slab_stats_body(const SlabStatsArgs& s) {
  StatsMfmaArgs a = s.a;
  a.tables += (size_t)blockIdx.y * s.table_stride;
  a.sg.partials += (size_t)blockIdx.y * s.partial_stride;
  stats_mfma_body<C, SP, BYTE_LUT>(a);
}

struct SlabHgvArgs {
  HgvMasksArgs m;             // k0, kskip, group0 are filled in per slab
  SlabPlan plan;
  int32_t table_stride;       // floats
};
template <class C>
__device__ void slab_hgv_body(const SlabHgvArgs& s) {
  HgvMasksArgs ma = s.m;
  const int y = (int)blockIdx.y;
  const SlabSpan span = slab_span<C>(s.plan, y);
  ma.g.tables += (size_t)y * s.table_stride;
  ma.k0 = span.k0;
  ma.group0 = (uint32_t)(span.k0 / 10);
  ma.kskip = span.kskip;               // units the neighbouring slab counts
  hgv_masks_body<C>(ma);
}

// free energy: the per-motif terms -v_k - cs of every slab (free_energy_body's `fem`) into a scratch [slab][n][Ks];
// slab_fe_combine_kernel (crbm_kernels_generic.h) puts them together
struct SlabFeArgs {
  FeArgs a;                   // fe unused; fem: the first slab's scratch
  int32_t table_stride;       // floats
  int32_t pad_;
  long long fem_stride;       // floats between the scratch of consecutive slabs
};
template <class C>
__device__ void slab_fe_body(const SlabFeArgs& s) {
  FeArgs a = s.a;
  a.tables += (size_t)blockIdx.y * s.table_stride;
  a.fem += (size_t)blockIdx.y * s.fem_stride;
  a.fe = nullptr;
  free_energy_body<C>(a);
}

// ===========================================================================
// Stream scan (crbm_scan_sites_codes): the sites of a 1-D stream of letters in which some positions hold no letter.
// A window [s, s + M) is valid when all of its M positions hold letters; a valid window scores exactly like the same
// M letters in a row of motif_sites_body (both score through window_strand_z: the same bits); an invalid one
// yields nothing.  The segment arrives as 2-bit letter words and a validity plane (crbm_layout.h, scan_layout;
// scan_encode_kernel).  A block keeps the gather table in LDS; a wave walks tiles of 64 window starts, a lane owns one.
// Records leave the device in their final order -- (start, motif, strand), + before - -- in two passes of this body:
//   pass 0  a lane counts its hits over all motifs and strands (lane_cnt) and the wave adds the counts up (tile_cnt);
//           scan_offsets_kernel then turns the tile counts into exclusive offsets and the total;
//   pass 1  the waves of tiles that have hits score them again; a lane writes its records one after the other from
//           tile offset + (counts of the lower lanes) on, those below `capacity`.
// No reservation atomics, no float combined across threads: the same bits in every run and for every geometry.
// blockIdx.y is the slab of a generic DNA model (its table image, its motifs [k0 + kskip, min(k0 + Ks, K)), its part of
// every buffer); a model on its own kernels is one slab of all its motifs.
// ===========================================================================
struct ScanArgs : ScanInput {
  unsigned short* lane_cnt;            // [slab][64 * tiles]
  uint32_t* tile_cnt;                  // [slab][tiles]
  const unsigned long long* tile_off;  // [slab][tiles], pass 1
  SiteRec* recs;                       // [slab][capacity], pass 1
  unsigned long long capacity;         // records per slab
  int32_t pos0;                        // stream position of the segment's first letter
  int32_t pass;
  float threshold;
  int32_t pad_;
};
// sum over the wave and over the lower lanes of a small per-lane count (< 2^BITS), bit plane by bit plane (all lanes call it)
template <int BITS>
__device__ __forceinline__ void wave_count_sums(uint32_t c, uint32_t& below, uint32_t& total) {
  below = 0; total = 0;
#pragma unroll
  for (int b = 0; b < BITS; ++b) {
    const unsigned long long m = __ballot((c >> b) & 1u);
    below += lanes_below(m) << b;
    total += (uint32_t)__popcll(m) << b;
  }
}

template <class C>
__device__ void scan_sites_body(const ScanArgs& a) {
  if constexpr (C::POOL == 1) {       // pool groups have no anchor in a stream: refused on the host, no body
    constexpr int M = C::M, S = C::DS ? 2 : 1;
    constexpr int NQW = C::NQ < 4 ? C::NQ : 4, NV = 4 * NQW;
    static_assert(C::K * S < (1 << 10), "a lane's count must fit ten bits");
    HIP_DYNAMIC_SHARED(float, smem);
    float* Tf = smem;
    const ScanInput& in = a;
    const int y = (int)blockIdx.y;
    const SlabSpan span = slab_span<C>(in.plan, y);
    copy_tables<C::TAB>(Tf, in.tables + (size_t)y * in.table_stride + C::OFF_TF);
    __syncthreads();
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, nwaves = blockDim.x >> 6;
    const float thr = a.threshold;
    unsigned short* lane_cnt = a.lane_cnt + (size_t)y * 64 * in.tiles;
    uint32_t* tile_cnt = a.tile_cnt + (size_t)y * in.tiles;
    // p[] = the scores of motifs [4 q0, 4 q0 + NV) of the window on `strand`
    auto scores = [&](const LetterWin<M>& w, int q0, int strand, float (&p)[NV]) {
      float z[NV];
      window_strand_z<C, NQW>(Tf, w, q0, strand, z);
#pragma unroll
      for (int j = 0; j < NV; ++j) p[j] = sigmoid_z(z[j]);
    };
    auto is_hit = [&](int kk, float p) { return kk >= span.kskip && kk < span.kend && p >= thr; };
    for (int t = blockIdx.x * nwaves + wave; t < in.tiles; t += gridDim.x * nwaves) {
      const int s = 64 * t + lane;
      if (a.pass == 0) {
        const bool ok = s < in.starts && window_valid<M>(in.valid, s);
        uint32_t c = 0;
        if (ok) {
          const LetterWin<M> w = letter_window<M>(in.letters, s);
#pragma unroll 1
          for (int q0 = 0; q0 < C::NQ; q0 += NQW)
#pragma unroll 1
            for (int strand = 0; strand < S; ++strand) {
              float p[NV];
              scores(w, q0, strand, p);
#pragma unroll
              for (int j = 0; j < NV; ++j) c += is_hit(4 * q0 + j, p[j]) ? 1u : 0u;
            }
        }
        lane_cnt[s] = (unsigned short)c;   // (the buffer holds whole tiles)
        uint32_t below, total;
        wave_count_sums<10>(c, below, total);
        if (lane == 0) tile_cnt[t] = total;
      } else {
        if (tile_cnt[t] == 0) continue;                     // wave-uniform
        const uint32_t c = lane_cnt[s];
        uint32_t below, total;
        wave_count_sums<10>(c, below, total);
        unsigned long long idx = a.tile_off[(size_t)y * in.tiles + t] + below;
        SiteRec* recs = a.recs + (size_t)y * a.capacity;
        const LetterWin<M> w = letter_window<M>(in.letters, s);
#pragma unroll 1
        for (int q0 = 0; q0 < (c ? C::NQ : 0); q0 += NQW) {   // lanes without hits sit the tile out
          float p[S][NV];
          scores(w, q0, 0, p[0]);
          if constexpr (S == 2) scores(w, q0, 1, p[1]);
#pragma unroll
          for (int j = 0; j < NV; ++j)
#pragma unroll
            for (int strand = 0; strand < S; ++strand)
              if (is_hit(4 * q0 + j, p[strand][j])) {
                if (idx < a.capacity) {
                  SiteRec* d = recs + idx;
                  d->seq = 0; d->motif = span.k0 + 4 * q0 + j; d->start = a.pos0 + s;
                  d->strand = C::DS ? (strand ? -1 : 1) : 0; d->prob = p[strand][j];
                }
                ++idx;
              }
        }
      }
    }
  }
}

// ===========================================================================
// Score histogram (crbm_scan_histogram_codes): the stream scan with a histogram per (motif, strand) in place of records.
// Same input (ScanInput), tiles and slabs as scan_sites_body; the score of a valid window is the log-odds
// x = x_of_z(z) of the z the scan scores with (window_strand_z; single-stranded models: z summed over both
// orientations, one strand), so that sigmoid(x) is the probability the scan reports.
// THE BIN RULE: t = (x - lo) * inv_w with inv_w = nbins / (hi - lo) formed on the host in fp32; the bin is 0 for
// t < 0, nbins - 1 for t >= nbins, (int)t otherwise -- the first bin holds everything below lo, the last everything at
// or above hi.  (A NaN score, which finite parameters cannot produce, would land in bin 0.)
// Counts go into 32-bit LDS counters behind the gather table -- a block sees fewer than 2^31 starts per segment -- for
// `gq` motif quads at a time: groups of quads in the outer loop, tiles in the inner one, the non-zero counters of a
// group added to hist [K][S][nbins] with 64-bit integer atomics before the next group starts.  Integer adds only: the
// same bits for every geometry, segment size and run.  hist[K * S * nbins] receives the number of valid windows,
// counted by slab 0 on its first group.
// The 64 lanes of a wave score the same motif at the same moment, and background scores cluster in few bins:
//   variant 0  every lane walks the motifs of a gather in order, one counter set per block;
//   variant 1  lane l starts at motif l mod NV (a select tree over the NV counter addresses per step);
//   variant 2  as 0 with `copies` counter sets, wave w adds into set w mod copies.
// ===========================================================================
struct ScanHistArgs : ScanInput {
  unsigned long long* hist;            // [K][S][nbins], then the valid windows
  int32_t nbins;
  int32_t gq;                          // motif quads whose counters the LDS holds: a multiple of the gather's quads, or fewer
  int32_t copies;                      // counter sets (variant 2; else 1)
  int32_t rotate;                      // variant 1
  float lo, inv_w;
};
// v[j] for a lane-dependent j in [0, N): a tree of selects, no indexed register access
template <int N>
__device__ __forceinline__ int select_entry(const int (&v)[N], int j) {
  constexpr int P2 = N <= 4 ? 4 : N <= 8 ? 8 : 16;
  static_assert(N <= 16, "a gather holds at most 16 motifs");
  int t[P2];
#pragma unroll
  for (int i = 0; i < P2; ++i) t[i] = i < N ? v[i] : -1;
#pragma unroll
  for (int bit = 0; (1 << bit) < P2; ++bit) {
    const bool odd = (j >> bit) & 1;
#pragma unroll
    for (int m = 0; m < (P2 >> (bit + 1)); ++m) t[m] = odd ? t[2 * m + 1] : t[2 * m];
  }
  return t[0];
}

template <class C>
__device__ void scan_hist_body(const ScanHistArgs& a) {
  if constexpr (C::POOL == 1) {       // refused on the host, as the scan
    constexpr int M = C::M, S = C::DS ? 2 : 1;
    constexpr int NQW = C::NQ < 4 ? C::NQ : 4, NV = 4 * NQW;
    HIP_DYNAMIC_SHARED(float, smem);
    float* Tf = smem;
    uint32_t* cnt = reinterpret_cast<uint32_t*>(smem + C::TAB);    // [copies][4 gq][S][nbins], then the block's valid windows
    const ScanInput& in = a;
    const int y = (int)blockIdx.y;
    const SlabSpan span = slab_span<C>(in.plan, y);
    const int nb = a.nbins, row = S * nb, per = 4 * a.gq * row;    // counters of a motif, of a counter set
    uint32_t* wcnt = cnt + (size_t)a.copies * per;
    copy_tables<C::TAB>(Tf, in.tables + (size_t)y * in.table_stride + C::OFF_TF);
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, nwaves = blockDim.x >> 6;
    uint32_t* mine = cnt + (size_t)(wave % a.copies) * per;
    const float lo = a.lo, inv_w = a.inv_w, nbf = (float)nb;
    const int r0 = lane % NV;
    for (int g0 = 0; g0 < C::NQ; g0 += a.gq) {
      const int g1 = min(g0 + a.gq, C::NQ);
      for (int i = threadIdx.x; i < a.copies * per + (g0 == 0 ? 1 : 0); i += blockDim.x) cnt[i] = 0u;
      __syncthreads();                 // (the first one also stands behind copy_tables)
      for (int t = blockIdx.x * nwaves + wave; t < in.tiles; t += gridDim.x * nwaves) {
        const int s = 64 * t + lane;
        const bool ok = s < in.starts && window_valid<M>(in.valid, s);
        if (g0 == 0 && y == 0) {       // wave-uniform
          const unsigned long long m = __ballot(ok);
          if (lane == 0 && m) atomicAdd(wcnt, (uint32_t)__popcll(m));
        }
        if (!ok) continue;
        const LetterWin<M> w = letter_window<M>(in.letters, s);
#pragma unroll 1
        for (int q0 = (g0 / NQW) * NQW; q0 < g1; q0 += NQW)
#pragma unroll 1
          for (int strand = 0; strand < S; ++strand) {
            float z[NV];
            window_strand_z<C, NQW>(Tf, w, q0, strand, z);
            int at[NV];                // the counter of motif 4 q0 + j, -1: not this block's, or not resident
#pragma unroll
            for (int j = 0; j < NV; ++j) {
              const int kk = 4 * q0 + j, qq = q0 + j / 4;
              const float tb = (x_of_z(z[j]) - lo) * inv_w;
              const int bin = !(tb >= 0.f) ? 0 : tb >= nbf ? nb - 1 : (int)tb;
              const bool live = kk >= span.kskip && kk < span.kend && qq >= g0 && qq < g1;
              at[j] = live ? ((kk - 4 * g0) * S + strand) * nb + bin : -1;
            }
            if (a.rotate) {
#pragma unroll
              for (int i = 0; i < NV; ++i) {
                const int jj = i + r0 < NV ? i + r0 : i + r0 - NV;
                const int ad = select_entry<NV>(at, jj);
                if (ad >= 0) atomicAdd(mine + ad, 1u);
              }
            } else {
#pragma unroll
              for (int j = 0; j < NV; ++j)
                if (at[j] >= 0) atomicAdd(mine + at[j], 1u);
            }
          }
      }
      __syncthreads();
      for (int i = threadIdx.x; i < per; i += blockDim.x) {
        uint32_t c = 0;
        for (int set = 0; set < a.copies; ++set) c += cnt[(size_t)set * per + i];
        if (c) atomicAdd(a.hist + (size_t)(span.k0 + 4 * g0) * row + i, (unsigned long long)c);   // (counters of motifs past kend stay 0)
      }
      __syncthreads();
    }
    if (threadIdx.x == 0 && y == 0 && *wcnt) atomicAdd(a.hist + (size_t)in.plan.K * row, (unsigned long long)*wcnt);
  }
}

// ===========================================================================
// Variant effects (crbm_variant_effects_codes): what one substitution changes in the free energy of a stream, per motif.
// The host gathers the context [pos - M + 1, pos + M - 1] of every variant of a chunk, CW = 2M - 1 codes with 4 for the
// positions outside the stream; the contexts back to back are a stream of cnt * CW codes that scan_encode_kernel turns
// into the letters and the validity plane of scan_layout.  The windows that cover variant v's letter start at
// s = v * CW + m, m in [0, M), and none of them reaches into a neighbour's context: a variant sees its own context alone.
// A wave owns a tile of 64 variants, a lane one of them.  The lane walks its M windows in ascending m, + strand before
// -, for NQW motif quads at a time (the outer loop): z of the window as free_energy_body gathers it (conv_gather_quads
// per strand, strand <= DS -- NOT window_strand_z's site score), then mutagenesis_body's one other table row: the
// variant's letter sits at offset o = strand ? m : M - 1 - m of the strand's window, in group g = o / G at slot t, and
// T[g][r ^ (x << 2t)] - T[g][r] with x = ref ^ alt is what the substitution adds to z (complementing commutes with
// ^ x: the same x on both strands).  m, g and t are wave-uniform; x and the rows differ between lanes.  The differences
// softplus(z_alt) - softplus(z_ref) of the valid windows are subtracted from the lane's registers acc[] (F carries
// -softplus) in that fixed order and stored to per_motif [cnt][K]: no cross-lane sum, no atomics, no LDS accumulator --
// a variant's bits depend on its context alone, not on the chunk, its place in the list or the launch geometry.
// alt == ref: x = 0, the same row twice, exactly 0.  ref no letter: no window is valid, all 0.
// blockIdx.y is the slab of a generic DNA model, which writes its own columns [k0 + kskip, k0 + kend); slab 0 counts the
// valid windows.  variant_combine_kernel (below, model-independent) sums a row in ascending k and adds the bias term.
// ===========================================================================
struct VariantArgs : ScanInput {         // starts = cnt * CW - M + 1 (unused), tiles = tiles of 64 VARIANTS
  const unsigned char* alt;              // [cnt] codes 0..3
  float* per_motif;                      // [cnt][K]
  int32_t* windows;                      // [cnt]
  int32_t cnt;
  int32_t pad_;
};

template <class C>
__device__ void variant_effects_body(const VariantArgs& a) {
  if constexpr (C::POOL == 1) {       // refused on the host, as the scan
    constexpr int K = C::K, M = C::M, G = C::G, CW = 2 * M - 1;
    constexpr int NQW = C::NQ < 4 ? C::NQ : 4, NV = 4 * NQW;
    HIP_DYNAMIC_SHARED(float, smem);
    float* Tf = smem;
    const ScanInput& in = a;
    const int y = (int)blockIdx.y;
    const SlabSpan span = slab_span<C>(in.plan, y);
    copy_tables<C::TAB>(Tf, in.tables + (size_t)y * in.table_stride + C::OFF_TF);
    __syncthreads();
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, nwaves = blockDim.x >> 6;
    for (int t = blockIdx.x * nwaves + wave; t < in.tiles; t += gridDim.x * nwaves) {
      const int v = 64 * t + lane;
      const bool live = v < a.cnt;
      const int base = (live ? v : a.cnt - 1) * CW;          // (idle lanes of the last tile repeat its last variant)
      const int p = base + M - 1;                            // the variant's own position: letter 0 under a code 4, where
      const uint32_t ref = (in.letters[p >> 4] >> (2 * (p & 15))) & 3u;   // no window is valid and x does not matter
      const uint32_t x = ref ^ (uint32_t)(a.alt[live ? v : a.cnt - 1] & 3u);
      int nwin = 0;
#pragma unroll 1
      for (int q0 = 0; q0 < C::NQ; q0 += NQW) {
        float acc[NV];
#pragma unroll
        for (int j = 0; j < NV; ++j) acc[j] = 0.f;
#pragma unroll 1
        for (int m = 0; m < M; ++m) {
          const int s = base + m;
          const bool ok = window_valid<M>(in.valid, s);
          if (q0 == 0) nwin += ok ? 1 : 0;
          const LetterWin<M> fwd = letter_window<M>(in.letters, s);
#pragma unroll 1
          for (int strand = 0; strand <= C::DS; ++strand) {
            const LetterWin<M> win = strand ? revcomp_window<M>(fwd) : fwd;
            float z[NV];
            conv_gather_quads<C, NQW>(Tf, win, q0, z);
            const int o = strand ? m : M - 1 - m;            // the variant's letter in this strand's window
            const int g = o / G, tt = o - g * G;
            const uint32_t r = window_bits<M>(win, 2 * G * g) & (uint32_t)(C::ROWS - 1);
            const uint32_t r2 = r ^ (x << (2 * tt));
            const float4* tab = reinterpret_cast<const float4*>(Tf + (size_t)g * C::ROWS * C::KP) + q0;
#pragma unroll
            for (int q = 0; q < NQW; ++q)
              if (q0 + q < C::NQ) {                          // wave-uniform
                const float4 cv = tab[(size_t)r * C::NQ + q], av = tab[(size_t)r2 * C::NQ + q];
                const float cur[4] = {cv.x, cv.y, cv.z, cv.w}, alt[4] = {av.x, av.y, av.z, av.w};
#pragma unroll
                for (int e = 0; e < 4; ++e)
                  if (4 * (q0 + q) + e < K) {
                    const float d = softplus_of_z(z[4 * q + e] + (alt[e] - cur[e])) - softplus_of_z(z[4 * q + e]);
                    if (ok) acc[4 * q + e] -= d;
                  }
              }
          }
        }
        if (live) {
          float* out = a.per_motif + (size_t)v * in.plan.K + span.k0;
#pragma unroll
          for (int j = 0; j < NV; ++j) {
            const int kk = 4 * q0 + j;
            if (kk >= span.kskip && kk < span.kend) out[kk] = acc[j];
          }
        }
      }
      if (live && y == 0) a.windows[v] = nwin;
    }
  }
}

// ===========================================================================
// Allele effects (crbm_allele_effects_codes): what replacing R codes of a stream by A letters -- an insertion, a
// deletion, a block substitution -- changes in its free energy, per motif.  The host stages both haplotypes of every
// variant of a chunk back to back (crbm_sweep.h, gather_haplotypes; crbm_layout.h, AlleleEntry) and
// scan_encode_kernel makes letters and validity plane of them.  refhap has R + M - 1 window starts from `off` on,
// althap A + M - 1 from off + R + 2M - 2 on: the last window of a haplotype ends on its last code, so none reaches into
// a neighbour.  The number of windows differs from variant to variant (M - 1 .. 65535 + M - 1), so a WAVE owns a
// variant: lane l takes windows l, l + 64, ... of a haplotype in ascending order, + strand before -, z as
// free_energy_body gathers it (conv_gather_quads per strand, strand <= DS), softplus added into the lane's registers
// for NQW motif quads at a time (the outer loop); wave_sum adds the 64 lanes in its fixed tree; lane 0 writes
// S_ref - S_alt = -(S_alt - S_ref).  Lane assignment and tree depend on the variant alone: no atomics, no LDS
// accumulator, the same bits for every chunk, place in the list and launch geometry.  A `zero` variant scores nothing
// and gets zeros.  blockIdx.y is the slab of a generic DNA model, which writes its own columns; slab 0 writes the valid
// windows [cnt][2].  allele_combine_kernel (below, model-independent) forms dfe.
// ===========================================================================
struct AlleleArgs : ScanInput {          // starts = staged codes (unused), tiles unused
  const AlleleEntry* table;              // [cnt]
  float* per_motif;                      // [cnt][K]
  int32_t* windows;                      // [cnt][2]
  int32_t cnt;
  int32_t pad_;
};

template <class C>
__device__ void allele_effects_body(const AlleleArgs& a) {
  if constexpr (C::POOL == 1) {       // refused on the host, as the scan
    constexpr int K = C::K, M = C::M;
    constexpr int NQW = C::NQ < 4 ? C::NQ : 4, NV = 4 * NQW;
    HIP_DYNAMIC_SHARED(float, smem);
    float* Tf = smem;
    const ScanInput& in = a;
    const int y = (int)blockIdx.y;
    const SlabSpan span = slab_span<C>(in.plan, y);
    copy_tables<C::TAB>(Tf, in.tables + (size_t)y * in.table_stride + C::OFF_TF);
    __syncthreads();
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, nwaves = blockDim.x >> 6;
    // sum[] = the wave's softplus sums of motifs [4 q0, 4 q0 + NV) over the valid ones of the n windows from `off` on;
    // returns their number (all lanes call it: wave-uniform trip counts)
    auto hap_sums = [&](int off, int n, int q0, float (&sum)[NV]) -> int {
      float acc[NV];
#pragma unroll
      for (int j = 0; j < NV; ++j) acc[j] = 0.f;
      int nwin = 0;
#pragma unroll 1
      for (int w0 = 0; w0 < n; w0 += 64) {
        const int w = w0 + lane;
        const bool ok = w < n && window_valid<M>(in.valid, off + w);
        nwin += __popcll(__ballot(ok));
        if (ok) {
          const LetterWin<M> fwd = letter_window<M>(in.letters, off + w);
#pragma unroll 1
          for (int strand = 0; strand <= C::DS; ++strand) {
            float z[NV];
            conv_gather_quads<C, NQW>(Tf, strand ? revcomp_window<M>(fwd) : fwd, q0, z);
#pragma unroll
            for (int j = 0; j < NV; ++j)
              if (4 * q0 + j < K) acc[j] += softplus_of_z(z[j]);
          }
        }
      }
#pragma unroll
      for (int j = 0; j < NV; ++j) sum[j] = wave_sum(acc[j]);
      return nwin;
    };
    for (int v = blockIdx.x * nwaves + wave; v < a.cnt; v += gridDim.x * nwaves) {
      const AlleleEntry e = a.table[v];
      const int n0 = e.zero ? 0 : e.R + M - 1, n1 = e.zero ? 0 : e.A + M - 1;
      const int off1 = e.off + e.R + 2 * (M - 1);
      float* out = a.per_motif + (size_t)v * in.plan.K + span.k0;
      int nwin0 = 0, nwin1 = 0;
#pragma unroll 1
      for (int q0 = 0; q0 < C::NQ; q0 += NQW) {
        float sref[NV], salt[NV];
        nwin0 = hap_sums(e.off, n0, q0, sref);
        nwin1 = hap_sums(off1, n1, q0, salt);
        if (lane == 0) {
#pragma unroll
          for (int j = 0; j < NV; ++j) {
            const int kk = 4 * q0 + j;
            if (kk >= span.kskip && kk < span.kend) out[kk] = sref[j] - salt[j];
          }
        }
      }
      if (lane == 0 && y == 0) {
        a.windows[2 * (size_t)v] = nwin0;
        a.windows[2 * (size_t)v + 1] = nwin1;
      }
    }
  }
}

// ===========================================================================
// Record summaries (crbm_scan_records_codes): per record of a stream -- records are separated by one code 4, rec_start
// holds their first positions and T + 1 behind them (sequences.seqsToStream) -- the valid windows, the letter counts,
// per motif the free-energy sum over the record's valid windows and the best site.  A window, and a letter, belongs to
// the record its position lies in; a separator belongs to the record in front of it and contributes nothing.
//   free energy  z as free_energy_body gathers it (conv_gather_quads per strand, strand <= DS; for a double-stranded
//                model that is window_strand_z's z, gathered once).  ONE WINDOW IS THE UNIT OF ROUNDING: the lane adds
//                the window's softplus over the strands in float32, + before -, rounds to nearest into fixed point
//                (`scale` units per 1.0, a power of two: crbm_layout.h, records_unit_exp) and from there on everything
//                is a 64-bit integer add.  No float is combined across windows: which windows share a tile, a wave or a
//                segment changes with the segmenting, the sum of integers does not.
//   best site    motif_sites_body's key (site_key) with the start relative to the record, reduced with max.
//   letters      position s of a segment counts when s < own: a segment owns the positions of its window starts, the
//                last one the M - 1 letters behind them too -- every letter of the stream exactly once.
// A wave owns a CONTIGUOUS run of tiles of 64 positions, a lane one position per tile.  Every lane keeps integer sums,
// keys and counts of the record the wave is in (`cur`) in registers, for NQW motif quads at a time (the outer loop);
// when the record changes, and at the end of the run, the wave flushes: one integer wave sum, one key maximum and one
// atomic per motif on the call's accumulators, then zeros.  A record of 10^8 letters costs a wave one flush per run, not
// one per tile.  A tile inside one record is the wave-uniform path (no search); a tile with a record boundary finds
// every lane's record by a binary search over at most 64 entries of rec_start (a record holds at least its separator)
// and folds its records in ascending order, flushing between them.  Integer add and max commute: the same bits for
// every geometry, segmenting and run.  blockIdx.y is the slab of a generic DNA model, which owns its columns
// [k0 + kskip, k0 + kend); slab 0 counts windows and letters, on its first group of quads.
// ===========================================================================
struct ScanRecordsArgs : ScanInput {
  const long long* rec_start;            // [nrec + 1] stream positions
  unsigned long long* sums;              // [nrec][K] fixed-point softplus sums, or null
  unsigned long long* best;              // [nrec][K] keys, or null
  unsigned long long* counts;            // [nrec][5]: valid windows, then A, C, G, T; or null
  long long pos0;                        // stream position of the segment's first letter
  int32_t nrec;
  int32_t own;                           // positions of the segment whose letters it counts
  float scale;                           // fixed-point units per 1.0
  int32_t pad_;
};

// sum over the wave of 64-bit integers (all lanes call it; every lane gets it): wave_sum's DPP moves on both halves
__device__ __forceinline__ unsigned long long wave_sum_u64(unsigned long long v) {
  auto step = [&](auto CTRL, auto ROW_MASK) {
    const uint32_t lo = (uint32_t)__builtin_amdgcn_update_dpp(0, (int)(uint32_t)v, decltype(CTRL)::value, decltype(ROW_MASK)::value, 0xf, false);
    const uint32_t hi = (uint32_t)__builtin_amdgcn_update_dpp(0, (int)(uint32_t)(v >> 32), decltype(CTRL)::value, decltype(ROW_MASK)::value, 0xf, false);
    v += ((unsigned long long)hi << 32) | lo;
  };
  step(IC<0x121>{}, IC<0xf>{});
  step(IC<0x122>{}, IC<0xf>{});
  step(IC<0x124>{}, IC<0xf>{});
  step(IC<0x128>{}, IC<0xf>{});
  step(IC<0x142>{}, IC<0xa>{});
  step(IC<0x143>{}, IC<0xc>{});
  return ((unsigned long long)(uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)(v >> 32), 63) << 32) |
         (uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)v, 63);
}
// a window's softplus sum in fixed point: v * scale rounded to nearest (ties to even); v >= 0, v * scale < 2^31
__device__ __forceinline__ uint32_t records_fx(float v, float scale) { return (uint32_t)__builtin_rintf(v * scale); }
// the record of stream position p: the largest r in [lo, hi] with rec_start[r] <= p (rec_start[lo] <= p)
__device__ __forceinline__ int record_of(const long long* rec_start, int lo, int hi, long long p) {
  while (lo < hi) {
    const int mid = lo + (hi - lo + 1) / 2;
    if (rec_start[mid] <= p) lo = mid; else hi = mid - 1;
  }
  return lo;
}

template <class C>
__device__ void scan_records_body(const ScanRecordsArgs& a) {
  if constexpr (C::POOL == 1) {       // refused on the host, as the scan
    constexpr int M = C::M, S = C::DS ? 2 : 1;
    constexpr int NQW = C::NQ < 4 ? C::NQ : 4, NV = 4 * NQW;
    HIP_DYNAMIC_SHARED(float, smem);
    float* Tf = smem;
    const ScanInput& in = a;
    const int y = (int)blockIdx.y;
    const SlabSpan span = slab_span<C>(in.plan, y);
    copy_tables<C::TAB>(Tf, in.tables + (size_t)y * in.table_stride + C::OFF_TF);
    __syncthreads();
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, nwaves = blockDim.x >> 6;
    const bool want_fe = a.sums != nullptr, want_best = a.best != nullptr;
    const int K = in.plan.K;
    // the wave's run of tiles
    const int ntiles = (a.own + 63) >> 6;
    const int nw_all = (int)gridDim.x * nwaves, per = (ntiles + nw_all - 1) / nw_all;
    const int t0 = min(ntiles, ((int)blockIdx.x * nwaves + wave) * per), t1 = min(ntiles, t0 + per);
    if (t0 >= t1) return;
    const int r_run = record_of(a.rec_start, 0, a.nrec - 1, a.pos0 + 64ll * t0);
#pragma unroll 1
    for (int q0 = 0; q0 < C::NQ; q0 += NQW) {
      const bool counting = q0 == 0 && y == 0 && a.counts != nullptr;
      if (!counting && !want_fe && !want_best) continue;
      unsigned long long acc[NV], key[NV];
      uint32_t nwin = 0, nlet[4] = {0u, 0u, 0u, 0u};
#pragma unroll
      for (int j = 0; j < NV; ++j) { acc[j] = 0ull; key[j] = 0ull; }
      int cur = -1;                    // the record the registers belong to
      auto flush = [&]() {
        if (cur < 0) return;           // wave-uniform
#pragma unroll
        for (int j = 0; j < NV; ++j) {
          const int kk = 4 * q0 + j;
          if (kk < span.kskip || kk >= span.kend) continue;    // wave-uniform
          const size_t cell = (size_t)cur * K + span.k0 + kk;
          if (want_fe) {
            const unsigned long long s = wave_sum_u64(acc[j]);
            if (lane == 0 && s) atomicAdd(a.sums + cell, s);
          }
          if (want_best) {
            const unsigned long long k = wave_max_key(key[j]);
            if (lane == 0 && k) atomicMax(a.best + cell, k);
          }
          acc[j] = 0ull; key[j] = 0ull;
        }
        if (counting) {
          const unsigned long long w = wave_sum_u64(nwin);
          if (lane == 0 && w) atomicAdd(a.counts + (size_t)cur * 5, w);
#pragma unroll
          for (int l = 0; l < 4; ++l) {
            const unsigned long long c = wave_sum_u64(nlet[l]);
            if (lane == 0 && c) atomicAdd(a.counts + (size_t)cur * 5 + 1 + l, c);
            nlet[l] = 0u;
          }
          nwin = 0u;
        }
      };
      int r0 = r_run;
#pragma unroll 1
      for (int t = t0; t < t1; ++t) {
        const int s = 64 * t + lane;
        const long long p0 = a.pos0 + 64ll * t, p = p0 + lane;
        const bool single = p0 + 63 < a.rec_start[r0 + 1];             // wave-uniform: the tile lies in one record
        const int r_lane = single ? r0 : record_of(a.rec_start, r0, min(r0 + lane, a.nrec - 1), p);
        const bool ok = s < in.starts && window_valid<M>(in.valid, s);
        const bool letter = s < a.own && ((in.valid[s >> 6] >> (s & 63)) & 1ull);
        uint32_t fx[NV], pb[NV], minus = 0u;    // the window's fixed-point sums, the bits of its best scores, whose is the - strand's
#pragma unroll
        for (int j = 0; j < NV; ++j) { fx[j] = 0u; pb[j] = 0u; }
        if (ok && (want_fe || want_best)) {
          const LetterWin<M> w = letter_window<M>(in.letters, s);
          float sp[NV];
#pragma unroll
          for (int j = 0; j < NV; ++j) sp[j] = 0.f;
#pragma unroll
          for (int strand = 0; strand < S; ++strand) {
            float z[NV];
            window_strand_z<C, NQW>(Tf, w, q0, strand, z);
#pragma unroll
            for (int j = 0; j < NV; ++j) {
              if (want_best) {
                const uint32_t b = __float_as_uint(sigmoid_z(z[j]));
                if (strand == 0 || b > pb[j]) {                        // a tie stays with +
                  pb[j] = b;
                  minus = strand ? minus | (1u << j) : minus;
                }
              }
              if (C::DS && want_fe) sp[j] += softplus_of_z(z[j]);
            }
          }
          if (!C::DS && want_fe) {     // a single-stranded model's free energy sees the forward activation alone
            float z[NV];
            conv_gather_quads<C, NQW>(Tf, w, q0, z);
#pragma unroll
            for (int j = 0; j < NV; ++j) sp[j] = softplus_of_z(z[j]);
          }
          if (want_fe) {
#pragma unroll
            for (int j = 0; j < NV; ++j) fx[j] = records_fx(sp[j], a.scale);
          }
        }
        const uint32_t code = (in.letters[s >> 4] >> (2 * (s & 15))) & 3u;   // (inside the letter words for every s of a tile)
        // the records of the tile that have something to add, in ascending order
        unsigned long long todo = __ballot(ok || letter);
        while (todo) {                 // wave-uniform
          const int r = __builtin_amdgcn_readlane(r_lane, __ffsll(todo) - 1);
          const bool mine = r_lane == r;
          if (r != cur) { flush(); cur = r; }
          if (mine && ok) {
            const int rel = (int)(p - a.rec_start[r]);
#pragma unroll
            for (int j = 0; j < NV; ++j) {
              acc[j] += fx[j];
              if (want_best) {
                const unsigned long long k = ((unsigned long long)pb[j] << 32) |
                                             (unsigned long long)(0xFFFFFFFFu - (uint32_t)(2 * rel + (int)((minus >> j) & 1u)));
                key[j] = k > key[j] ? k : key[j];
              }
            }
            nwin += 1u;
          }
          if (mine && letter) {
#pragma unroll
            for (int l = 0; l < 4; ++l) nlet[l] += code == (uint32_t)l ? 1u : 0u;
          }
          todo &= ~__ballot(mine);
        }
        // the record of the next tile's first position: at most one further than that of this tile's last
        const int r63 = __builtin_amdgcn_readlane(r_lane, 63);
        r0 = (r63 + 1 < a.nrec && a.rec_start[r63 + 1] <= p0 + 64) ? r63 + 1 : r63;
      }
      flush();
    }
  }
}

#ifdef CRBM_DEFINE_MISC_KERNELS
// ===========================================================================
// Model-independent kernels, compiled ahead of time into libcrbm_hip.so.
// ===========================================================================

// plain streaming copy, 16 bytes per lane (crbm_copy_bandwidth): a block moves one contiguous 16 KB
// chunk, four loads in flight per lane
__global__ void __launch_bounds__(256) copy_float4_kernel(const float4* src, float4* dst, size_t n4) {
  const size_t base = (size_t)blockIdx.x * 1024 + threadIdx.x;
  if (base + 768 < n4) {
    const float4 a = src[base], b = src[base + 256], c = src[base + 512], d = src[base + 768];
    dst[base] = a; dst[base + 256] = b; dst[base + 512] = c; dst[base + 768] = d;
  } else {
    for (size_t i = base; i < n4 && i < base + 1024; i += 256) dst[i] = src[i];
  }
}

// one-hot fp32 (n,1,4,L) -> packed letters [n][LW]; flags[0] |= 1 on a column
// that is not exactly one-hot.
struct EncodeArgs {
  const float* v;
  uint32_t* letters;
  uint32_t* flags;
  int32_t n, L, LW;
  int32_t A;          // letters (the *_any kernels; the 2-bit kernels are DNA)
};

__global__ void encode_onehot_kernel(EncodeArgs a) {
  const long total = (long)a.n * a.LW;
  for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (long)gridDim.x * blockDim.x) {
    const int nn = (int)(i / a.LW);
    const int w = (int)(i - (long)nn * a.LW);
    uint32_t word = 0;
    bool bad = false;
    const float* base = a.v + (size_t)nn * 4 * a.L;
    for (int t = 0; t < 16; ++t) {
      const int p = w * 16 + t;
      if (p < a.L) {
        const float v0 = base[p], v1 = base[a.L + p], v2 = base[2 * a.L + p], v3 = base[3 * a.L + p];
        const int ones = (v0 == 1.f) + (v1 == 1.f) + (v2 == 1.f) + (v3 == 1.f);
        const int zeros = (v0 == 0.f) + (v1 == 0.f) + (v2 == 0.f) + (v3 == 0.f);
        bad |= (ones != 1) | (zeros != 3);
        const uint32_t l = (v1 == 1.f) ? 1u : (v2 == 1.f) ? 2u : (v3 == 1.f) ? 3u : 0u;
        word |= l << (2 * t);
      }
    }
    a.letters[i] = word;
    if (bad) atomicOr(a.flags, 1u);
  }
}

// one-hot fp32 (n,1,A,L) of any alphabet -> rows of bytes [n][LW] (four letters per word)
__global__ void encode_onehot_any_kernel(EncodeArgs a) {
  const long total = (long)a.n * a.LW;
  for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (long)gridDim.x * blockDim.x) {
    const int nn = (int)(i / a.LW);
    const int w = (int)(i - (long)nn * a.LW);
    uint32_t word = 0;
    bool bad = false;
    const float* base = a.v + (size_t)nn * a.A * a.L;
    for (int t = 0; t < 4; ++t) {
      const int p = w * 4 + t;
      if (p < a.L) {
        int ones = 0, zeros = 0;
        uint32_t l = 0u;
        for (int al = 0; al < a.A; ++al) {
          const float v = base[(size_t)al * a.L + p];
          if (v == 1.f) { if (!ones) l = (uint32_t)al; ++ones; }
          zeros += v == 0.f;
        }
        bad |= (ones != 1) | (zeros != a.A - 1);
        word |= l << (8 * t);
      }
    }
    a.letters[i] = word;
    if (bad) atomicOr(a.flags, 1u);
  }
}

// letter codes (one byte per base: 0..3 = A,C,G,T as in sequences.py:9-17) -> packed
// letters [n][LW]; flags[0] |= 1 on any other code.
struct EncodeCodesArgs {
  const unsigned char* codes;   // [n][L]
  uint32_t* letters;
  uint32_t* flags;
  int32_t n, L, LW;
  int32_t A;
};

__global__ void encode_codes_kernel(EncodeCodesArgs a) {
  const long total = (long)a.n * a.LW;
  for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (long)gridDim.x * blockDim.x) {
    const int nn = (int)(i / a.LW);
    const int w = (int)(i - (long)nn * a.LW);
    uint32_t word = 0;
    bool bad = false;
    const unsigned char* base = a.codes + (size_t)nn * a.L;
    for (int t = 0; t < 16; ++t) {
      const int p = w * 16 + t;
      if (p < a.L) {
        const uint32_t c = base[p];
        bad |= c > 3u;
        word |= (c & 3u) << (2 * t);
      }
    }
    a.letters[i] = word;
    if (bad) atomicOr(a.flags, 1u);
  }
}

// letter codes of any alphabet (one byte per letter, 0 .. A-1) -> rows of bytes [n][LW]; flags[0] |= 1 on any other code
__global__ void encode_codes_any_kernel(EncodeCodesArgs a) {
  const long total = (long)a.n * a.LW;
  for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (long)gridDim.x * blockDim.x) {
    const int nn = (int)(i / a.LW);
    const int w = (int)(i - (long)nn * a.LW);
    uint32_t word = 0;
    bool bad = false;
    const unsigned char* base = a.codes + (size_t)nn * a.L;
    for (int t = 0; t < 4; ++t) {
      const int p = w * 4 + t;
      if (p < a.L) {
        const uint32_t c = base[p];
        bad |= c >= (uint32_t)a.A;
        word |= (bad ? 0u : c) << (8 * t);
      }
    }
    a.letters[i] = word;
    if (bad) atomicOr(a.flags, 1u);
  }
}

// A segment of a stream (crbm_scan_sites_codes: codes 0..3 letters, 4 no letter) -> the validity plane and the letter
// words of scan_layout (crbm_layout.h), letter 0 under every invalid position.  A thread builds one validity word and
// its four letter words, those of the zero padding too: nothing else initialises the buffers.  flags[0] |= 1 on a code
// above 4.  `codes` is 4-byte aligned.
struct ScanEncodeArgs {
  const unsigned char* codes;   // [n]
  uint32_t* letters;
  unsigned long long* valid;
  uint32_t* flags;
  long long n, valid_words;
};
__global__ void scan_encode_kernel(ScanEncodeArgs a) {
  for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < a.valid_words; i += (long long)gridDim.x * blockDim.x) {
    unsigned long long v = 0ull;
    bool bad = false;
    const long long p0 = 64 * i;
#pragma unroll 1
    for (int w = 0; w < 4; ++w) {
      uint32_t word = 0;
      for (int q = 0; q < 4; ++q) {
        const long long p = p0 + 16 * w + 4 * q;
        uint32_t four = 0x04040404u;                         // past the end: no letters
        if (p + 4 <= a.n) four = *reinterpret_cast<const uint32_t*>(a.codes + p);
        else
          for (int t = 0; t < 4; ++t)
            if (p + t < a.n) four = (four & ~(0xFFu << (8 * t))) | ((uint32_t)a.codes[p + t] << (8 * t));
        for (int t = 0; t < 4; ++t) {
          const uint32_t c = (four >> (8 * t)) & 0xFFu;
          bad |= c > 4u;
          if (c < 4u) {
            word |= c << (2 * (4 * q + t));
            v |= 1ull << (16 * w + 4 * q + t);
          }
        }
      }
      a.letters[4 * i + w] = word;
    }
    a.valid[i] = v;
    if (bad) atomicOr(a.flags, 1u);
  }
}

// The tail of pass 0 of the stream scan: tile counts -> exclusive offsets and their total, one block per slab
// (blockIdx.x); a thread sums a run of tiles, the block scans the run sums in LDS (8 bytes per thread, dynamic).
struct ScanOffsetsArgs {
  const uint32_t* tile_cnt;        // [slab][tiles]
  unsigned long long* tile_off;    // [slab][tiles]
  unsigned long long* total;       // [slab]
  int32_t tiles;
};
__global__ void __launch_bounds__(1024) scan_offsets_kernel(ScanOffsetsArgs a) {
  HIP_DYNAMIC_SHARED(unsigned long long, part);
  const int tid = (int)threadIdx.x, nt = (int)blockDim.x;
  const uint32_t* cnt = a.tile_cnt + (size_t)blockIdx.x * a.tiles;
  unsigned long long* off = a.tile_off + (size_t)blockIdx.x * a.tiles;
  const int run = (a.tiles + nt - 1) / nt;
  const int lo = (int)min((long long)tid * run, (long long)a.tiles), hi = min(lo + run, a.tiles);
  unsigned long long sum = 0ull;
  for (int i = lo; i < hi; ++i) sum += cnt[i];
  part[tid] = sum;
  __syncthreads();
  for (int d = 1; d < nt; d <<= 1) {
    const unsigned long long add = tid >= d ? part[tid - d] : 0ull;
    __syncthreads();
    part[tid] += add;
    __syncthreads();
  }
  unsigned long long at = part[tid] - sum;
  for (int i = lo; i < hi; ++i) {
    off[i] = at;
    at += cnt[i];
  }
  if (tid == nt - 1) a.total[blockIdx.x] = part[tid];
}

// The tail of the variant effects (variant_effects_body): dfe[i] = sum_k per_motif[i][k] - (c[alt_i] - c[ref_i]), the
// motifs added in ascending k -- one rule for a model on its own kernels and for one that runs as slabs -- and exactly 0
// where the variant sits on no letter (its row is all zeros then).  ref_i is code M - 1 of the staged context.
struct VariantCombineArgs {
  const float* per_motif;       // [cnt][K]
  const unsigned char* codes;   // [cnt][CW], the staged contexts
  const unsigned char* alt;     // [cnt]
  const float* c;               // (4) the visible bias
  float* dfe;                   // [cnt]
  int32_t cnt, K, CW, M;
};
__global__ void __launch_bounds__(256) variant_combine_kernel(VariantCombineArgs a) {
  for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < a.cnt; i += gridDim.x * blockDim.x) {
    const uint32_t ref = a.codes[(size_t)i * a.CW + a.M - 1];
    const float* row = a.per_motif + (size_t)i * a.K;
    float s = 0.f;
    for (int k = 0; k < a.K; ++k) s += row[k];
    a.dfe[i] = ref < 4u ? s - (a.c[a.alt[i] & 3u] - a.c[ref]) : 0.f;
  }
}

// The tail of the allele effects (allele_effects_body), variant_combine_kernel's rule for alleles of any length:
// dfe[i] = sum_k per_motif[i][k] - (sum_j c[alt_j] - sum_j c[ref_j]), the motifs added in ascending k, the bias sums
// in ascending letter order, ref and alt separately; exactly 0 for a `zero` variant (its row is all zeros).  The ref
// letters are codes [M - 1, M - 1 + R) of the staged refhap, the alt letters codes [M - 1, M - 1 + A) of the althap.
struct AlleleCombineArgs {
  const float* per_motif;       // [cnt][K]
  const unsigned char* codes;   // the staged haplotypes
  const AlleleEntry* table;     // [cnt]
  const float* c;               // (4) the visible bias
  float* dfe;                   // [cnt]
  int32_t cnt, K, M, pad_;
};
__global__ void __launch_bounds__(256) allele_combine_kernel(AlleleCombineArgs a) {
  for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < a.cnt; i += gridDim.x * blockDim.x) {
    const AlleleEntry e = a.table[i];
    if (e.zero) { a.dfe[i] = 0.f; continue; }
    const float* row = a.per_motif + (size_t)i * a.K;
    float s = 0.f;
    for (int k = 0; k < a.K; ++k) s += row[k];
    const unsigned char* ref = a.codes + e.off + a.M - 1;
    const unsigned char* alt = ref + e.R + 2 * (a.M - 1);
    float cr = 0.f, ca = 0.f;
    for (int j = 0; j < e.R; ++j) cr += a.c[ref[j] & 3u];
    for (int j = 0; j < e.A; ++j) ca += a.c[alt[j] & 3u];
    a.dfe[i] = s - (ca - cr);
  }
}

// packed letters -> one-hot fp32 (n,1,4,L)
struct DecodeArgs {
  const uint32_t* letters;
  float* v;
  int32_t n, L, LW;
  int32_t A;
};

// rows of bytes -> one-hot fp32 (n,1,A,L)
__global__ void decode_onehot_any_kernel(DecodeArgs a) {
  const long total = (long)a.n * a.L;
  for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (long)gridDim.x * blockDim.x) {
    const int nn = (int)(i / a.L);
    const int p = (int)(i - (long)nn * a.L);
    const uint32_t l = reinterpret_cast<const unsigned char*>(a.letters + (size_t)nn * a.LW)[p];
    float* base = a.v + (size_t)nn * a.A * a.L + p;
    for (int al = 0; al < a.A; ++al) base[(size_t)al * a.L] = l == (uint32_t)al ? 1.f : 0.f;
  }
}

__global__ void decode_onehot_kernel(DecodeArgs a) {
  const long total = (long)a.n * a.L;
  for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (long)gridDim.x * blockDim.x) {
    const int nn = (int)(i / a.L);
    const int p = (int)(i - (long)nn * a.L);
    const uint32_t l = (a.letters[(size_t)nn * a.LW + (p >> 4)] >> (2 * (p & 15))) & 3u;
    float* base = a.v + (size_t)nn * 4 * a.L + p;
    base[0] = l == 0 ? 1.f : 0.f;
    base[a.L] = l == 1 ? 1.f : 0.f;
    base[2 * a.L] = l == 2 ? 1.f : 0.f;
    base[3 * a.L] = l == 3 ? 1.f : 0.f;
  }
}

// dense hidden (n,K,1,Lh) <-> K-bit masks [n][Lh][NW]; flags[0] |= 2 if not 0/1
struct HiddenPackArgs {
  float* dense;
  uint32_t* masks;
  uint32_t* flags;
  int32_t n, K, Lh, NW;
};

__global__ void pack_hidden_kernel(HiddenPackArgs a) {
  const long total = (long)a.n * a.Lh;
  for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (long)gridDim.x * blockDim.x) {
    const int nn = (int)(i / a.Lh);
    const int s = (int)(i - (long)nn * a.Lh);
    bool bad = false;
    for (int w = 0; w < a.NW; ++w) {
      uint32_t m = 0;
      for (int bit = 0; bit < 32; ++bit) {
        const int k = w * 32 + bit;
        if (k < a.K) {
          const float v = a.dense[((size_t)nn * a.K + k) * a.Lh + s];
          bad |= !(v == 0.f || v == 1.f);
          m |= (v == 1.f ? 1u : 0u) << bit;
        }
      }
      a.masks[i * a.NW + w] = m;
    }
    if (bad) atomicOr(a.flags, 2u);
  }
}

__global__ void unpack_hidden_kernel(HiddenPackArgs a) {
  const long total = (long)a.n * a.Lh;
  for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (long)gridDim.x * blockDim.x) {
    const int nn = (int)(i / a.Lh);
    const int s = (int)(i - (long)nn * a.Lh);
    for (int k = 0; k < a.K; ++k) {
      const uint32_t m = a.masks[i * a.NW + (k >> 5)];
      a.dense[((size_t)nn * a.K + k) * a.Lh + s] = (float)((m >> (k & 31)) & 1u);
    }
  }
}

// ---------------------------------------------------------------------------
// v_given_h from DENSE hidden tensors (any finite values): _topDownActivity,
// _topDownProbability, _topDownSample (convRBM.py:277-325).  API/test pass;
// the training chain uses the Gibbs kernel.
// ---------------------------------------------------------------------------
struct VghArgs {
  const float* W;       // (K,4,M)
  const float* c;       // (4)
  int32_t K, M;
  const float* hid;
  const float* hidp;    // null when single-stranded
  int32_t n, Lh, L;
  int32_t TS;
  FastDiv divL;
  float* act;
  float* prob;
  float* sample;
  RngView rng;
  uint32_t kind;
};

// The filters pass through LDS a slab of KS motifs at a time (vgh_dense_ks, crbm_layout.h: a fixed budget, so every model
// the constructor accepts can be launched); a position's four activations stay in registers across the slabs, and the
// additions keep their order -- motif outer, column inner -- whatever the slab size.  A model of one slab stages its
// filters once per block; a larger one stages every slab once per round of blockDim positions (an API / test pass).
__global__ void __launch_bounds__(256) vgh_dense_kernel(VghArgs a) {
  HIP_DYNAMIC_SHARED(float, smem);
  const int K = a.K, M = a.M, KS = vgh_dense_ks(K, M);
  const bool one_slab = KS >= K;
  float4* W4 = reinterpret_cast<float4*>(smem);   // [j][k - k0] -> W[k][0..3][j] of the slab's motifs
  auto stage = [&](int k0, int kc) {
    for (int idx = threadIdx.x; idx < M * kc; idx += blockDim.x) {
      const int j = idx / kc, k = k0 + idx - j * kc;
      W4[idx] = make_float4(a.W[(k * 4 + 0) * M + j], a.W[(k * 4 + 1) * M + j],
                            a.W[(k * 4 + 2) * M + j], a.W[(k * 4 + 3) * M + j]);
    }
  };
  if (one_slab) {
    stage(0, K);
    __syncthreads();
  }
  const float c0 = a.c[0], c1 = a.c[1], c2 = a.c[2], c3 = a.c[3];
  const int ntiles = (a.n + a.TS - 1) / a.TS;
  for (int tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
    const int n0 = tile * a.TS;
    const int ns = min(a.TS, a.n - n0);
    const uint32_t items = (uint32_t)ns * (uint32_t)a.L;
    // (a round of blockDim positions: the bound is the block's, so every thread meets the barriers of the slab loop)
    for (uint32_t i0 = 0; i0 < items; i0 += blockDim.x) {
      const uint32_t i = i0 + threadIdx.x;
      const bool live = i < items;
      const uint32_t nl = live ? fastdiv(i, a.divL) : 0u;
      const int p = (int)(i - nl * (uint32_t)a.L);
      const int nn = n0 + (int)nl;
      float y0 = c0, y1 = c1, y2 = c2, y3 = c3;
      const int jlo = max(0, p - a.Lh + 1), jhi = min(M - 1, p);
      for (int k0 = 0; k0 < K; k0 += KS) {
        const int kc = min(KS, K - k0);
        if (!one_slab) {
          __syncthreads();                        // the previous slab is still being read
          stage(k0, kc);
          __syncthreads();
        }
        if (!live) continue;
        for (int k = k0; k < k0 + kc; ++k) {
          const float* hrow = a.hid + ((size_t)nn * K + k) * a.Lh;
          const float* hprow = a.hidp ? a.hidp + ((size_t)nn * K + k) * a.Lh : nullptr;
          for (int j = jlo; j <= jhi; ++j) {
            const float hv = hrow[p - j];
            const float4 w = W4[j * kc + (k - k0)];
            y0 = fmaf(w.x, hv, y0); y1 = fmaf(w.y, hv, y1); y2 = fmaf(w.z, hv, y2); y3 = fmaf(w.w, hv, y3);
            if (hprow) {   // rc(W)[k,a,j] = W[k,3-a,M-1-j]
              const float hp = hprow[p - j];
              const float4 wr = W4[(M - 1 - j) * kc + (k - k0)];
              y0 = fmaf(wr.w, hp, y0); y1 = fmaf(wr.z, hp, y1); y2 = fmaf(wr.y, hp, y2); y3 = fmaf(wr.x, hp, y3);
            }
          }
        }
      }
      if (!live) continue;
      const size_t o = (size_t)nn * 4 * a.L + p;
      if (a.act) { a.act[o] = y0; a.act[o + a.L] = y1; a.act[o + 2 * a.L] = y2; a.act[o + 3 * a.L] = y3; }
      const float mx = fmaxf(fmaxf(y0, y1), fmaxf(y2, y3));
      const float e0 = __expf(y0 - mx), e1 = __expf(y1 - mx), e2 = __expf(y2 - mx), e3 = __expf(y3 - mx);
      const float sum = (e0 + e1) + (e2 + e3);
      if (a.prob) {
        const float inv = 1.0f / sum;
        a.prob[o] = e0 * inv; a.prob[o + a.L] = e1 * inv; a.prob[o + 2 * a.L] = e2 * inv; a.prob[o + 3 * a.L] = e3 * inv;
      }
      if (a.sample) {
        const Philox4 r = philox4x32(a.rng.seq_offset + (uint32_t)nn, (uint32_t)(p >> 2),
                                        rng_word2(a.kind, 0, 0, 0), a.rng.step, a.rng.seed_lo, a.rng.seed_hi);
        const float t = u01(philox_pick(r, p & 3)) * sum;
        const int l = (t >= e0) + (t >= e0 + e1) + (t >= (e0 + e1) + e2);
        a.sample[o] = l == 0 ? 1.f : 0.f; a.sample[o + a.L] = l == 1 ? 1.f : 0.f;
        a.sample[o + 2 * a.L] = l == 2 ? 1.f : 0.f; a.sample[o + 3 * a.L] = l == 3 ? 1.f : 0.f;
      }
    }
  }
}


// The same for an alphabet of A != 4 letters: a thread keeps the A activations of its position in LDS
// (yl[letter][thread]); filters straight from global memory (an API / test pass).
struct VghAnyArgs {
  VghArgs g;
  int32_t A;
};

__global__ void __launch_bounds__(256) vgh_dense_any_kernel(VghAnyArgs aa) {
  HIP_DYNAMIC_SHARED(float, smem);
  const VghArgs& a = aa.g;
  const int K = a.K, M = a.M, A = aa.A, CH = (int)blockDim.x, tid = (int)threadIdx.x;
  float* yl = smem;   // [A][CH]
  const long items = (long)a.n * a.L;
  for (long i0 = (long)blockIdx.x * CH; i0 < items; i0 += (long)gridDim.x * CH) {
    const long i = i0 + tid;
    if (i >= items) continue;
    const int nn = (int)(i / a.L), p = (int)(i - (long)nn * a.L);
    for (int al = 0; al < A; ++al) yl[al * CH + tid] = a.c[al];
    const int jlo = max(0, p - a.Lh + 1), jhi = min(M - 1, p);
    for (int k = 0; k < K; ++k) {
      const float* hrow = a.hid + ((size_t)nn * K + k) * a.Lh;
      const float* hprow = a.hidp ? a.hidp + ((size_t)nn * K + k) * a.Lh : nullptr;
      for (int j = jlo; j <= jhi; ++j) {
        const float hv = hrow[p - j];
        const float hp = hprow ? hprow[p - j] : 0.f;
        for (int al = 0; al < A; ++al) {
          float y = fmaf(a.W[((size_t)k * A + al) * M + j], hv, yl[al * CH + tid]);
          if (hprow) y = fmaf(a.W[((size_t)k * A + (A - 1 - al)) * M + (M - 1 - j)], hp, y);   // rc(W)[k,a,j] = W[k,A-1-a,M-1-j]
          yl[al * CH + tid] = y;
        }
      }
    }
    const size_t o = (size_t)nn * A * a.L + p;
    float mx = yl[tid];
    for (int al = 0; al < A; ++al) {
      const float y = yl[al * CH + tid];
      if (a.act) a.act[o + (size_t)al * a.L] = y;
      mx = fmaxf(mx, y);
    }
    float sum = 0.f;
    for (int al = 0; al < A; ++al) {
      const float e = __expf(yl[al * CH + tid] - mx);
      yl[al * CH + tid] = e;
      sum += e;
    }
    if (a.prob) {
      const float inv = 1.0f / sum;
      for (int al = 0; al < A; ++al) a.prob[o + (size_t)al * a.L] = yl[al * CH + tid] * inv;
    }
    if (a.sample) {
      const Philox4 r = philox4x32(a.rng.seq_offset + (uint32_t)nn, (uint32_t)(p >> 2),
                                      rng_word2(a.kind, 0, 0, 0), a.rng.step, a.rng.seed_lo, a.rng.seed_hi);
      const float t = u01(philox_pick(r, p & 3)) * sum;
      float cum = 0.f;
      int l = 0;
      for (int al = 0; al < A - 1; ++al) {
        cum += yl[al * CH + tid];
        l += t >= cum ? 1 : 0;
      }
      for (int al = 0; al < A; ++al) a.sample[o + (size_t)al * a.L] = l == al ? 1.f : 0.f;
    }
  }
}

#include "crbm_kernels_generic.h"   // models the LDS-resident kernels do not take: more motifs, longer motifs, other alphabets

// fixed-point sums over the position chunks of a sequence (hit_summary_body) -> mean over positions
__global__ void hit_finalize_kernel(const unsigned long long* fx, float* out, size_t count, float scale) {
  for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < count; i += (size_t)gridDim.x * blockDim.x)
    out[i] = (float)((double)fx[i] * (double)scale);
}

// Motif sites of the models the fused pass does not take (crbm_api.hip, motif_sites_any on h->big): the same records and
// keys (emit_sites, site_key) from the dense probabilities of a slab, p0 = the forward strand (single-stranded models:
// sigma-pool(x + x')), p1 = the reverse-complemented filter or null.  One wave per (sequence, motif) row: the key is
// stored, no atomics but the record counter's.
struct SitesSelectArgs {
  const float* p0;
  const float* p1;
  int32_t n, K, Lh, ds;
  SitesOut o;
};
__global__ void __launch_bounds__(256) motif_sites_select_kernel(SitesSelectArgs a) {
  const int lane = threadIdx.x & 63, nwaves = blockDim.x >> 6;
  const long rows = (long)a.n * a.K;
  for (long r = (long)blockIdx.x * nwaves + (threadIdx.x >> 6); r < rows; r += (long)gridDim.x * nwaves) {
    const int nn = (int)(r / a.K), k = (int)(r - (long)nn * a.K);
    unsigned long long key = 0ull;
    for (int s0 = 0; s0 < a.Lh; s0 += 64) {
      const int s = s0 + lane;
      const bool valid = s < a.Lh;
      float p[2] = {0.f, 0.f};
      if (valid) {
        p[0] = a.p0[(size_t)r * a.Lh + s];
        if (a.p1) p[1] = a.p1[(size_t)r * a.Lh + s];
      }
      if (a.o.recs) {
        const bool hit[2] = {valid && p[0] >= a.o.threshold, valid && a.p1 && p[1] >= a.o.threshold};
        emit_sites<2>(a.o, hit, [&](int j) { return SiteRec{nn, k, s, a.ds ? (j ? -1 : 1) : 0, p[j]}; });
      }
      if (valid) {
        const unsigned long long k0 = site_key(p[0], s, 0);
        key = k0 > key ? k0 : key;
        if (a.p1) {
          const unsigned long long k1 = site_key(p[1], s, 1);
          key = k1 > key ? k1 : key;
        }
      }
    }
    if (a.o.best) {
      const unsigned long long kmax = wave_max_key(key);
      if (lane == 0) a.o.best[r] = kmax;
    }
  }
}

// One wave that does nothing for `ticks` of the GPU's wall clock: put in front of a partition's first chain launch
// so that the partitions' launches interleave from the start (crbm_api.hip, launch_gibbs_parts)
__global__ void __launch_bounds__(64) delay_kernel(unsigned long long ticks) {
  const uint64_t t0 = realtime_ticks();
  while (realtime_ticks() - t0 < ticks) short_sleep();
}

__global__ void __launch_bounds__(1024) reduce_partials_kernel(ReduceArgs a) { reduce_partials_body<false>(a); }

// IPC all-reduce: the column reduction writes this rank's sums straight into its slot of every rank's buffer,
// and the block that arrives last raises the rank's flag in all of them -- the all-reduce then costs no launch of
// its own (the stores are system-scope and drained before a block's ticket; the last block's fence orders them
// before the flags)
struct PublishTail {
  uint32_t* ticket;      // zero before the launch, left zero
  uint32_t* flag[8];     // this rank's flag word of the step's parity in every rank's buffer
  uint32_t value;
  PushTargets push;
};
__global__ void __launch_bounds__(1024) reduce_publish_pair_kernel(ReducePair p, PublishTail t) {
  reduce_partials_body<true>(p.half[blockIdx.y], &t.push);
  wait_vector_memory();
  __syncthreads();
  if (threadIdx.x == 0) {
    const uint32_t prev = ticket_add(t.ticket);
    if (prev == gridDim.x * gridDim.y - 1u) {
      atomicExch(t.ticket, 0u);
      fence_system();
      for (int r = 0; r < t.push.n; ++r) store_system(t.flag[r], t.value);
    }
  }
}

__global__ void __launch_bounds__(1024) reduce_partials_pair_kernel(ReducePair p) {
  reduce_partials_body<false>(p.half[blockIdx.y]);
}

__global__ void apply_update_kernel(UpdateArgs a) { apply_update_body<0>(a, nullptr, true, PlainSums{a.sums}); }   // one block, in place

// IPC all-reduce: this rank's sums of the step (formed in d_sums) -> its slot of every rank's buffer, then its
// flags (one block)
struct PublishArgs {
  const float* src;
  float* dst[8];         // this rank's slot of the step's parity in every rank's buffer
  uint32_t* flag[8];
  uint32_t value;
  int32_t count, n;
};
__global__ void __launch_bounds__(1024) publish_sums_kernel(PublishArgs a) {
  for (int i = threadIdx.x; i < a.count; i += blockDim.x) {
    const float v = a.src[i];
    for (int r = 0; r < a.n; ++r) store_system(a.dst[r] + i, v);
  }
  wait_vector_memory();                             // this wave's (write-through) stores have left ...
  __syncthreads();                                  // ... and so have everybody's
  if (threadIdx.x == 0) {
    fence_system();                                 // one release for the block (a fence per thread costs microseconds)
    for (int r = 0; r < a.n; ++r) store_system(a.flag[r], a.value);
  }
}
#endif  // CRBM_DEFINE_MISC_KERNELS

}  // namespace crbm
