// Markov backgrounds on the device (gfx950, wave64): the j-mer counts of a stream and exact sampling from a Markov
// chain of order 0..3 over A, C, G, T.  Model-independent: compiled ahead of time into libcrbm_hip.so (crbm_api.hip:
// crbm_stream_kmer_counts / crbm_background_sample) and, with g++ against tests/emu/shim, into the emulation program
// tests/emu/background_main.cpp.  DESIGN.md section 5, "Markov backgrounds".
//
// Integers only: counts are integer adds, a letter is three unsigned comparisons of a Philox word with a threshold row.
// Nothing depends on the launch geometry, the chunk length or how a stream is cut into segments: the same bits always.
//
// Contexts.  A context is the last j <= order letters l_1 .. l_j (oldest first) and has the index
// (4^j - 1) / 3 + sum_i l_i 4^(j - i); 0 is the empty context (the start of a stream and the position behind a gap).
// There are contexts(order) = 1, 5, 21, 85 of them.  The sampler works on rows of four words per context: the three
// thresholds, and the four successor contexts (one byte per letter) packed into the fourth word.
//
// The chain is sequential; the parallelism comes from transition maps.  A draw u_p maps every context to the next one,
// and maps compose associatively:
//   maps     a lane owns a chunk of `chunk` positions and carries the image of every entry context through it, all on
//            the same draws; once the images agree (a gap makes them agree at once) it carries one.  Out: the chunk's
//            map, contexts(order) bytes.
//   groups   a lane composes the maps of GROUP consecutive chunks: the group's map.
//   walk     one block walks the group maps in order, a tile at a time through the LDS: the entry context of every
//            group, from the carry of the segment before; leaves the carry of the next.
//   entries  a lane walks the chunks of its group from the group's entry context: the entry context of every chunk.
//   letters  a lane regenerates its chunk from its true entry context and writes the letters, a word of four at a time.
// The dependent chain is 2 GROUP global loads and one LDS load per group.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "crbm_kernels.h"

namespace crbm {
namespace bg {

constexpr int MAX_ORDER = 3;
constexpr int GROUP = 64;            // chunks per group
constexpr int WALK_TILE = 256;       // group maps per LDS tile of the walk
constexpr int CHUNK_DEFAULT = 256;   // positions per chunk (CRBM_BG_CHUNK): the fastest of 64 .. 4096, profiles/background_chunk_scan.json
constexpr int CHUNK_MIN = 4, CHUNK_MAX = 1 << 20;
constexpr int64_t MAX_T = 2147483647;
constexpr int64_t MAX_POS = (int64_t)1 << 62;

__host__ __device__ constexpr int pow4(int j) { return 1 << (2 * j); }
__host__ __device__ constexpr int contexts(int order) { return (pow4(order + 1) - 1) / 3; }
__host__ __device__ constexpr int context_base(int j) { return (pow4(j) - 1) / 3; }          // first context of j letters
__host__ __device__ constexpr int kmer_offset(int j) { return (pow4(j) - 4) / 3; }           // first j-mer counter, j >= 1
__host__ __device__ constexpr int kmer_slots(int order) { return kmer_offset(order + 2); }   // 4, 20, 84, 340

// the context behind context s once letter a has been appended
inline int next_context(int order, int s, int a) {
  int j = 0;
  while (j < order && s >= context_base(j + 1)) ++j;
  const int v = (s - context_base(j)) * 4 + a;
  return j < order ? context_base(j + 1) + v : context_base(order) + (v & (pow4(order) - 1));
}
// rows [contexts(order)][4] from thresholds [contexts(order)][3]
inline void build_rows(const uint32_t* thr, int order, uint32_t* rows) {
  for (int s = 0; s < contexts(order); ++s) {
    uint32_t next = 0;
    for (int a = 0; a < 4; ++a) next |= (uint32_t)next_context(order, s, a) << (8 * a);
    rows[4 * s] = thr[3 * s]; rows[4 * s + 1] = thr[3 * s + 1]; rows[4 * s + 2] = thr[3 * s + 2]; rows[4 * s + 3] = next;
  }
}
// CRBM_BG_CHUNK as the kernels take it: a multiple of four within [CHUNK_MIN, CHUNK_MAX]
inline int chunk_length(long want) {
  if (want < CHUNK_MIN) want = CHUNK_MIN;
  if (want > CHUNK_MAX) want = CHUNK_MAX;
  return (int)(want & ~3L);
}

// ---- what the entry points refuse (host; the emulation program prints these too) --------------------------------
inline const char* codes_refusal(const uint8_t* codes, int64_t n) {
  unsigned bad = 0;
  for (int64_t i = 0; i < n; ++i) bad |= codes[i] > 4 ? 1u : 0u;
  return bad ? "stream codes must lie in 0..4 (0..3 = A,C,G,T; 4 = no letter)" : nullptr;
}
inline const char* counts_refusal(const uint8_t* codes, int64_t T, int32_t order, const void* counts) {
  if (order < 0 || order > MAX_ORDER) return "order must lie in [0, 3]";
  if (T < 0 || T > MAX_T) return "stream length must lie in [0, 2^31 - 1]";
  if (!counts || (!codes && T > 0)) return "null argument";
  return codes_refusal(codes, T);
}
inline const char* sample_refusal(const uint32_t* thr, int32_t order, int64_t T, int64_t pos0, const uint8_t* tmpl, const void* out) {
  if (order < 0 || order > MAX_ORDER) return "order must lie in [0, 3]";
  if (T < 0 || T > MAX_T) return "T must lie in [0, 2^31 - 1]";
  if (pos0 < 0 || pos0 > MAX_POS) return "pos0 must lie in [0, 2^62]";
  if (!thr || (!out && T > 0)) return "null argument";
  for (int s = 0; s < contexts(order); ++s)
    if (thr[3 * s] > thr[3 * s + 1] || thr[3 * s + 1] > thr[3 * s + 2]) return "a row of the threshold table does not ascend";
  return tmpl ? codes_refusal(tmpl, T) : nullptr;
}

// ---- 1. j-mer counts ------------------------------------------------------------------------------------------------
struct KmerArgs {
  const uint8_t* codes;             // n staged codes: the segment's own positions and the halo behind them
  unsigned long long* counts;       // kmer_slots(order), added to
  int64_t n, starts;                // positions [0, starts) are the segment's own; a j-mer at p reads codes [p, p + j), p + j <= n
  int order;
};

// A lane owns a position and counts the j-mers that start there, j = 1 .. order + 1, until a code is no letter or the
// staged codes end.  32-bit counters in the LDS (a block sees fewer than 2^32 positions), flushed with 64-bit atomics.
// LDS: kmer_slots(order) * 4 bytes.
__global__ void __launch_bounds__(256) kmer_count_kernel(KmerArgs a) {
  HIP_DYNAMIC_SHARED(uint32_t, kmer_lds);
  const int slots = kmer_slots(a.order);
  for (int e = (int)threadIdx.x; e < slots; e += (int)blockDim.x) kmer_lds[e] = 0u;
  __syncthreads();
  for (int64_t p = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; p < a.starts; p += (int64_t)gridDim.x * blockDim.x) {
    uint32_t v = 0;
    for (int j = 1; j <= a.order + 1 && p + j <= a.n; ++j) {
      const uint32_t c = a.codes[p + j - 1];
      if (c > 3u) break;
      v = v * 4u + c;
      atomicAdd(&kmer_lds[kmer_offset(j) + (int)v], 1u);
    }
  }
  __syncthreads();
  for (int e = (int)threadIdx.x; e < slots; e += (int)blockDim.x)
    if (kmer_lds[e]) atomicAdd(&a.counts[e], (unsigned long long)kmer_lds[e]);
}

// ---- 2. sampling ----------------------------------------------------------------------------------------------------
struct SampleArgs {
  const uint4* rows;        // contexts(order) rows: thresholds x, y, z; successors in w
  const uint8_t* tmpl;      // n codes, or null: all letters
  uint8_t* out;             // n codes
  uint8_t* cmap;            // [chunks][contexts]: a chunk's map
  uint8_t* gmap;            // [groups][contexts]: a group's map
  uint8_t* centry;          // [chunks]: a chunk's entry context
  uint8_t* gentry;          // [groups]
  uint8_t* carry;           // [1]: the entry context of this segment, replaced by that of the next
  int64_t n, pos0;          // positions [0, n) of the segment are positions pos0 + p of the contract
  int64_t chunks, groups;
  int32_t chunk;            // positions per chunk, a multiple of 4
  uint32_t seed_lo, seed_hi;
};

// the Philox block of position P: word P & 3 is the draw
__device__ __forceinline__ Philox4 draw_block(int64_t P, uint32_t k0, uint32_t k1) {
  return philox4x32((uint32_t)((uint64_t)P >> 2), (uint32_t)((uint64_t)P >> 34), rng_word2(KIND_BACKGROUND, 0u, 0u, 0u), 0u, k0, k1);
}
// the successor of the row's context under draw u; `letter` is what was drawn
__device__ __forceinline__ uint32_t advance(const uint4& row, uint32_t u, uint32_t& letter) {
  letter = (u >= row.x ? 1u : 0u) + (u >= row.y ? 1u : 0u) + (u >= row.z ? 1u : 0u);
  return (row.w >> (8u * letter)) & 255u;
}
// template codes [p, p + cnt), cnt <= 4, one per byte; p is a multiple of 4 and so is the buffer's base
__device__ __forceinline__ uint32_t codes4(const uint8_t* tmpl, int64_t p, int cnt) {
  if (!tmpl) return 0u;
  if (cnt == 4) return *reinterpret_cast<const uint32_t*>(tmpl + p);
  uint32_t w = 0;
  for (int i = 0; i < cnt; ++i) w |= (uint32_t)tmpl[p + i] << (8 * i);
  return w;
}

// maps: one lane per chunk.  LDS: contexts(ORDER) * 16 bytes.
template <int ORDER>
__global__ void __launch_bounds__(256) sample_maps_kernel(SampleArgs a) {
  constexpr int NS = contexts(ORDER);
  HIP_DYNAMIC_SHARED(uint4, maps_rows);
  for (int e = (int)threadIdx.x; e < NS; e += (int)blockDim.x) maps_rows[e] = a.rows[e];
  __syncthreads();
  for (int64_t c = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; c < a.chunks; c += (int64_t)gridDim.x * blockDim.x) {
    const int64_t p0 = c * a.chunk, p1 = p0 + a.chunk < a.n ? p0 + a.chunk : a.n;
    uint32_t m[NS];
#pragma unroll
    for (int s = 0; s < NS; ++s) m[s] = (uint32_t)s;
    bool one = NS == 1;                                  // the images agree: m[0] is the image of every entry context
    int64_t P = a.pos0 + p0;
    Philox4 r = draw_block(P, a.seed_lo, a.seed_hi);
    for (int64_t p = p0; p < p1; p += 4) {
      const int cnt = p1 - p < 4 ? (int)(p1 - p) : 4;
      const uint32_t tw = codes4(a.tmpl, p, cnt);
#pragma unroll 1
      for (int i = 0; i < cnt; ++i) {
        const uint32_t u = philox_pick(r, (int)(P & 3)), code = (tw >> (8 * i)) & 255u;
        uint32_t letter;
        if (code > 3u) {
          m[0] = 0u;
          one = true;
        } else if (one) {
          m[0] = advance(maps_rows[m[0]], u, letter);
        } else {
          bool same = true;
#pragma unroll
          for (int s = 0; s < NS; ++s) {
            m[s] = advance(maps_rows[m[s]], u, letter);
            same = same && m[s] == m[0];
          }
          one = same;
        }
        ++P;
        if ((P & 3) == 0) r = draw_block(P, a.seed_lo, a.seed_hi);
      }
    }
    uint8_t* dst = a.cmap + c * NS;
#pragma unroll
    for (int s = 0; s < NS; ++s) dst[s] = (uint8_t)(one ? m[0] : m[s]);
  }
}

// the composition of the maps [i0, i1) of `maps` ([..][NS] bytes), in order, written to dst
template <int NS>
__device__ __forceinline__ void compose(const uint8_t* maps, int64_t i0, int64_t i1, uint8_t* dst) {
  uint32_t m[NS];
#pragma unroll
  for (int s = 0; s < NS; ++s) m[s] = (uint32_t)s;
  bool one = NS == 1;
  for (int64_t i = i0; i < i1; ++i) {
    const uint8_t* map = maps + i * NS;
    if (one) {
      m[0] = map[m[0]];
    } else {
      bool same = true;
#pragma unroll
      for (int s = 0; s < NS; ++s) {
        m[s] = map[m[s]];
        same = same && m[s] == m[0];
      }
      one = same;
    }
  }
#pragma unroll
  for (int s = 0; s < NS; ++s) dst[s] = (uint8_t)(one ? m[0] : m[s]);
}

// groups: one lane per group of GROUP chunks
template <int ORDER>
__global__ void __launch_bounds__(256) sample_groups_kernel(SampleArgs a) {
  constexpr int NS = contexts(ORDER);
  for (int64_t g = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; g < a.groups; g += (int64_t)gridDim.x * blockDim.x) {
    const int64_t c0 = g * GROUP, c1 = c0 + GROUP < a.chunks ? c0 + GROUP : a.chunks;
    compose<NS>(a.cmap, c0, c1, a.gmap + g * NS);
  }
}

// walk: one block.  LDS: WALK_TILE * contexts(ORDER) bytes.
template <int ORDER>
__global__ void __launch_bounds__(256) sample_walk_kernel(SampleArgs a) {
  constexpr int NS = contexts(ORDER);
  HIP_DYNAMIC_SHARED(uint8_t, walk_tile);
  uint32_t e = a.carry[0];
  for (int64_t g0 = 0; g0 < a.groups; g0 += WALK_TILE) {
    const int cnt = a.groups - g0 < WALK_TILE ? (int)(a.groups - g0) : WALK_TILE;
    __syncthreads();
    for (int i = (int)threadIdx.x; i < cnt * NS; i += (int)blockDim.x) walk_tile[i] = a.gmap[g0 * NS + i];
    __syncthreads();
    if (threadIdx.x == 0)
      for (int i = 0; i < cnt; ++i) {
        a.gentry[g0 + i] = (uint8_t)e;
        e = walk_tile[i * NS + (int)e];
      }
  }
  if (threadIdx.x == 0) a.carry[0] = (uint8_t)e;
}

// entries: one lane per group
template <int ORDER>
__global__ void __launch_bounds__(256) sample_entries_kernel(SampleArgs a) {
  constexpr int NS = contexts(ORDER);
  for (int64_t g = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; g < a.groups; g += (int64_t)gridDim.x * blockDim.x) {
    const int64_t c0 = g * GROUP, c1 = c0 + GROUP < a.chunks ? c0 + GROUP : a.chunks;
    uint32_t e = a.gentry[g];
    for (int64_t c = c0; c < c1; ++c) {
      a.centry[c] = (uint8_t)e;
      e = a.cmap[c * NS + (int)e];
    }
  }
}

// letters: one lane per chunk.  LDS: contexts(ORDER) * 16 bytes.
template <int ORDER>
__global__ void __launch_bounds__(256) sample_letters_kernel(SampleArgs a) {
  constexpr int NS = contexts(ORDER);
  HIP_DYNAMIC_SHARED(uint4, letters_rows);
  for (int e = (int)threadIdx.x; e < NS; e += (int)blockDim.x) letters_rows[e] = a.rows[e];
  __syncthreads();
  for (int64_t c = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; c < a.chunks; c += (int64_t)gridDim.x * blockDim.x) {
    const int64_t p0 = c * a.chunk, p1 = p0 + a.chunk < a.n ? p0 + a.chunk : a.n;
    uint32_t s = a.centry[c];
    int64_t P = a.pos0 + p0;
    Philox4 r = draw_block(P, a.seed_lo, a.seed_hi);
    for (int64_t p = p0; p < p1; p += 4) {
      const int cnt = p1 - p < 4 ? (int)(p1 - p) : 4;
      const uint32_t tw = codes4(a.tmpl, p, cnt);
      uint32_t ow = 0;
#pragma unroll 1
      for (int i = 0; i < cnt; ++i) {
        const uint32_t u = philox_pick(r, (int)(P & 3)), code = (tw >> (8 * i)) & 255u;
        uint32_t letter = 4u;
        if (code > 3u) s = 0u;
        else s = advance(letters_rows[s], u, letter);
        ow |= letter << (8 * i);
        ++P;
        if ((P & 3) == 0) r = draw_block(P, a.seed_lo, a.seed_hi);
      }
      if (cnt == 4) *reinterpret_cast<uint32_t*>(a.out + p) = ow;
      else
        for (int i = 0; i < cnt; ++i) a.out[p + i] = (uint8_t)(ow >> (8 * i));
    }
  }
}

}  // namespace bg
}  // namespace crbm
