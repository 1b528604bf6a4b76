// t-SNE on the device (gfx950, wave64): exact k nearest neighbours, conditional affinities, and gradient descent on
// the KL divergence with an exact O(n^2) repulsion.  Model-independent: compiled ahead of time into libcrbm_hip.so
// (crbm_api.hip: crbm_tsne_neighbors / _affinities / _descend) and, with g++ against tests/emu/shim, into the
// emulation program tests/emu/tsne_main.cpp.  DESIGN.md section 5, "t-SNE".
//
// Every sum has an order that depends on n alone, never on the launch geometry, and nothing is combined with a float
// atomic: two runs return the same bits, and so do two grids.
//  * d2(i,j) = sum_d (x_id - x_jd)^2 in float32, d ascending, difference form, no fused multiply-add (the build sets
//    -ffp-contract=off): a float32 NumPy loop over d gives the same bits.
//  * repulsion: the j range is cut into tsne::slices(n) slices of whole tiles of TJ points; inside a tile four
//    accumulators take j mod 4 and fold as (a0 + a1) + (a2 + a3); a slice adds its tiles in order; the slices of a row
//    are added in order (combine kernel).
//  * float64 sums (Z, KL): chunks of SUM_CHUNK consecutive rows by a binary tree over the chunk's slots, the chunk sums
//    by a strided pass into SUM_CHUNK slots and the same tree.
#pragma once
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

namespace crbm {
namespace tsne {

constexpr int KNN_MAX_K = 1024;      // a wave's list: k (d2, j) pairs in the LDS, 8 KB at the cap
constexpr int KNN_MAX_D = 256;       // a tile of 64 candidate rows and the block's query rows stay within the LDS
constexpr int KNN_TILE = 64;         // candidates per step: one per lane
constexpr int TJ = 256;              // points of a repulsion tile
constexpr int SUM_CHUNK = 256;       // rows of a float64 chunk sum
constexpr int BISECTION_STEPS = 100;
constexpr int MAX_SLICES = 64;
constexpr int64_t MAX_N = 1 << 30;          // indices and their tile arithmetic stay within int32
constexpr double KL_EPS = 2.2e-16;

// ---- what the entry points refuse (host; the emulation program prints these too) --------------------------------
inline const char* neighbors_refusal(int64_t n, int32_t D, int32_t k) {
  if (n < 2) return "t-SNE needs at least two rows";
  if (n > MAX_N) return "too many rows";
  if (D < 1) return "D must be at least 1";
  if (D > KNN_MAX_D) return "D above 256: a tile of candidate rows does not fit the LDS";
  if (k < 1 || (int64_t)k > n - 1) return "k must lie in [1, n - 1]";
  if (k > KNN_MAX_K) return "k above 1024: a wave's neighbour list does not fit the LDS";
  return nullptr;
}
inline const char* affinities_refusal(int64_t n, int32_t k, float perplexity) {
  if (n < 2) return "t-SNE needs at least two rows";
  if (n > MAX_N) return "too many rows";
  if (k < 1 || (int64_t)k > n - 1) return "k must lie in [1, n - 1]";
  if (k > KNN_MAX_K) return "k above 1024";
  if (!(perplexity > 0.f) || !(perplexity < (float)k + 1.f) || !(perplexity <= 3.0e38f)) return "the perplexity must be finite, positive and below k + 1";
  return nullptr;
}
inline const char* descend_refusal(int64_t n, const int64_t* indptr, const int32_t* indices, int32_t iterations) {
  if (n < 2) return "t-SNE needs at least two rows";
  if (n > MAX_N) return "too many rows";
  if (iterations < 0) return "iterations must not be negative";
  if (indptr[0] != 0) return "indptr must start at 0";
  for (int64_t i = 0; i < n; ++i)
    if (indptr[i + 1] < indptr[i]) return "indptr must ascend";
  for (int64_t e = 0; e < indptr[n]; ++e)
    if (indices[e] < 0 || (int64_t)indices[e] >= n) return "an index outside [0, n)";
  return nullptr;
}

// slices of the repulsion's j range and tiles per slice: a function of n alone (it fixes the order of the sums).
// Small n gets slices so that the grid fills the machine: about 2048 blocks of TJ rows x one slice.
inline int slice_tiles(int64_t n) {
  const int64_t tiles = (n + TJ - 1) / TJ;
  int64_t want = (2048 + tiles - 1) / tiles;
  if (want > MAX_SLICES) want = MAX_SLICES;
  if (want > tiles) want = tiles;
  return (int)((tiles + want - 1) / want);
}
inline int slices(int64_t n) {
  const int64_t tiles = (n + TJ - 1) / TJ, per = slice_tiles(n);
  return (int)((tiles + per - 1) / per);
}
__host__ __device__ inline int64_t sum_chunks(int64_t n) { return (n + SUM_CHUNK - 1) / SUM_CHUNK; }
__host__ __device__ inline int knn_stride(int D) { return D | 1; }   // odd: lane l reads word l * stride + d, one bank each
inline size_t knn_lds_bytes(int D, int k, int waves) {
  return ((size_t)(KNN_TILE + waves) * knn_stride(D) + (size_t)waves * k * 2) * 4;
}

// ---- wave-wide helpers ------------------------------------------------------------------------------------------
// lanes of a wave exchange data through the LDS: stores before, loads after
__device__ __forceinline__ void wave_sync() {
#if defined(__HIP_DEVICE_COMPILE__)
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
#else
  __builtin_amdgcn_wave_barrier();
#endif
}
__device__ __forceinline__ float lane_value(float v, int src) {
  int b;
  __builtin_memcpy(&b, &v, 4);
  b = __builtin_amdgcn_readlane(b, src);
  __builtin_memcpy(&v, &b, 4);
  return v;
}
__device__ __forceinline__ bool key_less(float d, int j, float kd, int kj) { return d < kd || (d == kd && j < kj); }

// ---- a. exact k nearest neighbours --------------------------------------------------------------------------------
struct KnnArgs {
  const float* X;     // (n, D)
  int32_t* idx;       // (n, k)
  float* d2;          // (n, k)
  int n, D, k;
};

// (nd, nj) sorts before the list's last entry: the whole wave puts it in its place.  The place by a binary search every
// lane makes alike (broadcast reads), the shift from the top down, 64 entries a step, loads before stores.
__device__ __forceinline__ void knn_insert(float* ld, int32_t* lj, int k, float nd, int nj, int lane) {
  int lo = 0, hi = k - 1;
  while (lo < hi) {
    const int mid = (lo + hi) >> 1;
    if (key_less(ld[mid], lj[mid], nd, nj)) lo = mid + 1; else hi = mid;
  }
  for (int top = k - 1; top > lo; top -= 64) {
    const int t = top - lane;
    const bool act = t > lo;
    float vd = 0.f;
    int32_t vj = 0;
    if (act) { vd = ld[t - 1]; vj = lj[t - 1]; }
    wave_sync();
    if (act) { ld[t] = vd; lj[t] = vj; }
    wave_sync();
  }
  if (lane == 0) { ld[lo] = nd; lj[lo] = nj; }
  wave_sync();
}

// One wave per query row, blockDim / 64 queries per block at a time; tiles of 64 candidate rows go through the LDS and
// serve every wave of the block.  LDS: knn_lds_bytes(D, k, waves).
__global__ void __launch_bounds__(512) tsne_knn_kernel(KnnArgs a) {
  HIP_DYNAMIC_SHARED(float, knn_smem);
  const int waves = (int)(blockDim.x >> 6), wave = (int)(threadIdx.x >> 6), lane = (int)(threadIdx.x & 63u);
  const int n = a.n, D = a.D, k = a.k, stride = knn_stride(D);
  float* cand = knn_smem;
  float* myq = cand + (size_t)KNN_TILE * stride + (size_t)wave * stride;
  float* ld = cand + (size_t)(KNN_TILE + waves) * stride + (size_t)wave * k;
  int32_t* lj = reinterpret_cast<int32_t*>(cand + (size_t)(KNN_TILE + waves) * stride + (size_t)waves * k) + (size_t)wave * k;
  const float INF = __builtin_inff();
  const int groups = (n + waves - 1) / waves;
  for (int g = (int)blockIdx.x; g < groups; g += (int)gridDim.x) {
    const int q = g * waves + wave;                  // the last group may have waves without a row: they only keep step
    const bool live = q < n;
    if (live) {
      for (int d = lane; d < D; d += 64) myq[d] = a.X[(size_t)q * D + d];
      for (int p = lane; p < k; p += 64) { ld[p] = INF; lj[p] = 0x7fffffff; }
    }
    float kd = INF;
    int kj = 0x7fffffff;
    for (int c0 = 0; c0 < n; c0 += KNN_TILE) {
      const int rows = min(KNN_TILE, n - c0);
      __syncthreads();                               // the tile is free (and the wave's row and list are written)
      for (int e = (int)threadIdx.x; e < rows * D; e += (int)blockDim.x) {
        const int r = e / D;
        cand[(size_t)r * stride + (e - r * D)] = a.X[(size_t)c0 * D + e];
      }
      __syncthreads();
      if (live) {
        float acc = 0.f;
        if (lane < rows) {
          const float* c = cand + (size_t)lane * stride;
          for (int d = 0; d < D; ++d) {
            const float diff = myq[d] - c[d];
            acc = acc + diff * diff;
          }
        }
        const int j = c0 + lane;
        unsigned long long m = __ballot(lane < rows && j != q && key_less(acc, j, kd, kj));
        while (m) {                                  // ascending lane = ascending j
          const int src = __ffsll(m) - 1;
          m &= m - 1;
          const float nd = lane_value(acc, src);
          const int nj = c0 + src;
          if (key_less(nd, nj, kd, kj)) {            // the bar may have come down since the ballot
            knn_insert(ld, lj, k, nd, nj, lane);
            kd = ld[k - 1];
            kj = lj[k - 1];
          }
        }
      }
    }
    if (live)
      for (int p = lane; p < k; p += 64) {
        a.idx[(size_t)q * k + p] = lj[p];
        a.d2[(size_t)q * k + p] = ld[p];
      }
  }
}

// ---- b. conditional affinities ----------------------------------------------------------------------------------------
struct AffinityArgs {
  const float* d2;    // (n, k)
  float* p;           // (n, k)
  float* beta;        // (n)
  int n, k;
  double target;      // log(perplexity)
};

// One thread per row, float64, j ascending.  Bisection on beta from 1, doubling or halving while a bound is open,
// BISECTION_STEPS evaluations.  The row's smallest d2 is subtracted inside the exponent, so the largest term is 1 and
// the sum is never 0.  A row of equal distances has entropy log k whatever beta is: beta ends at 2^+-100, finite in
// float32, and p is uniform.
__global__ void __launch_bounds__(256) tsne_affinity_kernel(AffinityArgs a) {
  const int k = a.k;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < a.n; i += (int64_t)gridDim.x * blockDim.x) {
    const float* row = a.d2 + (size_t)i * k;
    float dmin = row[0];
    for (int j = 1; j < k; ++j) dmin = fminf(dmin, row[j]);
    double beta = 1.0, lo = 0.0, hi = 0.0;
    bool lo_open = true, hi_open = true;
    for (int step = 0; step < BISECTION_STEPS; ++step) {
      double S = 0.0, SD = 0.0;
      for (int j = 0; j < k; ++j) {
        const double dd = (double)row[j] - (double)dmin;
        const double e = exp(-beta * dd);
        S += e;
        SD += dd * e;
      }
      const double H = log(S) + beta * SD / S;
      if (H > a.target) {                            // too flat: beta goes up
        lo = beta; lo_open = false;
        beta = hi_open ? beta * 2.0 : 0.5 * (beta + hi);
      } else {
        hi = beta; hi_open = false;
        beta = lo_open ? beta * 0.5 : 0.5 * (beta + lo);
      }
    }
    const float bf = (float)beta;
    const double b = (double)bf;                     // p belongs to the beta that is returned
    double S = 0.0;
    for (int j = 0; j < k; ++j) S += exp(-b * ((double)row[j] - (double)dmin));
    for (int j = 0; j < k; ++j) a.p[(size_t)i * k + j] = (float)(exp(-b * ((double)row[j] - (double)dmin)) / S);
    a.beta[i] = bf;
  }
}

// ---- c. gradient descent ---------------------------------------------------------------------------------------------
// fixed-order float64 sum of the SUM_CHUNK slots of `buf` (LDS), any blockDim; the result is in buf[0] for every thread
__device__ __forceinline__ void chunk_tree(double* buf) {
  __syncthreads();
  for (int h = SUM_CHUNK / 2; h >= 1; h >>= 1) {
    for (int e = (int)threadIdx.x; e < h; e += (int)blockDim.x) buf[e] += buf[e + h];
    __syncthreads();
  }
}

struct RepulsionArgs {
  const float2* y;    // (n)
  float4* part;       // (slices, n): R.x, R.y, s (self included: exactly 0 is added for it), 0
  int n, slices, slice_tiles;
};

// the four accumulator sets of a tile
struct RepAcc {
  float x[4], y[4], s[4];
};

// One pair: 2 subtractions, 4 fused multiply-adds (written out: the build does not contract), an addition, a multiply
// and v_rcp_f32: nine vector instructions, the reciprocal at a quarter of the rate.  `self` (only in the tile that holds the block's own rows) adds
// an exact zero for j = i.
template <bool SELF>
__device__ __forceinline__ void rep_pair(float2 yi, float2 yj, bool self, float& ax, float& ay, float& as) {
  const float dx = yi.x - yj.x, dy = yi.y - yj.y;
  const float t = fmaf(dx, dx, fmaf(dy, dy, 1.0f));
  float w = __builtin_amdgcn_rcpf(t);
  if (SELF) w = self ? 0.f : w;
  const float w2 = w * w;
  as = as + w;
  ax = fmaf(w2, dx, ax);
  ay = fmaf(w2, dy, ay);
}

template <bool SELF>
__device__ __forceinline__ void rep_tile(const float2* tile, int cnt, float2 yi, int self_at, RepAcc& acc) {
  const int whole = cnt & ~3;
  for (int j = 0; j < whole; j += 4) {
#pragma unroll
    for (int u = 0; u < 4; ++u) rep_pair<SELF>(yi, tile[j + u], j + u == self_at, acc.x[u], acc.y[u], acc.s[u]);
  }
  for (int j = whole; j < cnt; ++j) rep_pair<SELF>(yi, tile[j], j == self_at, acc.x[j & 3], acc.y[j & 3], acc.s[j & 3]);
}

// R_i and s_i over one slice of j: y_j tiles in the LDS (every lane reads the same address: a broadcast), y_i in
// registers.  grid (row blocks, slices); blockDim divides TJ, so a block's rows lie in one tile.  LDS: TJ * 8 bytes.
__global__ void __launch_bounds__(256) tsne_repulsion_kernel(RepulsionArgs a) {
  HIP_DYNAMIC_SHARED(float2, rep_tile_lds);
  const int n = a.n;
  const int j0 = (int)blockIdx.y * a.slice_tiles * TJ;
  const int j1 = (int64_t)j0 + (int64_t)a.slice_tiles * TJ < (int64_t)n ? j0 + a.slice_tiles * TJ : n;
  const int row_blocks = (n + (int)blockDim.x - 1) / (int)blockDim.x;
  for (int rb = (int)blockIdx.x; rb < row_blocks; rb += (int)gridDim.x) {
    const int i = rb * (int)blockDim.x + (int)threadIdx.x;
    float2 yi;
    yi.x = 0.f; yi.y = 0.f;
    if (i < n) yi = a.y[i];
    const int own_tile = rb * (int)blockDim.x / TJ * TJ;     // the tile that holds this block's rows
    float rx = 0.f, ry = 0.f, rs = 0.f;
    for (int t0 = j0; t0 < j1; t0 += TJ) {
      const int cnt = min(TJ, j1 - t0);
      __syncthreads();
      for (int e = (int)threadIdx.x; e < cnt; e += (int)blockDim.x) rep_tile_lds[e] = a.y[t0 + e];
      __syncthreads();
      RepAcc acc;
#pragma unroll
      for (int u = 0; u < 4; ++u) acc.x[u] = acc.y[u] = acc.s[u] = 0.f;
      if (t0 == own_tile) rep_tile<true>(rep_tile_lds, cnt, yi, i - t0, acc);
      else rep_tile<false>(rep_tile_lds, cnt, yi, -1, acc);
      rx = rx + ((acc.x[0] + acc.x[1]) + (acc.x[2] + acc.x[3]));
      ry = ry + ((acc.y[0] + acc.y[1]) + (acc.y[2] + acc.y[3]));
      rs = rs + ((acc.s[0] + acc.s[1]) + (acc.s[2] + acc.s[3]));
    }
    if (i < n) {
      float4 o;
      o.x = rx; o.y = ry; o.z = rs; o.w = 0.f;
      a.part[(size_t)blockIdx.y * n + i] = o;
    }
  }
}

struct CombineArgs {
  const float4* part;   // (slices, n)
  float4* rs;           // (n): R.x, R.y, s, 0
  double* chunk;        // (sum_chunks(n)): float64 sums of s over SUM_CHUNK rows
  int n, slices;
};

// a row's slices in order, and the chunk sums of s for Z.  LDS: SUM_CHUNK * 8 bytes.
__global__ void __launch_bounds__(256) tsne_combine_kernel(CombineArgs a) {
  HIP_DYNAMIC_SHARED(double, combine_lds);
  const int chunks = (int)sum_chunks(a.n);
  for (int c = (int)blockIdx.x; c < chunks; c += (int)gridDim.x) {
    for (int e = (int)threadIdx.x; e < SUM_CHUNK; e += (int)blockDim.x) {
      const int i = c * SUM_CHUNK + e;
      double v = 0.0;
      if (i < a.n) {
        float4 t = a.part[i];
        for (int s = 1; s < a.slices; ++s) {
          const float4 u = a.part[(size_t)s * a.n + i];
          t.x = t.x + u.x; t.y = t.y + u.y; t.z = t.z + u.z;
        }
        a.rs[i] = t;
        v = (double)t.z;
      }
      combine_lds[e] = v;
    }
    chunk_tree(combine_lds);
    if (threadIdx.x == 0) a.chunk[c] = combine_lds[0];
    __syncthreads();
  }
}

struct SumArgs {
  const double* in;
  double* out;
  int64_t m;
};

// chunk sums of `in` (m values): out[c] = tree sum of in[c * SUM_CHUNK ..].  LDS: SUM_CHUNK * 8 bytes.
__global__ void __launch_bounds__(256) tsne_chunk_sum_kernel(SumArgs a) {
  HIP_DYNAMIC_SHARED(double, chunk_lds);
  const int64_t chunks = sum_chunks(a.m);
  for (int64_t c = blockIdx.x; c < chunks; c += gridDim.x) {
    for (int e = (int)threadIdx.x; e < SUM_CHUNK; e += (int)blockDim.x) {
      const int64_t i = c * SUM_CHUNK + e;
      chunk_lds[e] = i < a.m ? a.in[i] : 0.0;
    }
    chunk_tree(chunk_lds);
    if (threadIdx.x == 0) a.out[c] = chunk_lds[0];
    __syncthreads();
  }
}

// out[0] = sum of the m values of `in`: slot e takes in[e], in[e + SUM_CHUNK], ... in order, then the tree.  One block.
__global__ void __launch_bounds__(256) tsne_final_sum_kernel(SumArgs a) {
  HIP_DYNAMIC_SHARED(double, final_lds);
  for (int e = (int)threadIdx.x; e < SUM_CHUNK; e += (int)blockDim.x) {
    double v = 0.0;
    for (int64_t i = e; i < a.m; i += SUM_CHUNK) v += a.in[i];
    final_lds[e] = v;
  }
  chunk_tree(final_lds);
  if (threadIdx.x == 0) a.out[0] = final_lds[0];
}

struct StepArgs {
  const int64_t* indptr;    // (n + 1)
  const int32_t* indices;
  const float* values;
  const float2* y;          // read: this iteration's positions (other rows' too)
  float2* y_out;            // written: the next positions (another buffer)
  float2* velocity;
  float2* gains;
  const float4* rs;         // the combine kernel's R and s
  const double* z;          // Z
  float2* grad;             // may be null
  double* kl_row;           // may be null: the row's share of the KL divergence
  int n, update;
  float exaggeration, learning_rate, momentum;
};

// attraction over the row's entries in order (one thread per row), gradient, and the update rule
__global__ void __launch_bounds__(256) tsne_step_kernel(StepArgs a) {
  const double Z = *a.z;
  const float inv_z = Z > 0.0 ? (float)(1.0 / Z) : 0.f;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < a.n; i += (int64_t)gridDim.x * blockDim.x) {
    const float2 yi = a.y[i];
    float ax = 0.f, ay = 0.f;
    double kl = 0.0;
    const int64_t e1 = a.indptr[i + 1];
    for (int64_t e = a.indptr[i]; e < e1; ++e) {
      const float2 yj = a.y[a.indices[e]];
      const float p = a.values[e];
      const float dx = yi.x - yj.x, dy = yi.y - yj.y;
      const float w = __builtin_amdgcn_rcpf(fmaf(dx, dx, fmaf(dy, dy, 1.0f)));   // the repulsion's w to the bit: q = w / Z sums to 1 over the pairs
      const float pw = p * w;
      ax = fmaf(pw, dx, ax);
      ay = fmaf(pw, dy, ay);
      if (a.kl_row) kl += (double)p * log(fmax((double)p, KL_EPS) / fmax((double)w / Z, KL_EPS));
    }
    if (a.kl_row) a.kl_row[i] = kl;
    const float4 r = a.rs[i];
    float2 g;
    g.x = 4.f * (a.exaggeration * ax - r.x * inv_z);
    g.y = 4.f * (a.exaggeration * ay - r.y * inv_z);
    if (a.grad) a.grad[i] = g;
    if (a.update) {
      float2 v = a.velocity[i], gn = a.gains[i];
      gn.x = fmaxf(v.x * g.x < 0.f ? gn.x + 0.2f : gn.x * 0.8f, 0.01f);
      gn.y = fmaxf(v.y * g.y < 0.f ? gn.y + 0.2f : gn.y * 0.8f, 0.01f);
      v.x = a.momentum * v.x - a.learning_rate * gn.x * g.x;
      v.y = a.momentum * v.y - a.learning_rate * gn.y * g.y;
      float2 o;
      o.x = yi.x + v.x; o.y = yi.y + v.y;
      a.gains[i] = gn;
      a.velocity[i] = v;
      a.y_out[i] = o;
    }
  }
}

}  // namespace tsne
}  // namespace crbm
