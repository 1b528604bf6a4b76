// Motif comparison on the device (gfx950, wave64): every placement of every query motif on every target motif, in both
// orientations, scored in integers and turned into a p-value by the exact null distribution of the query's columns
// against the pool of target columns.  Model-independent: compiled ahead of time into libcrbm_hip.so (crbm_api.hip:
// crbm_motif_compare, crbm_motif_compare_null) and, with g++ against tests/emu/shim, into the emulation program
// tests/emu/compare_main.cpp.  DESIGN.md section 5, "Motif comparison".
//
// A column is four uint16 (A, C, G, T), p * 4096 rounded, packed into a uint2.  The score of two columns is the integer
//   D = sum_a (x_a - y_a)^2;  sim = 2^25 - min(D, 2^25);  bin = (sim * (B - 1) + 2^24) >> 25   in [0, B).
// Three stages per group of queries (a group's tail tables and output rows fit CRBM_COMPARE_BYTES):
//   counts_kernel  count[i][y]: the pool columns whose bin against query column i is y.  Counters in the LDS, flushed
//                  with integer atomics: integer adds commute, any geometry gives the same counts.
//   conv_kernel    pmf_{i,l}[x] = sum_y pmf_{i,l-1}[x - y] * col[i+l-1][y], col = (double)count * invC, one launch per
//                  length l over (tile of cells, start i, query); every cell is a gather added in ascending y from 0.0,
//                  so the bits do not depend on the tiling.  No atomics.
//   tail_kernel    tail[x] = tail[x + 1] + pmf[x], x descending, in place: one lane per (query, i, l) array.
//   place_kernel   grid (tile of targets, query): one lane sums the bins of one diagonal (target, strand, offset), looks
//                  its tail up, and the block reduces to the lexicographic minimum of (p, strand, offset) per target.
// The tables of a query lie packed by start i ascending, then length l = 1 .. m - i ascending, G_l + 1 doubles each,
// G_l = l (B - 1) + 1 (table_offset).  The build compiles with -ffp-contract=off: a product and an add round separately.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <algorithm>
#include <cmath>
#include <cstdlib>
#include <vector>

namespace crbm {
namespace compare {

constexpr int MAX_WIDTH = 64;
constexpr int MIN_BINS = 2, MAX_BINS = 256;
constexpr int SCALE = 4096;                       // a probability of 1
constexpr int TILE_DEFAULT = 32;                  // targets per block of place_kernel (CRBM_COMPARE_TILE)
constexpr int TILE_MAX = 64;
constexpr int CONV_TILE = 256;                    // cells per block of conv_kernel
constexpr int COUNT_CHUNK = 2048;                 // pool columns per block of counts_kernel, at least
constexpr int COUNT_BLOCKS = 256;                 // blocks per query of counts_kernel, at most
constexpr int64_t BYTES_DEFAULT = (int64_t)1 << 30;   // the tables and output rows of a group (CRBM_COMPARE_BYTES)
constexpr int64_t MAX_POOL = 2147483647;
constexpr int64_t OUT_BYTES = 8 + 4 + 1 + 4 + 4;  // of one (query, target) pair
constexpr int MAX_GRID_YZ = 65535;
constexpr uint32_t NOT_EVALUATED = 0xffffu;       // the score slot of a diagonal that is not a placement

// ---- the layout of a query's tables -----------------------------------------------------------------------------------
// sum_{l' = 1 .. L} (G_l' + 1)
__host__ __device__ inline int64_t lengths_up_to(int B, int L) { return (int64_t)(B - 1) * L * (L + 1) / 2 + 2 * (int64_t)L; }
// sum_{k = 1 .. n} lengths_up_to(k): the doubles of a query of width n
__host__ __device__ inline int64_t table_elems(int B, int n) { return (int64_t)(B - 1) * n * (n + 1) * (n + 2) / 6 + (int64_t)n * (n + 1); }
// where tail_{i,l} of a query of width m begins, 1 <= l <= m - i
__host__ __device__ inline int64_t table_offset(int B, int m, int i, int l) {
  return table_elems(B, m) - table_elems(B, m - i) + lengths_up_to(B, l - 1);
}

__host__ __device__ inline uint2 reverse_letters(uint2 x) {
  uint2 r;
  r.x = (x.y >> 16) | (x.y << 16);
  r.y = (x.x >> 16) | (x.x << 16);
  return r;
}

__host__ __device__ inline uint32_t bin_of(uint2 x, uint2 y, uint32_t Bm1) {
  const int32_t d0 = (int32_t)(x.x & 0xffffu) - (int32_t)(y.x & 0xffffu), d1 = (int32_t)(x.x >> 16) - (int32_t)(y.x >> 16);
  const int32_t d2 = (int32_t)(x.y & 0xffffu) - (int32_t)(y.y & 0xffffu), d3 = (int32_t)(x.y >> 16) - (int32_t)(y.y >> 16);
  const uint32_t D = (uint32_t)(d0 * d0) + (uint32_t)(d1 * d1) + (uint32_t)(d2 * d2) + (uint32_t)(d3 * d3);     // at most 2^26
  const uint32_t sim = (1u << 25) - (D < (1u << 25) ? D : (1u << 25));
  return (uint32_t)(((uint64_t)sim * Bm1 + (1u << 24)) >> 25);
}

inline int64_t env_i64(const char* name, int64_t dflt) {
  const char* v = getenv(name);
  return (v && *v) ? atoll(v) : dflt;
}
inline int tile_targets(int64_t want) { return (int)(want < 1 ? 1 : want > TILE_MAX ? TILE_MAX : want); }

// ---- the plan (host): what is refused, and the groups of queries; shared by crbm_api.hip and the emulation program -----
struct Plan {
  std::vector<int32_t> group_start;   // [groups + 1]: the queries [group_start[g], group_start[g + 1]) form group g
  std::vector<int64_t> table_base;    // [K]: where a query's tables begin in its group's buffer, in doubles
  int64_t table_elems_max = 0;        // doubles of the largest group's tables
  int64_t count_elems_max = 0;        // counters of the largest group: its query columns * bins
  int32_t rows_max = 0;               // queries of the largest group
  int32_t tile = 0, width_max_targets = 0;
  int64_t tcols = 0;                  // target columns
  int groups() const { return (int)group_start.size() - 1; }
};

inline const char* starts_refusal(const int32_t* start, int32_t n) {
  if (start[0] != 0) return "a start array must begin at 0";
  for (int32_t e = 0; e < n; ++e) {
    if (start[e + 1] <= start[e]) return "a start array must ascend";
    if (start[e + 1] - start[e] > MAX_WIDTH) return "a width must lie in [1, 64]";
  }
  return nullptr;
}
inline const char* entries_refusal(const uint16_t* cols, int64_t n) {
  for (int64_t e = 0; e < n * 4; ++e)
    if (cols[e] > SCALE) return "an entry lies above 4096";
  return nullptr;
}

// What crbm_motif_compare refuses, or null with the plan filled.  budget: CRBM_COMPARE_BYTES; tile: CRBM_COMPARE_TILE.
inline const char* plan_or_refusal(const uint16_t* qcols, const int32_t* qstart, int32_t K, const uint16_t* tcols, const int32_t* tstart,
                                   int32_t N, int32_t bins, int32_t both, int32_t min_overlap, double invC, bool outputs,
                                   int64_t budget, int64_t tile, Plan* plan) {
  if (!qcols || !qstart || !tcols || !tstart || !outputs) return "null argument";
  if (K < 1 || N < 1) return "K and N must be at least 1";
  if (bins < MIN_BINS || bins > MAX_BINS) return "bins must lie in [2, 256]";
  if (min_overlap < 1) return "min_overlap must be at least 1";
  if (const char* why = starts_refusal(qstart, K)) return why;
  if (const char* why = starts_refusal(tstart, N)) return why;
  if ((int64_t)tstart[N] * (both ? 2 : 1) > MAX_POOL) return "the pool holds more than 2^31 - 1 columns";
  if (const char* why = entries_refusal(qcols, qstart[K])) return why;
  if (const char* why = entries_refusal(tcols, tstart[N])) return why;
  if (!(invC > 0.0) || !(invC <= 1.0)) return "invC must lie in (0, 1]";
  Plan p;
  p.tcols = tstart[N];
  p.tile = tile_targets(tile);
  for (int32_t t = 0; t < N; ++t) p.width_max_targets = std::max(p.width_max_targets, tstart[t + 1] - tstart[t]);
  p.table_base.assign((size_t)K, 0);
  if (budget < 1) budget = 1;
  const int64_t row_bytes = (int64_t)N * OUT_BYTES;
  int64_t used = 0, elems = 0;
  int32_t first = 0;
  p.group_start.push_back(0);
  for (int32_t q = 0; q < K; ++q) {
    const int64_t mine = table_elems(bins, qstart[q + 1] - qstart[q]);
    if (mine * 8 + row_bytes > budget) return "the tables of one query do not fit CRBM_COMPARE_BYTES";
    if (q > first && (used + mine * 8 + row_bytes > budget || q - first >= MAX_GRID_YZ)) {
      p.group_start.push_back(q);
      first = q;
      used = elems = 0;
    }
    p.table_base[(size_t)q] = elems;
    elems += mine;
    used += mine * 8 + row_bytes;
    p.table_elems_max = std::max(p.table_elems_max, elems);
    p.count_elems_max = std::max(p.count_elems_max, (int64_t)(qstart[q + 1] - qstart[first]) * bins);
    p.rows_max = std::max(p.rows_max, q - first + 1);
  }
  p.group_start.push_back(K);
  *plan = std::move(p);
  return nullptr;
}

// ---- kernels ----------------------------------------------------------------------------------------------------------
struct Motifs {
  const uint2* qcols;        // every query column
  const int32_t* qstart;     // [K + 1]
  const uint2* tcols;        // every target column
  const int32_t* tstart;     // [N + 1]
};

struct CountArgs {
  Motifs m;
  uint32_t* counts;          // the group's counters, zeroed: [query columns of the group][bins]
  int64_t tcols;
  int32_t q0, bins, both;    // q0: the first query of the group
};

// grid (chunks of the pool, queries of the group).  LDS: width * bins uint32.
__global__ void __launch_bounds__(256) counts_kernel(CountArgs a) {
  HIP_DYNAMIC_SHARED(uint32_t, compare_counters);
  uint32_t* cnt = compare_counters;
  const int q = a.q0 + (int)blockIdx.y;
  const int c0 = a.m.qstart[q], m = a.m.qstart[q + 1] - c0, B = a.bins;
  for (int e = (int)threadIdx.x; e < m * B; e += (int)blockDim.x) cnt[e] = 0u;
  __syncthreads();
  const uint32_t Bm1 = (uint32_t)(B - 1);
  for (int64_t c = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; c < a.tcols; c += (int64_t)gridDim.x * blockDim.x) {
    const uint2 y = a.m.tcols[c], yr = reverse_letters(y);      // (the pool does not care where a column stood)
    for (int i = 0; i < m; ++i) {
      const uint2 x = a.m.qcols[c0 + i];
      atomicAdd(&cnt[i * B + (int)bin_of(x, y, Bm1)], 1u);
      if (a.both) atomicAdd(&cnt[i * B + (int)bin_of(x, yr, Bm1)], 1u);
    }
  }
  __syncthreads();
  uint32_t* out = a.counts + (int64_t)(c0 - a.m.qstart[a.q0]) * B;
  for (int e = (int)threadIdx.x; e < m * B; e += (int)blockDim.x)
    if (cnt[e]) atomicAdd(&out[e], cnt[e]);
}

struct NullArgs {
  const int32_t* qstart;
  const uint32_t* counts;    // the group's counters
  double* tables;            // the group's tables
  const int64_t* table_base; // [K]
  double invC;
  int32_t q0, bins, l, tiles; // conv_kernel: the length of this launch and its tiles of cells per start
};

// grid (tiles of CONV_TILE cells * starts i, queries of the group).  LDS: (2 * bins - 1 + CONV_TILE) doubles.
// Writes pmf_{i,l} into the first G_l doubles of the slot of tail_{i,l}.
__global__ void __launch_bounds__(256) conv_kernel(NullArgs a) {
  HIP_DYNAMIC_SHARED(double, compare_cells);
  const int q = a.q0 + (int)blockIdx.y, i = (int)blockIdx.x / a.tiles, l = a.l, B = a.bins;
  const int c0 = a.qstart[q], m = a.qstart[q + 1] - c0;
  if (i + l > m) return;                                         // (the whole block)
  const int G = l * (B - 1) + 1, Gp = G - (B - 1), x0 = ((int)blockIdx.x % a.tiles) * CONV_TILE;
  if (x0 >= G) return;
  const int n = G - x0 < CONV_TILE ? G - x0 : CONV_TILE;
  double* col = compare_cells;
  double* prev = compare_cells + B;                                  // pmf_{i,l-1}[x0 - (B - 1) .. x0 + n), zero outside its support
  const uint32_t* cnt = a.counts + (int64_t)(c0 - a.qstart[a.q0] + i + l - 1) * B;
  for (int y = (int)threadIdx.x; y < B; y += (int)blockDim.x) col[y] = (double)cnt[y] * a.invC;
  double* T = a.tables + a.table_base[q];
  const double* src = l > 1 ? T + table_offset(B, m, i, l - 1) : nullptr;
  for (int e = (int)threadIdx.x; e < n + B - 1; e += (int)blockDim.x) {
    const int x = x0 - (B - 1) + e;
    prev[e] = (x < 0 || x >= Gp) ? 0.0 : (l > 1 ? src[x] : 1.0);
  }
  __syncthreads();
  double* dst = T + table_offset(B, m, i, l) + x0;
  for (int e = (int)threadIdx.x; e < n; e += (int)blockDim.x) {
    const int x = x0 + e;
    const int ylo = x - (Gp - 1) > 0 ? x - (Gp - 1) : 0, yhi = x < B - 1 ? x : B - 1;
    double acc = 0.0;
    for (int y = ylo; y <= yhi; ++y) acc += prev[e + (B - 1) - y] * col[y];
    dst[e] = acc;
  }
}

// grid (lanes over the (i, l) arrays of the widest query, queries of the group).  In place: pmf -> tail.
__global__ void __launch_bounds__(64) tail_kernel(NullArgs a) {
  const int q = a.q0 + (int)blockIdx.y, B = a.bins;
  const int m = a.qstart[q + 1] - a.qstart[q];
  int e = (int)(blockIdx.x * blockDim.x + threadIdx.x);
  if (e >= m * (m + 1) / 2) return;
  int i = 0;
  while (e >= m - i) { e -= m - i; ++i; }
  const int l = e + 1, G = l * (B - 1) + 1;
  double* t = a.tables + a.table_base[q] + table_offset(B, m, i, l);
  double acc = 0.0;
  t[G] = 0.0;
  for (int x = G - 1; x >= 0; --x) {
    acc = acc + t[x];
    t[x] = acc;
  }
}

struct PlaceArgs {
  Motifs m;
  const double* tables;      // the group's tables
  const int64_t* table_base; // [K]
  double* p_min;             // the group's output rows: [queries of the group][N]
  int32_t* offset;
  int8_t* strand;
  int32_t* overlap;
  int32_t* n_off;
  int32_t q0, N, bins, both, min_overlap, tile;
  int32_t diagonals;         // what the LDS holds per target and strand: the group's widest query + the widest target - 1
};

// bytes of the LDS of place_kernel
__host__ __device__ inline size_t place_lds(int tile, int diagonals) {
  return (size_t)tile * 8 + 2 * MAX_WIDTH * 8 + (size_t)tile * MAX_WIDTH * 8 + (size_t)tile * 4 + ((size_t)tile * 2 * diagonals * 2 + 7) / 8 * 8;
}

// grid (tiles of targets, queries of the group)
__global__ void __launch_bounds__(256) place_kernel(PlaceArgs a) {
  HIP_DYNAMIC_SHARED(unsigned long long, compare_words);
  unsigned long long* best = compare_words;                                   // [tile]: the bits of the smallest p
  uint2* qc = reinterpret_cast<uint2*>(best + a.tile);                         // [2][MAX_WIDTH]: the query; its letters reversed
  uint2* tc = qc + 2 * MAX_WIDTH;                                              // the tile's columns
  uint32_t* bidx = reinterpret_cast<uint32_t*>(tc + (size_t)a.tile * MAX_WIDTH);   // [tile]: the first diagonal that holds it
  uint16_t* score = reinterpret_cast<uint16_t*>(bidx + a.tile);                // [tile][strands][diagonals]
  const int q = a.q0 + (int)blockIdx.y, B = a.bins, strands = a.both ? 2 : 1;
  const int c0 = a.m.qstart[q], m = a.m.qstart[q + 1] - c0;
  const int t0 = (int)blockIdx.x * a.tile, nt = a.N - t0 < a.tile ? a.N - t0 : a.tile;
  const int base = a.m.tstart[t0], ncols = a.m.tstart[t0 + nt] - base;
  for (int e = (int)threadIdx.x; e < ncols; e += (int)blockDim.x) tc[e] = a.m.tcols[base + e];
  for (int e = (int)threadIdx.x; e < m; e += (int)blockDim.x) {
    const uint2 x = a.m.qcols[c0 + e];
    qc[e] = x;
    qc[MAX_WIDTH + e] = reverse_letters(x);
  }
  for (int e = (int)threadIdx.x; e < nt; e += (int)blockDim.x) { best[e] = ~0ull; bidx[e] = ~0u; }
  __syncthreads();
  const int D = a.diagonals, per_target = strands * D, items = nt * per_target;
  const uint32_t Bm1 = (uint32_t)(B - 1);
  const double* T = a.tables + a.table_base[q];
  // one diagonal per lane: its integer score, its tail, the smallest bits per target
  for (int it = (int)threadIdx.x; it < items; it += (int)blockDim.x) {
    const int t = it / per_target, r = it - t * per_target, s = r >= D ? 1 : 0, d = r - s * D;
    const int tb = a.m.tstart[t0 + t] - base, n = a.m.tstart[t0 + t + 1] - a.m.tstart[t0 + t];
    const int o = d - (n - 1), need = min(a.min_overlap, min(m, n));
    const int i0 = o > 0 ? o : 0, j0 = o < 0 ? -o : 0, l = min(m - i0, n - j0);
    uint32_t S = NOT_EVALUATED;
    if (o < m && l >= need) {
      S = 0;
      const uint2* x = qc + s * MAX_WIDTH + i0;
      if (s) for (int u = 0; u < l; ++u) S += bin_of(x[u], tc[tb + n - 1 - j0 - u], Bm1);      // the reverse complement's column j
      else for (int u = 0; u < l; ++u) S += bin_of(x[u], tc[tb + j0 + u], Bm1);               // is column n - 1 - j, letters reversed
      const double p = T[table_offset(B, m, i0, l) + S];
      atomicMin(&best[t], (unsigned long long)__double_as_longlong(p));       // (p >= +0: its bits order as it does)
    }
    score[it] = (uint16_t)S;
  }
  __syncthreads();
  // ties on bit-equal p: strand + before -, then the smaller offset -- the smallest diagonal index
  for (int it = (int)threadIdx.x; it < items; it += (int)blockDim.x) {
    const uint32_t S = score[it];
    if (S == NOT_EVALUATED) continue;
    const int t = it / per_target, r = it - t * per_target, s = r >= D ? 1 : 0, d = r - s * D;
    const int n = a.m.tstart[t0 + t + 1] - a.m.tstart[t0 + t];
    const int o = d - (n - 1), i0 = o > 0 ? o : 0, j0 = o < 0 ? -o : 0, l = min(m - i0, n - j0);
    const double p = T[table_offset(B, m, i0, l) + S];
    if ((unsigned long long)__double_as_longlong(p) == best[t]) atomicMin(&bidx[t], (uint32_t)r);
  }
  __syncthreads();
  for (int t = (int)threadIdx.x; t < nt; t += (int)blockDim.x) {
    const int n = a.m.tstart[t0 + t + 1] - a.m.tstart[t0 + t], need = min(a.min_overlap, min(m, n));
    const int r = (int)bidx[t], s = r >= D ? 1 : 0, o = r - s * D - (n - 1);
    const int i0 = o > 0 ? o : 0, j0 = o < 0 ? -o : 0;
    const int64_t at = (int64_t)blockIdx.y * a.N + t0 + t;
    a.p_min[at] = __longlong_as_double((long long)best[t]);
    a.offset[at] = o;
    a.strand[at] = s ? -1 : 1;
    a.overlap[at] = min(m - i0, n - j0);
    a.n_off[at] = strands * (m + n - 1 - 2 * (need - 1));       // the lengths 1 .. need - 1 occur once at either end
  }
}

// ---- launch geometry (host) -------------------------------------------------------------------------------------------
inline unsigned count_blocks(int64_t tcols) {
  const int64_t b = (tcols + COUNT_CHUNK - 1) / COUNT_CHUNK;
  return (unsigned)(b < 1 ? 1 : b > COUNT_BLOCKS ? COUNT_BLOCKS : b);
}
inline size_t counts_lds(int width, int bins) { return (size_t)width * bins * 4; }
inline size_t conv_lds(int bins) { return (size_t)(2 * bins - 1 + CONV_TILE) * 8; }
inline unsigned conv_tiles(int bins, int l) { return (unsigned)((l * (bins - 1) + 1 + CONV_TILE - 1) / CONV_TILE); }
inline int widest(const int32_t* start, int from, int to) {
  int w = 0;
  for (int e = from; e < to; ++e) w = std::max(w, start[e + 1] - start[e]);
  return w;
}

}  // namespace compare
}  // namespace crbm
