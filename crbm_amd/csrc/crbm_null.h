// The analytic null on the device (gfx950, wave64): the exact distribution of a quantised position weight matrix score
// under a Markov chain of order 0..3, by a dynamic programme over (context, integer score).  Model-independent: compiled
// ahead of time into libcrbm_hip.so (crbm_api.hip: crbm_score_distribution) and, with g++ against tests/emu/shim, into
// the emulation program tests/emu/null_main.cpp.  DESIGN.md section 5, "Analytic null".
//
// A row r is one (motif, strand) with the integer weights q[r][j][a] >= 0, j = 0 .. M - 1, min_a q[r][j][.] = 0.  With
// the contexts of crbm_background.h (partial contexts are ordinary states) and the transition probabilities P:
//   f_0[s][0] = init[s]
//   f_{j+1}[s'][Q] = sum over the pairs (s, a) with next_context(s, a) = s' of P[s][a] * f_j[s][Q - q[j][a]]
//   pmf[Q] = sum_s f_M[s][Q]
// Every cell is a gather of at most five terms (table: build_table), summed in the table's slot order; the contexts are
// summed in index order.  No atomics: the bits depend neither on the launch geometry, nor on the tile length, nor on how
// rows are grouped, nor on the kernel variant.  The build compiles with -ffp-contract=off: a product and an add round
// separately everywhere.
//
// One launch per motif position over (tile of Q, target context, row); the state ping-pongs between two global buffers of
// [rows][contexts][gmax] doubles.  Position j writes the cells below its reach, reach[j + 1] = sum_{i <= j} max_a q[i] + 1,
// and reads everything at or beyond reach[j] as zero, so no buffer is ever cleared.
//   step_plain_kernel     a lane owns cells of one target context: up to five strided global reads each.
//   step_siblings_kernel  the four full-length targets (l_2 .. l_m, a), a = 0..3, have the same sources, target a reading
//                         them at shift q[j][a]: one block serves the four, the source tiles and a halo of max_a q[j][a]
//                         staged in the LDS once.  Taken (CRBM_NULL_VARIANT=1) at positions whose halo fits the LDS.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <cmath>
#include <cstdlib>
#include <vector>

namespace crbm {
namespace null {

constexpr int MAX_ORDER = 3;
constexpr int MAX_M = 512;
constexpr int64_t MAX_G = (int64_t)1 << 24;
constexpr int PREDS = 5;                        // predecessor pairs of a target context, at most
constexpr int TILE_DEFAULT = 1024;              // cells of Q per block (CRBM_NULL_TILE)
constexpr int TILE_MIN = 8, TILE_MAX = 1 << 16;
constexpr int64_t BYTES_DEFAULT = (int64_t)1 << 30;   // both state buffers of a group of rows (CRBM_NULL_BYTES)
constexpr int LDS_BYTES = 64 << 10;             // what a block of the siblings kernel may stage
constexpr int VARIANT_DEFAULT = 0;              // CRBM_NULL_VARIANT: 0 plain gather, 1 sibling tiles through the LDS
constexpr int MAX_GRID_Y = 65535;

__host__ __device__ constexpr int pow4(int j) { return 1 << (2 * j); }
__host__ __device__ constexpr int contexts(int order) { return (pow4(order + 1) - 1) / 3; }
__host__ __device__ constexpr int context_base(int j) { return (pow4(j) - 1) / 3; }

// the context behind context s once letter a has been appended (crbm_background.h)
inline int next_context(int order, int s, int a) {
  int j = 0;
  while (j < order && s >= context_base(j + 1)) ++j;
  const int v = (s - context_base(j)) * 4 + a;
  return j < order ? context_base(j + 1) + v : context_base(order) + (v & (pow4(order) - 1));
}

struct Pred {
  int32_t src, letter;      // the pair (s, a)
  double prob;              // P[s][a]; 0: the slot is not used
};

// table [contexts][PREDS]: the pairs (s, a) that lead to each target, s ascending (a partial predecessor before the full
// ones), a ascending.  The four siblings of a full-length target hold the same sources slot by slot.
inline void build_table(int order, const double* trans, Pred* table) {
  const int NS = contexts(order);
  std::vector<int> used((size_t)NS, 0);
  for (int e = 0; e < NS * PREDS; ++e) table[e] = Pred{0, 0, 0.0};
  for (int s = 0; s < NS; ++s)
    for (int a = 0; a < 4; ++a) {
      const int t = next_context(order, s, a);
      table[t * PREDS + used[(size_t)t]++] = Pred{s, a, trans[4 * s + a]};
    }
}

inline int64_t env_i64(const char* name, int64_t dflt) {
  const char* v = getenv(name);
  return (v && *v) ? atoll(v) : dflt;
}
inline int tile_length(int64_t want) {
  if (want < TILE_MIN) want = TILE_MIN;
  if (want > TILE_MAX) want = TILE_MAX;
  return (int)want;
}

// ---- the plan (host): reaches, groups of rows and buffer sizes; shared by crbm_api.hip and the emulation program ------
struct Plan {
  std::vector<int32_t> reach;     // [R][M + 1]: reach[r][0] = 1, reach[r][M] = G_r
  int64_t gmax = 0;               // the largest G_r: the stride of a context's cells
  int32_t rows_per_group = 0, groups = 0, tile = 0, contexts = 0;
  int64_t state_elems = 0;        // doubles of one state buffer: rows_per_group * contexts * gmax
};

// What crbm_score_distribution refuses, or null with the plan filled.  budget: CRBM_NULL_BYTES; tile: CRBM_NULL_TILE.
inline const char* plan_or_refusal(const int32_t* q, int32_t R, int32_t M, int32_t order, const double* trans, const double* init,
                                   int64_t G, const void* pmf, int64_t budget, int64_t tile, Plan* plan) {
  if (!q || !trans || !init || !pmf) return "null argument";
  if (R < 1) return "R must be at least 1";
  if (M < 1 || M > MAX_M) return "M must lie in [1, 512]";
  if (order < 0 || order > MAX_ORDER) return "order must lie in [0, 3]";
  const int NS = contexts(order);
  for (int s = 0; s < NS; ++s) {
    double sum = 0.0;
    for (int a = 0; a < 4; ++a) {
      const double p = trans[4 * s + a];
      if (!(p >= 0.0) || !std::isfinite(p)) return "a probability is negative or not finite";
      sum += p;
    }
    if (!(std::fabs(sum - 1.0) <= 1e-9)) return "a row of trans does not sum to 1 within 1e-9";
    if (!(init[s] >= 0.0) || !std::isfinite(init[s])) return "a probability is negative or not finite";
  }
  Plan p;
  p.reach.assign((size_t)R * (M + 1), 0);
  for (int64_t r = 0; r < R; ++r) {
    int64_t reach = 1;
    p.reach[(size_t)(r * (M + 1))] = 1;
    for (int j = 0; j < M; ++j) {
      const int32_t* w = q + (r * M + j) * 4;
      int32_t lo = w[0], hi = w[0];
      for (int a = 1; a < 4; ++a) { lo = w[a] < lo ? w[a] : lo; hi = w[a] > hi ? w[a] : hi; }
      if (lo < 0) return "q must not be negative";
      if (lo != 0) return "the smallest q of every position must be 0";
      reach += hi;
      if (reach > MAX_G) return "G must be at least the largest G_r and at most 2^24: use a larger step";
      p.reach[(size_t)(r * (M + 1) + j + 1)] = (int32_t)reach;
    }
    p.gmax = reach > p.gmax ? reach : p.gmax;
  }
  if (G < p.gmax || G > MAX_G) return "G must be at least the largest G_r and at most 2^24: use a larger step";
  if (budget < 1) budget = 1;
  const int64_t per_row = 2 * (int64_t)NS * p.gmax * 8;
  if (per_row > budget) return "the state of one row (2 * contexts * G * 8 bytes) does not fit CRBM_NULL_BYTES: use a larger step";
  int64_t rows = budget / per_row;
  if (rows > R) rows = R;
  if (rows > MAX_GRID_Y / NS) rows = MAX_GRID_Y / NS;
  p.rows_per_group = (int32_t)rows;
  p.groups = (int32_t)((R + rows - 1) / rows);
  p.tile = tile_length(tile);
  p.contexts = NS;
  p.state_elems = rows * NS * p.gmax;
  *plan = std::move(p);
  return nullptr;
}

// ---- kernels ----------------------------------------------------------------------------------------------------------
struct StepArgs {
  const double* src;        // f_j:     [rows][contexts][gmax]
  double* dst;              // f_{j+1}
  const int32_t* q;         // [rows][M][4], the group's rows
  const int32_t* reach;     // [rows][M + 1]
  const Pred* table;        // [contexts][PREDS]
  int64_t gmax;
  int32_t M, j, tile, contexts;
  int32_t ctx0, nctx;       // the target contexts of this launch: [ctx0, ctx0 + nctx)
  int32_t lds_width;        // siblings: cells of a staged source row, tile + the largest halo of the launch
};

// grid (tiles, rows * nctx).  No LDS.
__global__ void __launch_bounds__(256) step_plain_kernel(StepArgs a) {
  const int r = (int)blockIdx.y / a.nctx, t = a.ctx0 + (int)blockIdx.y % a.nctx;
  const int64_t Q0 = (int64_t)blockIdx.x * a.tile;
  const int32_t reach_prev = a.reach[(int64_t)r * (a.M + 1) + a.j], reach_now = a.reach[(int64_t)r * (a.M + 1) + a.j + 1];
  if (Q0 >= reach_now) return;
  const int32_t* w = a.q + ((int64_t)r * a.M + a.j) * 4;
  const Pred* row = a.table + t * PREDS;
  const double* from[PREDS];
  double prob[PREDS];
  int32_t shift[PREDS];
  for (int p = 0; p < PREDS; ++p) {
    prob[p] = row[p].prob;
    shift[p] = w[row[p].letter];
    from[p] = a.src + ((int64_t)r * a.contexts + row[p].src) * a.gmax;
  }
  double* to = a.dst + ((int64_t)r * a.contexts + t) * a.gmax;
  const int64_t Q1 = Q0 + a.tile < reach_now ? Q0 + a.tile : reach_now;
  for (int64_t Q = Q0 + threadIdx.x; Q < Q1; Q += blockDim.x) {
    double acc = 0.0;
    for (int p = 0; p < PREDS; ++p) {
      const int64_t i = Q - shift[p];
      if (prob[p] != 0.0 && i >= 0 && i < reach_prev) acc += prob[p] * from[p][i];
    }
    to[Q] = acc;
  }
}

// grid (tiles, rows * nctx / 4); [ctx0, ctx0 + nctx) are the full-length contexts of an order >= 1.
// LDS: PREDS * lds_width * 8 bytes.
__global__ void __launch_bounds__(256) step_siblings_kernel(StepArgs a) {
  HIP_DYNAMIC_SHARED(double, null_tiles);
  const int families = a.nctx / 4;
  const int r = (int)blockIdx.y / families, t0 = a.ctx0 + 4 * ((int)blockIdx.y % families);
  const int64_t Q0 = (int64_t)blockIdx.x * a.tile;
  const int32_t reach_prev = a.reach[(int64_t)r * (a.M + 1) + a.j], reach_now = a.reach[(int64_t)r * (a.M + 1) + a.j + 1];
  if (Q0 >= reach_now) return;                                  // (the whole block)
  const int32_t* w = a.q + ((int64_t)r * a.M + a.j) * 4;
  int32_t halo = w[0];
  for (int c = 1; c < 4; ++c) halo = w[c] > halo ? w[c] : halo;
  const int n = (int)(Q0 + a.tile < reach_now ? a.tile : reach_now - Q0);
  const int width = n + halo;                                   // cells [Q0 - halo, Q0 + n) of every source
  const Pred* row0 = a.table + t0 * PREDS;
  for (int p = 0; p < PREDS; ++p) {
    const double* from = a.src + ((int64_t)r * a.contexts + row0[p].src) * a.gmax;
    for (int e = (int)threadIdx.x; e < width; e += (int)blockDim.x) {
      const int64_t i = Q0 - halo + e;
      null_tiles[p * a.lds_width + e] = (i >= 0 && i < reach_prev) ? from[i] : 0.0;
    }
  }
  __syncthreads();
  for (int c = 0; c < 4; ++c) {
    const Pred* row = a.table + (t0 + c) * PREDS;
    double prob[PREDS];
    for (int p = 0; p < PREDS; ++p) prob[p] = row[p].prob;
    const int back = halo - w[c];                               // (every slot of target c carries the letter c)
    double* to = a.dst + ((int64_t)r * a.contexts + t0 + c) * a.gmax + Q0;
    for (int e = (int)threadIdx.x; e < n; e += (int)blockDim.x) {
      double acc = 0.0;
      for (int p = 0; p < PREDS; ++p)
        if (prob[p] != 0.0) acc += prob[p] * null_tiles[p * a.lds_width + e + back];
      to[e] = acc;
    }
  }
}

struct EdgeArgs {
  double* state;            // [rows][contexts][gmax]
  const double* init;       // [contexts]
  double* pmf;              // [rows][G]
  const int32_t* reach;     // [rows][M + 1]
  int64_t gmax, G;
  int32_t M, tile, contexts, rows;
};

// f_0: cell 0 of every context.  grid: rows * contexts lanes.
__global__ void __launch_bounds__(256) start_kernel(EdgeArgs a) {
  const int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (e < (int64_t)a.rows * a.contexts) a.state[e * a.gmax] = a.init[e % a.contexts];
}

// pmf[r][Q] = sum_s f_M[r][s][Q] in index order below G_r, 0 from there to G.  grid (tiles of G, rows).
__global__ void __launch_bounds__(256) marginal_kernel(EdgeArgs a) {
  const int r = (int)blockIdx.y;
  const int32_t Gr = a.reach[(int64_t)r * (a.M + 1) + a.M];
  const int64_t Q0 = (int64_t)blockIdx.x * a.tile, Q1 = Q0 + a.tile < a.G ? Q0 + a.tile : a.G;
  const double* f = a.state + (int64_t)r * a.contexts * a.gmax;
  for (int64_t Q = Q0 + threadIdx.x; Q < Q1; Q += blockDim.x) {
    double acc = 0.0;
    if (Q < Gr)
      for (int s = 0; s < a.contexts; ++s) acc += f[(int64_t)s * a.gmax + Q];
    a.pmf[(int64_t)r * a.G + Q] = acc;
  }
}

// ---- the launches of one position for the rows [row0, row0 + rows) of a group (host) -----------------------------------
struct Launch {
  int siblings;             // 0: step_plain_kernel, 1: step_siblings_kernel
  unsigned gx, gy, block;
  size_t lds;
  int32_t ctx0, nctx, lds_width;
};
inline unsigned block_for(int tile) { return tile >= 256 ? 256u : (unsigned)((tile + 63) / 64 * 64); }

// fills out[0 .. n), n <= 2, and returns n
inline int step_launches(const Plan& p, const int32_t* q, int M, int order, int variant, int row0, int rows, int j, Launch* out) {
  int64_t reach = 1;
  int32_t halo = 0;
  for (int r = row0; r < row0 + rows; ++r) {
    const int64_t now = p.reach[(size_t)r * (M + 1) + j + 1];
    reach = now > reach ? now : reach;
    for (int a = 0; a < 4; ++a) {
      const int32_t v = q[((int64_t)r * M + j) * 4 + a];
      halo = v > halo ? v : halo;
    }
  }
  const unsigned tiles = (unsigned)((reach + p.tile - 1) / p.tile), block = block_for(p.tile);
  const int NS = p.contexts, full0 = context_base(order), nfull = pow4(order);
  const int64_t lds = (int64_t)PREDS * (p.tile + (int64_t)halo) * 8;
  if (variant != 1 || order < 1 || lds > LDS_BYTES) {
    out[0] = Launch{0, tiles, (unsigned)(rows * NS), block, 0, 0, NS, 0};
    return 1;
  }
  out[0] = Launch{0, tiles, (unsigned)(rows * full0), block, 0, 0, full0, 0};                   // the partial targets
  out[1] = Launch{1, tiles, (unsigned)(rows * (nfull / 4)), block, (size_t)lds, full0, nfull, p.tile + halo};
  return 2;
}

}  // namespace null
}  // namespace crbm
