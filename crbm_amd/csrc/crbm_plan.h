// The launch plan of a model (crbm_api.hip), host only: which kernels a model takes (specialised or generic, slabbed or
// not), the geometry of every chain launch and what the specialised kernels are compiled with.  plan_launches is the one
// place that derives it: crbm_precompile compiles for the plan, crbm_create loads and launches by it, so the code object a
// handle asks for is the one the build left in the cache (the JIT cache key hashes G, GS, gibbs_wpe, gibbs_tb and the slab
// model).  No HIP types: the tests call it on the CPU (tests/emu/plan_driver.cpp).
#pragma once

#include "crbm_layout.h"

#include <algorithm>
#include <cmath>
#include <cstdlib>

namespace crbm {

inline int env_int(const char* name, int dflt) {
  const char* v = getenv(name);
  return (v && *v) ? atoi(v) : dflt;
}

// Letter grouping of PLAIN chain launches (crbm_gibbs_steps*: one 1024-thread block per CU whose LDS is otherwise idle):
// the largest grouping whose table stays within 48 KB -- config #2: G = 4 (49 152 B, four gathers per position) where the
// fused training launch, four blocks per CU beside the statistics slices, takes G = 3 (five gathers): 21.7 -> 21.4 us per
// launch.  Only for models whose training step never launches the plain kernel (Cfg::FUSE_STATS) -- the others would
// rebuild the second table every step -- and not beyond 48 KB: every block copies its table once per launch (config #5
// with G = 4, 82 KB: 144.6 -> 150 us).  CRBM_GROUP_SOLO overrides.
inline int solo_group(int K, int M, int ds, int G, int pool) {
  const int forced = env_int("CRBM_GROUP_SOLO", 0);
  if (forced >= 1 && forced <= 4) return forced;
  if (!model_shape(K, M, ds, G, pool).FUSE_STATS) return G;
  return std::max(G, choose_group(K, M, ds, 48 * 1024));
}

// Gibbs launch geometry.  A thread owns 4 consecutive positions, a block owns
// tiles of S whole chains (grid-stride).  Pick (S, threads) that keeps lanes
// busy in both phases and splits the tiles evenly over the CUs.
struct GibbsGeom {
  int S, threads, grid, lds;
};

// solo: geometry of launches that only advance the chains (crbm_gibbs_steps*, the chain launch of models
// whose statistics run in kernels of their own): free of the 256-thread build of the fused variants.
inline GibbsGeom choose_gibbs_geometry(const ModelShape& ms, int Lf, int B, int num_cu, bool sparse, bool solo = false) {
  const int forceS = env_int("CRBM_GIBBS_S", 0), forceT = env_int("CRBM_GIBBS_THREADS", 0);
  GibbsGeom best{1, 256, 1, 0};
  double best_score = -1.0;
  // 256 first: larger blocks (one table copy shared by up to 16 waves; the chain kernels are then compiled
  // with that launch bound) win only where they score strictly better -- models whose tables leave room
  // for fewer than four 256-thread blocks per CU.  The fused statistics variants are built for 256.
  double best_occupancy = 0.0;
  for (int threads : {256, 128, 64, 512, 1024}) {
    // measured: config #4 (two 256-thread blocks per CU) 2.62 -> 2.26 ms per launch with one 1024-thread
    // block; config #5 (three blocks per CU) is no faster with two 512-thread blocks -- so only when the
    // small blocks reach at most half the waves
    // Solo launches of single-stranded models take the large blocks whenever they score better (config #2:
    // one 1024-thread block of 32 chains per CU 22.7 us per launch against 23.8 with four 256-thread blocks:
    // one table copy per CU, and the short last round of the v|h pass spreads over all SIMDs).  Double-stranded
    // models too since they gather from one table and their queue of undecided units holds 254 entries
    // (config #5: 158 us per launch with three 256-thread blocks of 3 chains per CU, 145 with two 512-thread
    // blocks of 8, 143.6 with one 1024-thread block of 16 -- 147 when the queue overflows at 62 entries).
    const bool big_ok = solo ? true : (!ms.FUSE_STATS && best_occupancy <= 0.5);
    // (experiment: CRBM_FUSED_THREADS=512 with CRBM_JIT_DEFINES=-DCRBM_FUSED_TB=512 gives the fused training launch larger blocks)
    const int fusedT = (!solo && ms.FUSE_STATS) ? env_int("CRBM_FUSED_THREADS", 0) : 0;
    if (fusedT > 0 && threads != fusedT) continue;
    if (fusedT == 0 && threads > 256 && (!big_ok || env_int("CRBM_GIBBS_MAX_THREADS", 1024) < threads)) continue;
    if (forceT > 0 && threads != forceT) continue;
    for (int S = 1; S <= std::min(B, 64); ++S) {
      if (forceS > 0 && S != forceS) continue;
      const GibbsLayout gl = gibbs_layout(ms, Lf, S, sparse);
      if (gl.lds_bytes > 150 * 1024 && !(forceS > 0)) continue;
      if (gl.lds_bytes > 160 * 1024 || (long)S * gl.Lrow * ms.NW >= (1 << 20)) continue;
      // lanes are used at wave granularity (an idle wave of a pass costs nothing);
      // 4 hidden positions cost ~1.5x a 4-position visible block
      const double iv = (double)S * gl.nvb, ih = (double)S * gl.nhb;
      const double util = (iv + 0.375 * ih) / (64.0 * (std::ceil(iv / 64.0) + 0.375 * std::ceil(ih / 64.0)));
      const double ntiles = std::ceil((double)B / S);
      const double per_cu_tiles = ntiles / num_cu;
      const double balance = per_cu_tiles / std::ceil(per_cu_tiles);
      const int blocks_cu = std::max(1, std::min((160 * 1024) / gl.lds_bytes, 1024 / threads));   // <= 16 waves / CU
      const double waves_cu = std::min(per_cu_tiles, (double)blocks_cu) * std::min((double)threads, iv) / 64.0;
      const double occupancy = std::min(1.0, waves_cu / 16.0);                // 4 waves / SIMD hide the LDS latency
      const double score = util * balance * (0.4 + 0.6 * occupancy) - 1e-4 * S;
      if (score > best_score) {
        best_score = score;
        best = GibbsGeom{S, threads, (int)std::min(ntiles, (double)num_cu * blocks_cu), gl.lds_bytes};
        if (threads <= 256) best_occupancy = occupancy;
      }
    }
  }
  const int forceG = env_int("CRBM_GIBBS_GRID", 0);
  if (forceG > 0) best.grid = forceG;
  return best;
}

// Partitions of a plain chain launch (LaunchPlan::chain_parts).  Worth it where a launch is short and its blocks are
// small: the partitions' kernels then share every CU (several blocks of each resident at once) and one partition's
// drain / dispatch / ramp is filled by the other's work.  Measured (two handles of half the chains, alternating launches):
// config #2 with 256-thread blocks of 8 chains 21.7 -> 17.6 us per step of the whole batch (17.4 with four partitions);
// with one 1024-thread block per CU per partition nothing (20.5 vs 20.6): the partitions then own disjoint CUs.
// In the library: config #2 20.3 -> 17.8 us, config #5 137.9 -> 136.1 us, config #4 2191 -> 2180 us (not worth a second
// geometry there); more partitions do not help (config #2: three 17.8 us against 17.4 with two, four 28 us: a process has
// four hardware queues, and partitions that share one serialise).
// Auto: two partitions when the small-block geometry of half the batch puts at least two blocks on a CU, still covers
// every CU, and a launch is short (by the number of hidden units per step); CRBM_CHAIN_PARTS forces 1..4.
struct PartPlan {
  int parts, part_chains;
  GibbsGeom geom;      // of one partition
};
inline PartPlan plan_chain_parts(const ModelShape& ms, int Lf, int B, int num_cu) {
  PartPlan one{1, B, GibbsGeom{0, 0, 0, 0}};
  const int forced = env_int("CRBM_CHAIN_PARTS", 0);
  if (forced == 1 || B < 2) return one;
  const int parts = forced >= 2 ? std::min(forced, 4) : 2;
  // small blocks: the geometry the fused training launch uses (at most 256 threads unless they reach half the waves)
  const int half = (B + parts - 1) / parts;
  GibbsGeom g = choose_gibbs_geometry(ms, Lf, half, num_cu, true, false);
  if (g.lds <= 0) return one;
  const int tiles = (B + g.S - 1) / g.S, tiles_part = (tiles + parts - 1) / parts;
  const int blocks_cu = std::max(1, std::min((160 * 1024) / g.lds, 1024 / g.threads));
  if (forced < 2) {
    const double items = (double)B * Lf * ms.K * (1 + ms.DS);          // hidden units per step
    if (blocks_cu < 2 || tiles_part < num_cu || items > 256e6) return one;
  }
  if (tiles_part < 1) return one;
  PartPlan p{parts, tiles_part * g.S, g};
  p.geom.grid = std::min(tiles_part, num_cu * blocks_cu);
  // (Measured and NOT adopted: twice the chains per tile where the partition's tiles do not divide over its resident blocks
  //  -- config #5: 2048 tiles of 2 chains on 768 blocks.  Forced for every kernel of the handle, CRBM_GIBBS_S=4, it runs
  //  128.6 instead of 135.2 us per step; chosen here for the partitioned launch alone 150.7: the kernel is compiled with the
  //  occupancy hint of the handle's regular geometry, three blocks per CU, and the larger tiles leave two.)
  return p;
}

// Does the model need the generic ("big") kernels?  Beyond 256 motifs or 64 letters the specialised templates do not
// exist; within them the LDS decides: the chain kernel holds its tables and at least one chain, the statistics kernel a
// column image per 16 motifs beside the gather table (at most 16 roles of 64 threads).  CRBM_FORCE_BIG=1 puts any
// model on the generic path -- the tests compare the two paths on the same model with it.
inline bool model_needs_big(const ModelShape& ms, int Lf, int B, int num_cu) {
  if (env_int("CRBM_FORCE_BIG", 0)) return true;
  if (ms.K > MAX_MOTIFS || ms.M > MAX_MOTIF_LENGTH) return true;
  if (choose_gibbs_geometry(ms, Lf, B, num_cu, true).lds <= 0) return true;
  for (int want_sp = 0; want_sp <= 1; ++want_sp) {
    const int tabs = ms.TAB * 4;
    const StatsMfmaLayout st = stats_mfma_layout(ms, want_sp, Lf, 0, tabs, true);
    if (st.threads > 1024 || std::max(st.region_floats * 4 + tabs, st.combine_bytes) > 160 * 1024) return true;
  }
  return false;
}

// ---- geometry of the generic ("big") kernels (crbm_kernels_generic.h), all launched with 256-thread blocks -----------------
// The one place the host derives it: crbm_api.hip launches by these, tests/test_generic_geom_host.py reads them on the CPU
// (tests/emu/plan_driver.cpp) and holds every GPU case of tests/test_gpu_generic_geometry.py to the regime it is named for.
constexpr int BIG_THREADS = 256;
constexpr size_t BIG_LDS_MAX = 160 * 1024;

// h | v (big_hgv_kernel, big_hgv_pooled_kernel) of n rows of L letters in LW words, masks of NW words
struct BigHgvGeom { int KS, TS, split; size_t lds; };
inline BigHgvGeom big_hgv_geom(int A, int M, int pool, int n, int L, int LW, int NW, int num_cu) {
  BigHgvGeom g;
  const int Lh = L - M + 1;
  int ks = pool > 1 ? 8 : 32;                                // motifs per staged slab: a divisor of 32 whose filters fit 96 KB
  while (ks > 1 && (size_t)big_hgv_ksp(ks) * M * A * 4 > 96 * 1024) ks >>= 1;   // (pooled: at most 8, the capacity of big_hgv_pooled_kernel)
  g.KS = ks;
  // rows per tile: enough tiles to cover the chip a few times over (every tile stages the filters once per slab), at most
  // what the LDS takes of packed letters and ~4096 positions
  g.TS = std::max(1, std::min(std::min((n + 4 * num_cu - 1) / (4 * num_cu), (32 * 1024) / (LW * 4)), std::max(1, 4096 / Lh)));
  g.lds = ((size_t)big_hgv_ksp(ks) * M * A + 32) * 4 + (size_t)g.TS * LW * 4;
  const int ntiles = (n + g.TS - 1) / g.TS;
  // few tiles (small batches): one block per (tile, mask word) -- every slab lies inside one mask word, so blocks of
  // different words never touch the same output
  g.split = (NW > 1 && ntiles < 4 * num_cu) ? 1 : 0;
  return g;
}

// v | h of the chain (big_vgh_kernel for DNA, big_vgh_any_kernel): filter columns per staged slab, positions per chunk
struct BigVghGeom { int JS, CH; size_t lds; };
// (threads, JS: the CPU program tests/emu/big_vgh_main.cpp runs the kernels with 64-thread blocks and narrower slabs)
inline BigVghGeom big_vgh_geom(int A, int M, int Lv, int threads = BIG_THREADS, int JS = 0) {
  BigVghGeom g;
  g.JS = JS > 0 ? JS : std::max(1, std::min(M, (64 * 1024) / (32 * 4 * A)));
  g.CH = A == 4 ? BIG_VR * threads : threads;
  // DNA: activations in registers; any other alphabet: one position per thread, activations in LDS (big_vgh_any_kernel)
  g.lds = A == 4 ? (size_t)g.JS * 32 * 16 + (size_t)g.CH + (size_t)2 * (std::min(g.CH, Lv) + M - 1) * 4   // (+ one mask word of both strands for a chunk)
                 : ((size_t)g.JS * 32 * A + (size_t)A * threads) * 4 + threads;
  return g;
}

// statistics (big_stats_kernel, grid K x R): rows a block strides by, hidden positions per chunk
struct BigStatsGeom { int R, CH; size_t lds; };
inline BigStatsGeom big_stats_geom(int A, int M, int K, int n, int Lh, int pool, int num_cu) {
  BigStatsGeom g;
  g.R = std::max(1, std::min(n, std::max(1, (num_cu * 8) / K)));
  g.CH = std::max(64, std::min(4096, Lh));
  g.CH = std::max(pool, g.CH - g.CH % pool);                // chunks start on pooling-group boundaries
  g.lds = (((size_t)A * M + 3) & ~(size_t)3) * 4 + (size_t)(pool > 1 ? 5 : 3) * g.CH * 4 + 64 + 12 * BIG_THREADS * 4 +
          (size_t)((A + 3) & ~3) * 4 + (size_t)g.CH + M;
  return g;
}

// free energies and hit summaries (big_eval_kernel): the filter of one motif and the letters of a row as bytes
inline size_t big_eval_lds(int A, int M, int L) { return (((size_t)A * M + 3) & ~(size_t)3) * 4 + 64 + (size_t)L; }

// dense v | h (crbm_v_given_h): DNA stages a slab of motifs (vgh_dense_kernel), any other alphabet keeps a position's
// activations of all letters in LDS (vgh_dense_any_kernel)
inline size_t vgh_dense_lds(int A, int K, int M) {
  return A == 4 ? (size_t)vgh_dense_ks(K, M) * M * 16 : (size_t)A * BIG_THREADS * 4;
}

// block-size bound the chain kernels are compiled with
inline int gibbs_block_bound(int threads) { return threads > 512 ? 1024 : threads > 256 ? 512 : 256; }

// waves per SIMD the sparse Gibbs variant reaches with its geometry; 0 when >= 4 (no hint needed)
inline int gibbs_wpe_hint(const GibbsGeom& g) {
  if (g.lds <= 0) return 0;
  const int blocks_cu = std::max(1, std::min((160 * 1024) / g.lds, 2048 / g.threads));
  const int wpe = std::max(1, blocks_cu * (g.threads / 64) / 4);
  return wpe < 4 ? wpe : 0;
}

// The slab model of a generic DNA model: up to `want` motifs are one slab, a larger model takes slabs of a multiple of ten
// motifs (the sampler's groups); the largest candidate whose statistics kernel fits the LDS.  Returns 0 motifs when none does.
inline int slab_choose(int K, int M, int ds, int pool, int Lf, int* G_out, ModelShape* ms_out) {
  const int want = std::max(10, std::min(env_int("CRBM_SLAB_MOTIFS", 60), 64));      // (the slab kernels are compiled for models of up to 64 motifs: crbm_jit.h)
  const int first = K <= want ? K : want / 10 * 10;
  for (int cand : {first, 40, 30, 20, 10}) {
    if (cand > K || (cand != first && cand >= first)) continue;
    int G = env_int("CRBM_SLAB_GROUP", 0);
    if (G < 1 || G > 4) {
      // the table budget of the specialised kernels; long motifs that it leaves with single letters take pairs where those fit
      // twice 48 KB (60 x 40 double-stranded: 77 KB, training step 1.55 -> 1.19 ms at 2048 chains; a larger budget for ALL slabs
      // costs the statistics kernel waves: 256 x 4 double-stranded 1.72 -> 1.99 ms)
      const int budget = env_int("CRBM_SLAB_TABLE_BUDGET", 26 * 1024);
      G = choose_group(cand, M, ds, budget);
      if (G == 1) G = choose_group(cand, M, ds, std::max(budget, 48 * 1024));
    }
    const ModelShape ms = model_shape(cand, M, ds, G, pool);
    bool fit = true;
    for (int want_sp = 0; want_sp <= 1 && fit; ++want_sp) {
      const int tabs = ms.TAB * 4;
      const StatsMfmaLayout st = stats_mfma_layout(ms, want_sp, Lf, 0, tabs, true);
      if (st.threads > 1024 || std::max(st.region_floats * 4 + tabs, st.combine_bytes) > 160 * 1024) fit = false;
    }
    if (fit) { *G_out = G; *ms_out = ms; return cand; }
  }
  return 0;
}

// the geometry of one kind of chain launch; off (threads == 0) where the model has no launch of that kind
struct ChainGeom { GibbsLayout gl = {}; int threads = 0, grid = 0; bool on() const { return threads > 0; } };

// A chain launch shape whose kernels are compiled for exactly this geometry (crbm_kernels.h, GeomCT; crbm_jit.h,
// jit_geo_stub): the layout, the block, the grid and the number of chains of ONE launch, all tiles full.  A launch of any
// other shape (a ragged last partition, a launch without steps, profiling aids) takes the run-time form of the model's
// own module.  group: letters per gather-table group of the kernel's Cfg.
struct GeoSpec {
  GibbsLayout gl = {};
  int threads = 0, grid = 0, nchains = 0, group = 0;
  bool aligned = false;         // every tile's state starts and ends on a 16-byte boundary
  bool on() const { return threads > 0; }
  bool serves(const GibbsLayout& l, int threads_, int grid_, int nchains_) const {
    return on() && l.S == gl.S && l.Lv == gl.Lv && l.nvb == gl.nvb && l.nhb == gl.nhb && l.Lrow == gl.Lrow && l.LWs == gl.LWs &&
           threads_ == threads && grid_ == grid && nchains_ == nchains;
  }
};
inline GeoSpec geo_spec(const GibbsLayout& gl, int threads, int grid, int nchains, int NW, int group) {
  GeoSpec s;
  if (threads <= 0 || threads % 64 || gl.S < 1 || nchains < gl.S || nchains % gl.S || grid < 1 || grid > nchains / gl.S) return s;
  s.gl = gl; s.threads = threads; s.grid = grid; s.nchains = nchains; s.group = group;
  s.aligned = ((long)gl.S * gl.nhb * NW) % 4 == 0;
  return s;
}

struct LaunchPlan {
  bool big = false;             // model beyond the LDS-resident kernels: the generic "big" kernels serve every entry point
  int G = 0, GS = 0;            // letters per gather-table group: of the model, of plain chain launches (solo_group)
  ModelShape ms = {}, ms_solo = {};   // ... and the model in the two groupings (ms_solo == ms when GS == G)
  // top-down variants of the Gibbs kernel: [0] dense tables (small models only: has_dense), [1] set-bit walk
  bool has_dense = false;
  ChainGeom chain[2];
  ChainGeom solo;               // unpartitioned plain chain launches of the set-bit walk, where they differ from chain[1]
  // Plain chain launches of short kernels go out as `chain_parts` launches of `part_chains` chains each, one stream per
  // partition: chains are independent, so partition p's step t+1 only waits for partition p's step t, and the drain of
  // one partition's kernel, the dispatch and the ramp of its next one are filled by the other partition's blocks on the
  // same CUs (config #2: 20.9 -> 17.6 us per step of the whole batch).  (What a one-step launch still costs beyond its
  // step after that is not idle time: the counters show the vector issue busy for 0.92 of a step, i.e. instructions of
  // the launch's fixed path -- which geo_plain / geo_fused below remove, not overlap.)  `part` is the geometry of ONE partition's launch
  // (chain_parts > 1); solo / chain[1] stay the unpartitioned one, which the chain launch INSIDE a training step takes
  // (one launch, then the statistics wait for it).
  ChainGeom part;
  int chain_parts = 1, part_chains = 0;
  // what jit_compile / jit_load are keyed by: the register-allocation hint compiled into the sparse Gibbs kernel and
  // the block-size bound of the chain kernels (of the largest block any geometry above launches)
  int gibbs_wpe = 0, gibbs_tb = 256;
  // Launch shapes with geometry-specialised chain kernels, a second code object keyed by them: of the plain launches
  // of the API (one partition's where they go out in partitions) and of the chain half of the fused training launch
  // (chain[1] with statistics).  CRBM_GEOM: 0 none (every launch in the run-time form), 1 (default) handles whose
  // launch puts a tile on every CU -- below that a launch is over before its fixed path matters, and a handle of a few
  // chains should not pay a second compile --, 2 every handle.
  // Two shapes, not one per ChainGeom: where the plain launches go out in partitions (chain_parts > 1), an UNPARTITIONED
  // plain launch of that handle (solo / chain[1]: crbm_gibbs_steps on another stream, the chain launch inside a
  // training step of a model without fused statistics) is never specialised and takes the run-time form -- a third
  // instantiation of the body would lengthen every crbm_create of such a handle for launches the hot paths do not make.
  GeoSpec geo_plain, geo_fused;
  // the slab model of a generic DNA model (slab_choose); slab_K == 0: no slabs, slab_note says why
  int slab_K = 0, slab_G = 0;
  ModelShape slab_ms = {};
  const char* slab_note = nullptr;
  // crbm_create refuses the model with this message (a variant of the chain kernel has no geometry that fits the LDS).
  // The plan of a refused model is not to be launched by: that variant's ChainGeom is off, the rest is planned as if it
  // were not there (crbm_precompile, which never refused, still finds what to compile for).
  const char* refusal = nullptr;
};

// The geometry of a chain launch that only advances the chains, with top-down variant `variant` (0 dense, 1 set-bit
// walk): one partition's where such launches go out in partitions (`parts`: the plain launches of the API), else the
// solo one where the model has it, else the variant's own.
inline const ChainGeom& plain_geom(const LaunchPlan& p, int variant, bool parts = true) {
  if (variant == 1 && parts && p.chain_parts > 1) return p.part;
  if (variant == 1 && p.solo.on()) return p.solo;
  return p.chain[variant];
}

inline LaunchPlan plan_launches(int K, int M, int ds, int A, int pool, int Lf, int B, int num_cu) {
  LaunchPlan p;
  p.G = env_int("CRBM_GROUP", 0);
  if (p.G < 1 || p.G > 4) p.G = choose_group(K, M, ds, env_int("CRBM_TABLE_BUDGET", 26 * 1024));
  p.ms = model_shape(K, M, ds, p.G, pool);
  p.GS = p.G; p.ms_solo = p.ms;
  p.part_chains = B;
  // (the specialised kernels are DNA kernels: 2-bit letters, tables over letter tuples; any other alphabet is generic)
  p.big = (K > MAX_MOTIFS || M > MAX_MOTIF_LENGTH || A != 4) ? true : model_needs_big(p.ms, Lf, B, num_cu);
  if (p.big) {
    // the generic kernels are compiled ahead of time; a DNA model with motifs of up to 64 letters also takes the
    // specialised kernels of its slab model.  CRBM_SLAB_STATS=0 switches the slabs off (A/B runs, tests).
    // (read here with the rest of the plan: in crbm_create that is before any kernel is loaded, not where the slab model is set up)
    if (env_int("CRBM_SLAB_STATS", 1) == 0) p.slab_note = "CRBM_SLAB_STATS=0";
    else if (A != 4 || M > MAX_MOTIF_LENGTH) p.slab_note = "other alphabet, or motifs beyond 64 letters";
    else {
      p.slab_K = slab_choose(K, M, ds, pool, Lf, &p.slab_G, &p.slab_ms);
      if (!p.slab_K) p.slab_note = "no slab of this motif length fits the LDS";
    }
    return p;
  }
  p.has_dense = p.ms.DENSE != 0;
  for (int v = p.has_dense ? 0 : 1; v < 2; ++v) {
    const GibbsGeom geom = choose_gibbs_geometry(p.ms, Lf, B, num_cu, v == 1);
    if (geom.lds <= 0) { p.refusal = "model too large for the LDS-resident Gibbs kernel"; continue; }
    p.chain[v] = ChainGeom{gibbs_layout(p.ms, Lf, geom.S, v == 1), geom.threads, geom.grid};
    if (v == 1) p.gibbs_wpe = gibbs_wpe_hint(geom);
  }
  // plain chain launches: their own geometry; short launches in partitions on streams of their own (chain_parts);
  // unpartitioned ones of small fused models with their own letter grouping (solo_group)
  const PartPlan parts = plan_chain_parts(p.ms, Lf, B, num_cu);
  p.chain_parts = parts.parts;
  if (parts.parts > 1) {
    p.part_chains = parts.part_chains;
    p.part = ChainGeom{gibbs_layout(p.ms, Lf, parts.geom.S, true), parts.geom.threads, parts.geom.grid};
  }
  // the unpartitioned launch: its own geometry and, where nothing else launches that kernel, its own letter grouping
  p.GS = parts.parts > 1 ? p.G : solo_group(K, M, ds, p.G, pool);
  p.ms_solo = model_shape(K, M, ds, p.GS, pool);
  GibbsGeom solo = choose_gibbs_geometry(p.ms_solo, Lf, B, num_cu, true, true);
  if (solo.lds <= 0 && p.GS != p.G) {           // the larger table leaves no room for a chain: the model's grouping
    p.GS = p.G; p.ms_solo = p.ms;
    solo = choose_gibbs_geometry(p.ms_solo, Lf, B, num_cu, true, true);
  }
  if (solo.lds > 0 && (p.GS != p.G || solo.threads != p.chain[1].threads || solo.S != p.chain[1].gl.S || solo.grid != p.chain[1].grid))
    p.solo = ChainGeom{gibbs_layout(p.ms_solo, Lf, solo.S, true), solo.threads, solo.grid};
  int threads = 0;
  for (const ChainGeom* g : {&p.chain[0], &p.chain[1], &p.solo, &p.part}) threads = std::max(threads, g->threads);
  p.gibbs_tb = gibbs_block_bound(threads);
  const int geo_mode = env_int("CRBM_GEOM", 1);
  if (geo_mode > 0 && !p.refusal) {
    auto spec = [&](const ChainGeom& g, int nchains, int group) {
      GeoSpec s = g.on() ? geo_spec(g.gl, g.threads, g.grid, nchains, p.ms.NW, group) : GeoSpec();
      if (geo_mode == 1 && s.on() && nchains / s.gl.S < num_cu) s = GeoSpec();
      return s;
    };
    p.geo_plain = p.chain_parts > 1 ? spec(p.part, p.part_chains, p.G) : spec(plain_geom(p, 1, false), B, p.GS);
    if (p.ms.FUSE_STATS) p.geo_fused = spec(p.chain[1], B, p.G);
  }
  return p;
}

}  // namespace crbm
