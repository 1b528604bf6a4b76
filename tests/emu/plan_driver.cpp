// plan_launches (crbm_amd/csrc/crbm_plan.h) as plain ints, for tests/test_plan_host.py.
//   plan_ints:        the plan: PLAN_HEAD ints (big, G, GS, has_dense, chain_parts, part_chains, gibbs_wpe, gibbs_tb, slab_K,
//                     slab_G, refused, NW), then GEOM_INTS ints for each of chain[0], chain[1], solo, part (threads, grid, S,
//                     Lrow, lds_bytes, and whether gl is gibbs_layout of the geometry's model shape, Lf and S).  Returns the count.
//   plan_launch_info: what crbm_get_launch_info reports of a handle with that plan (grid, block, chains per tile, LDS bytes,
//                     table group, chain_parts, gibbs_sparse); `dense`: the handle was created under CRBM_TOPDOWN=dense.
//                     A MIRROR of crbm_get_launch_info and of crbm_create's choice of the variant (crbm_api.hip), which need a
//                     GPU: it must follow them (tests/test_gpu_sweeps.py, test_launch_info_is_the_recorded_plan, checks the
//                     real function against the same fixture); the geometry itself comes from the shared plain_geom.
//   plan_block_bound: gibbs_block_bound.
//   big_geom_ints:    the geometry of the generic kernels for tests/test_generic_geom_host.py, BIG_GEOM_INTS ints: h|v (KS, TS,
//                     split, lds) of n rows of L letters, chain v|h (JS, CH, lds) of chains of Lf hidden positions, statistics
//                     (R, CH, lds) of the n rows, the LDS of the evaluation kernel and of the dense v|h pass (slab of
//                     vgh_dense_ks motifs), and LW, NW.
#include "crbm_plan.h"

#include <cstring>

using namespace crbm;

extern "C" int plan_ints(int K, int M, int ds, int A, int pool, int Lf, int B, int num_cu, int* out) {
  const LaunchPlan p = plan_launches(K, M, ds, A, pool, Lf, B, num_cu);
  int n = 0;
  for (int v : {(int)p.big, p.G, p.GS, (int)p.has_dense, p.chain_parts, p.part_chains, p.gibbs_wpe, p.gibbs_tb, p.slab_K, p.slab_G,
                p.refusal ? 1 : 0, p.ms.NW})
    out[n++] = v;
  const ChainGeom* geoms[4] = {&p.chain[0], &p.chain[1], &p.solo, &p.part};
  for (int i = 0; i < 4; ++i) {
    const ChainGeom& g = *geoms[i];
    int same = 0;
    if (g.on()) {
      const GibbsLayout want = gibbs_layout(i == 2 ? p.ms_solo : p.ms, Lf, g.gl.S, i != 0);
      same = want.S == g.gl.S && want.Lv == g.gl.Lv && want.nvb == g.gl.nvb && want.nhb == g.gl.nhb && want.Lrow == g.gl.Lrow &&
             want.LWs == g.gl.LWs && want.lds_bytes == g.gl.lds_bytes;
    }
    for (int v : {g.threads, g.grid, g.gl.S, g.gl.Lrow, g.gl.lds_bytes, same}) out[n++] = v;
  }
  return n;
}

extern "C" void plan_launch_info(int K, int M, int ds, int A, int pool, int Lf, int B, int num_cu, int dense, int* out) {
  const LaunchPlan p = plan_launches(K, M, ds, A, pool, Lf, B, num_cu);
  if (p.big) {
    const int generic[7] = {0, 256, 0, 0, 0, 1, 1};
    memcpy(out, generic, sizeof(generic));
    return;
  }
  const int variant = (dense && p.has_dense) ? 0 : 1;
  const ChainGeom& g = plain_geom(p, variant);
  const int info[7] = {g.grid, g.threads, g.gl.S, g.gl.lds_bytes, p.GS, variant == 1 ? p.chain_parts : 1, variant};
  memcpy(out, info, sizeof(info));
}

extern "C" int plan_block_bound(int threads) { return gibbs_block_bound(threads); }

extern "C" int big_geom_ints(int K, int M, int A, int pool, int n, int L, int Lf, int num_cu, long* out) {
  const int LW = letter_words_any(A, L), NW = (K + 31) / 32, Lh = L - M + 1;
  const BigHgvGeom h = big_hgv_geom(A, M, pool, n, L, LW, NW, num_cu);
  const BigVghGeom v = big_vgh_geom(A, M, Lf + M - 1);
  const BigStatsGeom s = big_stats_geom(A, M, K, n, Lh, pool, num_cu);
  int i = 0;
  for (long x : {(long)h.KS, (long)h.TS, (long)h.split, (long)h.lds, (long)v.JS, (long)v.CH, (long)v.lds, (long)s.R, (long)s.CH, (long)s.lds,
                 (long)big_eval_lds(A, M, L), (long)vgh_dense_lds(A, K, M), (long)(A == 4 ? vgh_dense_ks(K, M) : K), (long)LW, (long)NW})
    out[i++] = x;
  return i;
}
