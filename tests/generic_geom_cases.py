"""The shapes of tests/test_gpu_generic_geometry.py and the regime of the generic kernels' geometry each one is named for.
A plain module, shared by that GPU suite and by tests/test_generic_geom_host.py, which holds every case to its regime on
the CPU (crbm_plan.h through tests/emu/plan_driver.cpp, at the 256 compute units of the MI355X).

A case: model (A letters, K motifs of M letters, ds, pooling), data (n rows of L letters), chains (B chains of Lf hidden
positions) and `regime`, the expected values of
  KS           motifs per staged slab of the h|v kernel                      (big_hgv_geom)
  split        one block per (tile, mask word)                               (big_hgv_geom)
  hgv_fits     the h|v launch of the data rows fits the LDS (False: refused) (big_hgv_geom)
  col_slabs    ceil(M / JS): column slabs of the chain v|h filter            (big_vgh_geom)
  vgh_chunks   ceil(Lv / CH): position chunks of the chain v|h               (big_vgh_geom)
  stats_chunks chunks of the statistics kernel over the data rows            (big_stats_geom)
  R            row stride of the statistics kernel                          (big_stats_geom)
  slots        (letter, column) accumulators per thread of the statistics kernel: ceil(A M / 256)
  slab_n       slabs of the slab model (0: the model is off the slab route)  (plan_launches)
  dense_slabs  ceil(K / KS) of the dense v|h pass                            (vgh_dense_ks)
Keys a case does not name are not asserted.
"""
import math

NUM_CU = 256


def wscale(M):
    """standard deviation of the filters: 0.7 for motifs of up to 15 letters (what the suite's tolerances were set for),
    0.7 sqrt(15 / M) beyond, so that activations keep that spread"""
    return 0.7 if M <= 15 else 0.7 * math.sqrt(15.0 / M)


def bshift(M):
    """shift of the hidden biases: the constructor's b = ppf(rho = 0.01) sqrt(M) switches the units of long motifs off for
    good (-30 at 171 letters); 3 for motifs of up to 15 letters as everywhere in the suite, beyond that what leaves b
    where 15 letters have it (about -6), so that the chains of every case hold units that are on"""
    return 3.0 if M <= 15 else 3.0 + 2.3263478740408408 * (math.sqrt(M) - math.sqrt(15.0))


def _case(id, A, K, M, ds, pool=1, n=3, L=None, B=4, Lf=None, **regime):
    L = M + 28 if L is None else L
    L -= (L - M + 1) % pool                    # pooled: the hidden length is a multiple of the pooling
    Lf = (L - M + 1 if Lf is None else Lf)
    return dict(id=id, A=A, K=K, M=M, ds=ds, pool=pool, n=n, L=L, B=B, Lf=Lf, regime=regime)


# 1. h|v slab size and mask words; 2. chain v|h column slabs.  The full check of check_model_against_oracle (four chains, as
# long as the data rows unless Lf says otherwise) plus the raw sums.
FULL = [
    _case("dna_3x171_ds_ks16", 4, 3, 171, True, KS=16, split=0, col_slabs=2, slab_n=0),
    _case("dna_40x171_ss_ks16_split_merge", 4, 40, 171, False, KS=16, split=1, col_slabs=2, slab_n=0),
    _case("dna_3x308_ss_ks8", 4, 3, 308, False, KS=8, col_slabs=3, slots=5, slab_n=0),
    _case("dna_3x512_ds_ks8_cols4_slots8", 4, 3, 512, True, KS=8, col_slabs=4, slots=8, slab_n=0),
    _case("a64_5x11_ds_ks16", 64, 5, 11, True, KS=16, col_slabs=2, slab_n=0),
    _case("a64_3x32_ds_ks8", 64, 3, 32, True, KS=8, col_slabs=4, slots=8, slab_n=0),
    _case("a20_4x102_ss_ks8", 20, 4, 102, False, KS=8, col_slabs=5, slots=8, slab_n=0),
    _case("a5_7x300_ds_pool2_ks8", 5, 7, 300, True, pool=2, KS=8, col_slabs=3, slab_n=0),
    _case("dna_3x129_ds_cols2", 4, 3, 129, True, KS=32, col_slabs=2, slab_n=0),
    _case("a64_5x9_ds_cols2", 64, 5, 9, True, KS=32, col_slabs=2, slab_n=0),
    _case("a20_4x26_ss_cols2", 20, 4, 26, False, KS=32, col_slabs=2, slab_n=0),
    _case("a3_3x171_ds_cols2", 3, 3, 171, True, KS=32, col_slabs=2, slab_n=0),
    # 4. statistics
    _case("dna_2x65_ss_Lh4097", 4, 2, 65, False, n=2, L=4161, stats_chunks=2, slab_n=0),
    _case("a3_3x4_ds_Lh4097", 3, 3, 4, True, n=2, L=4100, stats_chunks=2, slab_n=0),
    _case("a5_4x6_ds_pool3_Lh4098", 5, 4, 6, True, pool=3, n=2, L=4103, stats_chunks=2, stats_CH=4095, slab_n=0),
    _case("a3_2100x2_ss_R1", 3, 2100, 2, False, n=3, R=1, split=1, slab_n=0),
    _case("dna_2x257_ss_slots5_cols3", 4, 2, 257, False, KS=16, col_slabs=3, slots=5, slab_n=0),
    # 5. many slabs and the constructor's limits
    _case("dna_2110x10_ss_36slabs", 4, 2110, 10, False, n=2, slab_n=36, split=1),
    _case("dna_65536x1_ss_1093slabs", 4, 65536, 1, False, n=2, L=6, Lf=4, slab_n=1093, NW=2048, split=1),
]

# 3. chain v|h chunks: (case, hidden lengths of the chains and the chunks each one takes)
CHAINS = [
    (_case("dna_2x65_ds", 4, 2, 65, True, n=2, B=2, slab_n=0), [(1984, 1), (1985, 2), (4100, 3)]),
    (_case("a3_6x5_ds", 3, 6, 5, True, n=2, B=2, slab_n=0), [(252, 1), (253, 2), (509, 3)]),
    (_case("a20_5x9_ss", 20, 5, 9, False, n=2, B=2, slab_n=0), [(248, 1), (249, 2), (505, 3)]),
]
FORCED_CHAIN = (_case("dna_10x15_ds_forced", 4, 10, 15, True, n=2, B=2), [(2035, 2)])      # under CRBM_FORCE_BIG=1

# 6. long rows
LONG = [
    _case("dna_2x65_ds_L70001", 4, 2, 65, True, n=2, L=70001, B=2, Lf=29, TS=1, hgv_fits=True, slab_n=0),
    _case("a3_3x4_ds_L70001", 3, 3, 4, True, n=2, L=70001, B=2, Lf=29, TS=1, hgv_fits=True, slab_n=0),
]
REFUSED = _case("a64_3x32_ss_L66000", 64, 3, 32, False, n=2, L=66000, B=2, Lf=29, KS=8, TS=1, hgv_fits=False, slab_n=0)

# 7. dense v|h: (id, A, K, M, ds, n, Lh, dense_slabs)
DENSE = [
    ("a1_3x4_ss", 1, 3, 4, False, 4, 38, 1),
    ("a3_6x5_ds", 3, 6, 5, True, 4, 57, 1),
    ("a20_12x9_ss", 20, 12, 9, False, 3, 70, 1),
    ("a64_5x8_ds", 64, 5, 8, True, 3, 42, 1),
    ("a3_1x2_ds_second_round", 3, 1, 2, True, 9, 59999, 1),
    ("dna_300x40_ds", 4, 300, 40, True, 2, 20, 3),
    ("dna_256x64_ss", 4, 256, 64, False, 2, 20, 4),
    ("dna_65536x1_ss", 4, 65536, 1, False, 2, 4, 16),
    ("dna_10x15_ds", 4, 10, 15, True, 3, 47, 1),
]
