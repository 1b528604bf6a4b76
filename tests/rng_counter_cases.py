"""TEST INFRASTRUCTURE: the case table of tests/test_gpu_rng_counters.py (the samplers' counter words -- seed high word,
step, chain / row / run index -- near 2^16, 2^31 and 2^32 on the GPU against the float64 oracle) and of
tests/test_rng_counter_cases.py, which pins on the CPU that the oracle's OWN trajectory of every case stays inside the
helpers' caps on ties: the count of draws with |p - u| < 1e-6 along it.  A GPU case can then not pass by excusing
differences as ties.

Every sample is a Philox-4x32 value of the counter (chain or row index, position, kind|strand|sub|group, step) under
the key (seed_lo, seed_hi).  A setting is (seed, first step, index of chain / row 0); every counter word of the ABI is a
uint32 and wraps, the oracle masks its Python integers to 32 bits.
"""
import copy

import numpy as np

from oracle.crbm_oracle import (OracleCRBM, synthetic_onehot, hidden_uniforms, visible_uniforms,
                                KIND_API_H, KIND_API_V, KIND_CHAIN_H, KIND_CHAIN_V, KIND_EVAL_H)
from tests.test_gpu_geometry import SHAPES as GEOMETRY_SHAPES

TIE = 1e-6
MASK32 = 0xFFFFFFFF

SEED_HI = 0x9E3779B900000005          # low word 5 (the seed of nearly every other test), bit 63 set
STEPS = (2**16 - 2, 2**31 - 2, 2**32 - 2)          # each crossed inside a three-step launch
OFFSETS = (2**16 - 3, 2**31 - 3, 2**32 - 3)        # each crossed inside a batch of 6 or 8 chains; the last one wraps

# name -> (seed, first step, chain / row offset)
SETTINGS = {
    "seed_hi": (SEED_HI, 0, 0),
    "step_2p16": (5, STEPS[0], 0), "step_2p31": (5, STEPS[1], 0), "step_2p32": (5, STEPS[2], 0),
    "offset_2p16": (5, 0, OFFSETS[0]), "offset_2p31": (5, 0, OFFSETS[1]), "offset_2p32": (5, 0, OFFSETS[2]),
    "ALL": (SEED_HI, 2**32 - 2, 2**16 - 3),
    "ALL31": (SEED_HI, 2**31 - 2, 2**31 - 3),
}
EACH_WORD = ("seed_hi", "step_2p16", "step_2p31", "step_2p32", "offset_2p16", "offset_2p31", "offset_2p32")
BOTH = ("ALL", "ALL31")


def chain_cap(draws):
    """assert_chain_steps' cap on ties (tests/test_gpu_parity.py)"""
    return 1e-4 * draws + 2


# ---- 1. the chain, specialised kernels --------------------------------------------------------------------------------
# (K, M, ds, Lf, chains, chains per tile, form under CRBM_GEOM=2): tests/test_gpu_geometry.py SHAPES, then the golden
# mask-width shapes of tests/test_gpu_chain_golden.py
GOLDEN_WIDTHS = [(K, 5, False, 20, 4, 2, "compiled") for K in (7, 16, 21)]
CHAIN_SHAPES = list(GEOMETRY_SHAPES) + GOLDEN_WIDTHS
CHAIN_LAUNCHES = (1, 1, 1, 3)
# shape index -> settings: every word alone on the first shape, the two combined settings everywhere
CHAIN_SETTINGS = [EACH_WORD + BOTH] + [BOTH] * (len(CHAIN_SHAPES) - 1)
# the other specialised kernels, at ALL: (name, K, M, ds, Lf, chains, pooling, environment)
CHAIN_EXTRA = [("dense_10x15_ss", 10, 15, False, 186, 8, 1, {"CRBM_TOPDOWN": "dense"}),
               ("pool4_10x15_ss", 10, 15, False, 36, 7, 4, {})]


def chain_h0(K, ds, Lf, B, density=0.05):
    """the initial state of a chain case: seeded by the shape alone, the same for every setting"""
    rng = np.random.default_rng(40 + Lf + B)
    h0 = rng.binomial(1, density, size=(B, K, 1, Lf)).astype(np.float32)
    hp0 = rng.binomial(1, density, size=(B, K, 1, Lf)).astype(np.float32) if ds else None
    return h0, hp0


def pooled_h0(K, ds, Lf, B, pool):
    """at most one unit on per pooling group (what the pooled sampler leaves)"""
    rng = np.random.default_rng(40 + Lf + B)

    def one():
        pick = rng.integers(0, 4 * pool, size=(B, K, 1, Lf // pool))
        return (pick[..., None] == np.arange(pool)).reshape(B, K, 1, Lf).astype(np.float32)
    return one(), (one() if ds else None)


def set_oracle(o, setting, h0, hp0):
    seed, step0, offset = SETTINGS[setting] if isinstance(setting, str) else setting
    o.seed, o.gibbs_step, o.seq_offset = seed, step0, offset
    o.fantasy_h = h0.astype(np.float64)
    o.fantasy_h_prime = hp0.astype(np.float64) if o.doublestranded else None
    return o


def _visible_gap(Pv, uv):
    cum = np.cumsum(Pv[:, 0], axis=1)[:, :max(Pv.shape[2] - 1, 1)]
    return np.min(np.abs(cum - uv[:, None, :]), axis=1)


def _hidden_near(o, P, u):
    pool = int(getattr(o, "pooling", 1))
    if pool == 1:
        return int((np.abs(P - u) < TIE).sum())
    B, K, _, Lf = P.shape
    cum = np.cumsum(P.reshape(B, K, 1, Lf // pool, pool), axis=4)
    ug = u.reshape(B, K, 1, Lf // pool, pool)[..., :1]
    return int((np.min(np.abs(cum - ug), axis=4) < TIE).sum())


def chain_near_ties(o, steps):
    """Advances the oracle's chain by `steps` Gibbs steps (exactly OracleCRBM.gibbs_steps) and returns the number of draws
    on its way with |p - u| < TIE: visible letters against the inner cumulative thresholds, hidden units (pooled: groups
    against their cumulative probabilities) -- the draws at which assert_chain_steps would accept a difference."""
    ds = o.doublestranded
    B, K, _, Lf = o.fantasy_h.shape
    idx = np.arange(B) + o.seq_offset
    near = 0
    for _ in range(steps):
        t = o.gibbs_step
        uv = visible_uniforms(o.seed, t, idx, Lf + o.motif_length - 1, KIND_CHAIN_V)
        Pv, v = o._computeVgivenH(o.fantasy_h, o.fantasy_h_prime, uv)
        near += int((_visible_gap(Pv, uv) < TIE).sum())
        uh = hidden_uniforms(o.seed, t, idx, K, Lf, 0, KIND_CHAIN_H)
        P, h = o._computeHgivenV(v, False, uh)
        near += _hidden_near(o, P, uh)
        hp = None
        if ds:
            uhp = hidden_uniforms(o.seed, t, idx, K, Lf, 1, KIND_CHAIN_H)
            Pp, hp = o._computeHgivenV(v, True, uhp)
            near += _hidden_near(o, Pp, uhp)
        o.fantasy_h, o.fantasy_h_prime, o.last_v_model = h, hp, v
        o.gibbs_step += 1
    return near


def chain_draws(o, steps):
    B, K, _, Lf = o.fantasy_h.shape
    return steps * B * K * Lf * (2 if o.doublestranded else 1)


def spec_pair(K, M, ds, Lf, B, seed=5, **kw):
    """tests/test_gpu_geometry.py's pair of a shape (model on the host until its first call, oracle)"""
    from tests.test_gpu_parity import make_pair
    return make_pair(K, M, ds=ds, batchsize=B, Lf=Lf, seed=seed, wscale=1.5, bshift=5.0, **kw)


# ---- 2. the chain on the other routes ---------------------------------------------------------------------------------
ROUTE_CLASSES = ("slab_300x10_ss", "slab_150x6_ds_pool2", "big_8x100_ds", "alpha20_12x9_ss", "alpha5_7x6_ds_pool2")
ROUTE_B, ROUTE_STEPS = 6, 3


def route_class(name):
    from tests.test_gpu_sweeps import CLASSES
    return {c[0]: c for c in CLASSES}[name]


def route_h0(cls):
    name, K, M, ds, A, pool, Lf, L, env, spec = cls
    return pooled_h0(K, ds, Lf, ROUTE_B, pool) if pool > 1 else chain_h0(K, ds, Lf, ROUTE_B)


# ---- 3. partitioned launches at full width ----------------------------------------------------------------------------
PART_CHAINS, PART_OFFSET, PART_STEP, PART_BLOCK = 8192, 61440, 2**16 - 2, 16
PART_WRAP_OFFSET = 2**32 - 6000


def part_oracle(start, offset=PART_OFFSET):
    """the oracle of 16 chains of config #2 (tests/test_gpu_parity.py, _cfg2_model) from the zero state"""
    W = np.random.default_rng(42).standard_normal((10, 1, 4, 15)).astype(np.float32)
    o = OracleCRBM(10, 15, doublestranded=False, batchsize=PART_BLOCK, cd_k=1, fantasy_hidden_len=186, seed=SEED_HI, W=W)
    o.gibbs_step, o.seq_offset = PART_STEP, offset + start
    return o


def part_blocks(part_chains, cross):
    """starts of the blocks of 16 chains compared with the oracle: the first, the 16 around the partition boundary, the
    16 around local chain `cross` (where the global index crosses a power of two), the last.  At PART_OFFSET = 61440
    and partitions of 4096 chains (what the plan takes today) the boundary IS global index 65536 -- 61440 + 4096 -- so
    two of the four coincide and three blocks remain: the second partition's launch starts exactly at 2^16.  Only the
    run at PART_WRAP_OFFSET has its crossing (2^32, local chain 6000) inside a partition."""
    starts = [0, part_chains - PART_BLOCK // 2, cross - PART_BLOCK // 2, PART_CHAINS - PART_BLOCK]
    return sorted(set(starts))


# ---- 4. the training launch -------------------------------------------------------------------------------------------
TRAIN = dict(K=10, M=15, B=8, L=64, n=13, cd_k=2, S=2, updates=2)


def train_pair(setting):
    from tests.test_gpu_parity import make_pair
    seed, step0, offset = SETTINGS[setting]
    t = TRAIN
    m, o = make_pair(t["K"], t["M"], ds=True, batchsize=t["B"], Lf=t["L"] - t["M"] + 1, cd_k=t["cd_k"], bshift=4.0, rho=0.02,
                     seed=seed)
    o.gibbs_step, o.seq_offset = step0, offset
    return m, o


def train_batches():
    return [synthetic_onehot(TRAIN["n"], TRAIN["L"], seed=77 + i) for i in range(TRAIN["updates"])]


# ---- 5. stand-alone samplers ------------------------------------------------------------------------------------------
API_STEPS = (2**16 - 1, 2**31, 2**32 - 1)
API_OFFSET = 2**16 - 3
API = dict(K=10, M=5, n=11, L=200)


def api_pair():
    from tests.test_gpu_parity import make_pair
    return make_pair(API["K"], API["M"], seed=SEED_HI)


def api_hidden_case(o, flip, R):
    """(data, oracle probabilities, uniforms) of _computeHgivenV(data, flip, rng_step=R) at shard offset API_OFFSET"""
    data = synthetic_onehot(API["n"], API["L"], seed=3)
    P = o._computeHgivenV(data, flip)[0]
    u = hidden_uniforms(SEED_HI, R, API_OFFSET + np.arange(API["n"]), API["K"], API["L"] - API["M"] + 1, 1 if flip else 0, KIND_API_H)
    return data, P, u


def api_visible_case(o, ds, R):
    """(h, h' or None, oracle probabilities, uniforms, oracle sample) of _computeVgivenH(h, h', rng_step=R)"""
    rng = np.random.default_rng(8)
    shape = (API["n"], API["K"], 1, API["L"] - API["M"] + 1)
    h = rng.binomial(1, 0.1, size=shape).astype(np.float32)
    hp = rng.binomial(1, 0.1, size=shape).astype(np.float32) if ds else None
    P = o._topDownProbability(o._topDownActivity(h, hp))
    u = visible_uniforms(SEED_HI, R, API_OFFSET + np.arange(API["n"]), API["L"], KIND_API_V)
    return h, hp, P, u, o._topDownSample(P, u)


# ---- 6. the evaluation sample at high row indices ---------------------------------------------------------------------
# slabs of 17000 rows start at 51000 and 68000, one boundary on either side of row 65536 (the launch of the last slab
# gets a first row past 2^16); slabs of 21845 rows put a boundary at 65535 (3 x 21845): row 65536 is the second of a slab
EVAL = dict(K=4, M=5, n=70000, L=24, split=65536, slabs=(17000, 21845))
EVAL_STEPS = (2**16 - 1, 2**32 - 1)
EVAL_SLAB_CLASS, EVAL_SLAB_ROWS, EVAL_SLAB_SLAB = "slab_300x10_ss", 200, 64


def eval_pair():
    from tests.test_gpu_parity import make_pair
    return make_pair(EVAL["K"], EVAL["M"], ds=True, seed=SEED_HI, bshift=3.0)


def eval_codes(n=None, L=None, A=4):
    return np.random.default_rng(6).integers(0, A, size=(n or EVAL["n"], L or EVAL["L"]), dtype=np.uint8)


def onehot(codes, A=4):
    return np.ascontiguousarray(np.eye(A, dtype=np.float32)[codes].transpose(0, 2, 1)[:, None])


def eval_counts(o, codes, seed, eval_step, chunk=10000):
    """per row: the oracle's count of ones of evaluateData's sample (forward strand, kind EVAL_H, rows indexed from 0
    within the call) and the count of units with |P - u| < TIE; two int64 arrays (n,)"""
    n, L = codes.shape
    K, Lh = o.num_motifs, L - o.motif_length + 1
    ones, near = np.zeros(n, np.int64), np.zeros(n, np.int64)
    for a in range(0, n, chunk):
        D = onehot(codes[a:a + chunk], o.input_dims).astype(np.float64)
        P = o._computeHgivenV(D)[0]
        u = hidden_uniforms(seed, eval_step, np.arange(a, a + D.shape[0]), K, Lh, 0, KIND_EVAL_H)
        ones[a:a + chunk] = (P > u).sum(axis=(1, 2, 3))
        near[a:a + chunk] = (np.abs(P - u) < TIE).sum(axis=(1, 2, 3))
    return ones, near


# ---- 7. annealed importance sampling ----------------------------------------------------------------------------------
AIS = dict(L=200, runs=64, T=16, max_tied=4)
AIS_OFFSETS = (2**16 - 40, 2**32 - 40)
# The base-rate model of each offset (letter frequencies; cA = their logarithms in float32): what draws v_0, the initial
# state of a run.  A ladder of 64 runs x 16 temperatures makes 4e6 draws, about 7 of them within 1e-6 of their threshold
# with most base-rate models (cA = c: 5 and 6 runs); these two keep the runs with such a draw within MAX_TIED.
AIS_BASES = {2**16 - 40: (0.2, 0.3, 0.3, 0.2), 2**32 - 40: (0.25, 0.25, 0.25, 0.25)}


def ais_base(run_offset):
    return np.log(np.array(AIS_BASES[run_offset])).astype(np.float32)


def ais_pair():
    from tests.test_gpu_parity import make_pair
    return make_pair(10, 15, ds=True, Lf=200, bshift=3.0, wscale=0.7)          # tests/test_gpu_ais.py, spec_10x15_ds


def ais_tied_runs(o, run_offset):
    """runs of the yardstick's own ladder with a draw on a tie (what check_against_yardstick could set aside)"""
    from tests import ais_reference as ref
    L, runs, T = AIS["L"], AIS["runs"], AIS["T"]
    betas = ref.ladder(T)
    idx = np.arange(runs) + run_offset
    cA = ais_base(run_offset).astype(np.float64)
    v, P0, u0 = ref.base_draw(o, L, cA, SEED_HI, idx)
    tie = (ref._visible_gap(P0, u0) < TIE).any(axis=1)
    for t in range(T):
        _, P, U, _, _, v = ref.ais_step(o, v, t, betas, cA, SEED_HI, idx)
        tie |= (ref._visible_gap(P["v"], U["v"]) < TIE).any(axis=1)
        for key in ("h", "hp"):
            if P[key] is not None:
                tie |= (np.abs(P[key] - U[key]) < TIE).any(axis=(1, 2, 3))
    return int(tie.sum())


# ---- 8. counter bookkeeping across entry points -----------------------------------------------------------------------
BOOK = dict(K=10, M=15, B=8, Lf=50, cd_k=2, first=5, timed=(2, 2))          # gibbsSteps(3) + async 2; crbm_time_gibbs(k=2, launches=2)


def book_pair():
    from tests.test_gpu_parity import make_pair
    seed, step0, offset = SETTINGS["ALL"]
    m, o = make_pair(BOOK["K"], BOOK["M"], ds=True, batchsize=BOOK["B"], Lf=BOOK["Lf"], cd_k=BOOK["cd_k"], bshift=4.0, rho=0.02, seed=seed)
    set_oracle(o, "ALL", *chain_h0(BOOK["K"], True, BOOK["Lf"], BOOK["B"]))
    return m, o


def book_data():
    return synthetic_onehot(13, BOOK["Lf"] + BOOK["M"] - 1, seed=78)


def book_near_ties():
    """draws on a tie along the oracle's chain of the bookkeeping case: 5 steps, one PCD-2 update, 4 steps"""
    _, o = book_pair()
    near = chain_near_ties(o, BOOK["first"])
    near += chain_near_ties(copy.deepcopy(o), o.cd_k)
    o.train_step(book_data())
    return near + chain_near_ties(o, BOOK["timed"][0] * BOOK["timed"][1])


# ---- every case, for the pin: (id, function -> (near ties on the oracle's own trajectory, cap)) ------------------------
def _chain_case(build, setting, steps, h0fn):
    def run():
        o = build()
        set_oracle(o, setting, *h0fn(o))
        return chain_near_ties(o, steps), chain_cap(chain_draws(o, steps))
    return run


def _train_case(setting):
    def run():
        _, o = train_pair(setting)
        near = 0
        for D in train_batches():
            near += chain_near_ties(copy.deepcopy(o), o.cd_k)
            o.train_step(D)
        return near, chain_cap(chain_draws(o, o.cd_k))           # per update: assert_train_steps replays one at a time
    return run


def _eval_case(step):
    def run():
        _, o = eval_pair()
        ones, near = eval_counts(o, eval_codes(), SEED_HI, step)
        return int(near.sum()), chain_cap(EVAL["n"] * EVAL["K"] * (EVAL["L"] - EVAL["M"] + 1))
    return run


def _eval_slab_case():
    name, K, M, ds, A, pool, Lf, L, env, spec = route_class(EVAL_SLAB_CLASS)
    from tests.test_gpu_parity import make_pair
    _, o = make_pair(K, M, ds=ds, Lf=Lf, bshift=3.0, wscale=0.7, seed=SEED_HI)
    ones, near = eval_counts(o, eval_codes(EVAL_SLAB_ROWS, L), SEED_HI, 2**32 - 1)
    return int(near.sum()), chain_cap(EVAL_SLAB_ROWS * K * (L - M + 1))


def _api_hidden(flip, R):
    def run():
        _, o = api_pair()
        _, P, u = api_hidden_case(o, flip, R)
        return int((np.abs(P - u) < TIE).sum()), 1e-4 * P.size          # assert_samples: bad.mean() < 1e-4
    return run


def _api_visible(ds, R):
    def run():
        _, o = api_pair()
        _, _, P, u, _ = api_visible_case(o, ds, R)
        return int((_visible_gap(P, u) < TIE).sum()), 1                  # test_topdown: bad.sum() <= 1
    return run


def _route_oracle(name):
    from tests.test_gpu_parity import make_pair
    n, K, M, ds, A, pool, Lf, L, env, spec = route_class(name)
    extra = {}
    if A != 4:
        extra["input_dims"] = A
    if pool > 1:
        extra["pooling"] = pool
    return make_pair(K, M, ds=ds, Lf=Lf, bshift=3.0, wscale=0.7, batchsize=ROUTE_B, seed=SEED_HI, **extra)[1]


def all_cases():
    cases = []
    for shape, settings in zip(CHAIN_SHAPES, CHAIN_SETTINGS):
        K, M, ds, Lf, B, S, form = shape
        for s in settings:
            cases.append(("1-chain-%dx%d-%s-Lf%d-B%d-%s" % (K, M, "ds" if ds else "ss", Lf, B, s),
                          _chain_case(lambda K=K, M=M, ds=ds, Lf=Lf, B=B: spec_pair(K, M, ds, Lf, B)[1], s, sum(CHAIN_LAUNCHES),
                                      lambda o, K=K, ds=ds, Lf=Lf, B=B: chain_h0(K, ds, Lf, B))))
    for name, K, M, ds, Lf, B, pool, env in CHAIN_EXTRA:
        kw = {"pooling": pool} if pool > 1 else {}
        cases.append(("1-chain-%s-ALL" % name,
                      _chain_case(lambda K=K, M=M, ds=ds, Lf=Lf, B=B, kw=kw: spec_pair(K, M, ds, Lf, B, **kw)[1], "ALL", sum(CHAIN_LAUNCHES),
                                  lambda o, K=K, ds=ds, Lf=Lf, B=B, pool=pool: pooled_h0(K, ds, Lf, B, pool) if pool > 1 else chain_h0(K, ds, Lf, B))))
    for name in ROUTE_CLASSES:
        for s in BOTH:
            cases.append(("2-route-%s-%s" % (name, s),
                          _chain_case(lambda name=name: _route_oracle(name), s, ROUTE_STEPS, lambda o, name=name: route_h0(route_class(name)))))
    for start in part_blocks(4096, 65536 - PART_OFFSET):           # (the blocks of the partition size the default plan takes)
        cases.append(("3-partitioned-block-%d" % start,
                      _chain_case(lambda start=start: part_oracle(start), (SEED_HI, PART_STEP, PART_OFFSET + start), 3,
                                  lambda o: (np.zeros(o.fantasy_h.shape, np.float32), None))))
    for s in BOTH:
        cases.append(("4-train-%s" % s, _train_case(s)))
    for R in API_STEPS:
        for flip in (False, True):
            cases.append(("5-hidden-flip%d-%d" % (flip, R), _api_hidden(flip, R)))
        for ds in (False, True):
            cases.append(("5-visible-ds%d-%d" % (ds, R), _api_visible(ds, R)))
    for step in EVAL_STEPS:
        cases.append(("6-eval-%d" % step, _eval_case(step)))
    cases.append(("6-eval-slab", _eval_slab_case))
    for off in AIS_OFFSETS:
        cases.append(("7-ais-%d" % off, lambda off=off: (ais_tied_runs(ais_pair()[1], off), AIS["max_tied"])))

    cases.append(("8-bookkeeping", lambda: (book_near_ties(), 0)))          # the GPU test asks for the oracle's very chain
    return cases
