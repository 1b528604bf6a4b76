"""The samplers' counter words across their range, on the GPU against the float64 oracle.

Every sample the library draws is a Philox-4x32 value of the counter (chain or row index, position,
kind|strand|sub|group, step) under the key (seed_lo, seed_hi).  The rest of the suite visits seeds below 2^32 (seed_hi = 0),
steps of a handful and chain offsets 0 and 4096; here the seed has a high word (SEED_HI, bit 63 set, low word 5), the step
counters cross 2^16, 2^31 and 2^32 inside a launch, and the chain / row / run indices cross them inside a batch
(tests/rng_counter_cases.py: the settings and the case table).  Sections:

  1  the chain of the specialised kernels, both geometry forms (CRBM_GEOM=2 / 0), dense top-down, pooled
  2  the chain of the slab and generic routes
  3  partitioned launches of 8192 chains (seq_offset + c0), blocks of 16 chains against the oracle
  4  the training launch, resident and host-array entry points, both geometry forms
  5  the stand-alone samplers (_computeHgivenV / _computeVgivenH: rng_step, rows indexed from the shard offset)
  6  the evaluation sample at row indices past 2^16 (one-hot host rows and a resident set, slab boundaries around it)
  7  annealed importance sampling at run offsets whose batch crosses 2^16 and 2^32
  8  the counters' bookkeeping across entry points; the checkpoint round trip of a 64-bit seed and a step >= 2^31

Samples are compared sample for sample; a difference is accepted only on a |p - u| < 1e-6 tie, under the helpers' caps
(assert_chain_steps, assert_train_steps, check_against_yardstick).  tests/test_rng_counter_cases.py pins on the CPU that
the oracle's own trajectory of every case stays inside those caps, so no case can pass by excusing differences as ties.
Every test prints the ties it met ("ties met: ...").
"""
import ctypes

import numpy as np
import pytest

from tests import ais_reference as ref
from tests import rng_counter_cases as cases
from tests.rng_counter_cases import SEED_HI, SETTINGS, MASK32, TIE
from tests.test_gpu_ais import crbm_ais, segment_of, _bits
from tests.test_gpu_geometry import _launch_counts, _state, _same
from tests.test_gpu_parity import (assert_chain_steps, assert_chain_equal_or_tied, assert_train_steps, assert_samples,
                                   _cfg2_model, RTOL)
from tests.test_gpu_sweeps import _model, _assert_route, _budget

pytestmark = pytest.mark.gpu


def _install(model, o, setting, h0, hp0):
    """the setting's seed, step and chain offset and the state h0 / hp0 on the handle, mirrored on the oracle"""
    seed, step0, offset = SETTINGS[setting]
    model._h()
    model.set_rng(seed, step0, 0)
    model._call("crbm_set_shard", offset)
    model.set_fantasy(h0, hp0)
    cases.set_oracle(o, setting, h0, hp0)
    return seed, step0, offset


def _launches(model, o, setting, h0, hp0, launches):
    """launches of `launches` steps from h0 under the setting -> the states after each, the geometry-compiled launches
    among them; the oracle is left at the state before the first"""
    _install(model, o, setting, h0, hp0)
    before = _launch_counts(model)[0]
    states = []
    for k in launches:
        model.gibbsSteps(k)
        states.append(_state(model))
    return states, _launch_counts(model)[0] - before


def _against_oracle(model, o, setting, h0, hp0, steps):
    """after `steps` steps in all: the counters crbm_get_rng reports, then the chain against the oracle's -> ties"""
    seed, step0, offset = SETTINGS[setting]
    assert model.get_rng() == (seed, (step0 + steps) & MASK32, 0), "crbm_get_rng after %d steps" % steps
    o.gibbs_steps(steps)
    ties = assert_chain_equal_or_tied(model, o, (h0, hp0, step0), steps)
    assert o.fantasy_h.sum() > 0
    return ties


def _collect(failures, label, fn):
    """run one setting; an assertion that fails is kept under its label, so that one run names every word that is wrong"""
    try:
        return fn()
    except AssertionError as e:
        failures.append("%s: %s" % (label, str(e).strip() or "assertion failed"))
        return 0


# ---- 1. the chain, specialised kernels, both geometry forms -------------------------------------------------------------
@pytest.mark.parametrize("shape,settings", list(zip(cases.CHAIN_SHAPES, cases.CHAIN_SETTINGS)),
                         ids=["%dx%d_%s_Lf%d_B%d_S%d" % (s[0], s[1], "ds" if s[2] else "ss", s[3], s[4], s[5]) for s in cases.CHAIN_SHAPES])
def test_chain_of_the_specialised_kernels(shape, settings, monkeypatch):
    K, M, ds, Lf, B, S, form = shape
    monkeypatch.setenv("CRBM_GIBBS_S", str(S))
    h0, hp0 = cases.chain_h0(K, ds, Lf, B)
    pairs = {}
    for mode in ("2", "0"):                                 # one pair per form, reused across the settings
        monkeypatch.setenv("CRBM_GEOM", mode)
        pairs[mode] = cases.spec_pair(K, M, ds, Lf, B)
        pairs[mode][0]._h()
    failures, ties = [], 0
    for setting in settings:
        def one(setting=setting):
            model, o = pairs["2"]
            compiled, n_compiled = _launches(model, o, setting, h0, hp0, cases.CHAIN_LAUNCHES)
            t = _against_oracle(model, o, setting, h0, hp0, sum(cases.CHAIN_LAUNCHES))
            runtime, n_runtime = _launches(pairs["0"][0], pairs["0"][1], setting, h0, hp0, cases.CHAIN_LAUNCHES)
            assert n_runtime == 0 and n_compiled == (len(cases.CHAIN_LAUNCHES) if form == "compiled" else 0)
            for a, b in zip(compiled, runtime):
                _same(a, b)                                 # both forms leave the same bits after every launch
            assert pairs["0"][0].get_rng() == (SETTINGS[setting][0], (SETTINGS[setting][1] + 6) & MASK32, 0)
            return t
        ties += _collect(failures, setting, one)
    if "seed_hi" in settings:
        def differs():
            model, o = pairs["2"]
            hi = _launches(model, o, "seed_hi", h0, hp0, (1,))[0][0]
            model.set_rng(5, 0, 0)
            model.set_fantasy(h0, hp0)
            model.gibbsSteps(1)
            assert not np.array_equal(hi[0], model.get_fantasy()[0]), "the chain of SEED_HI is the chain of seed 5: the high key word is dropped"
            return 0
        _collect(failures, "seed_hi against seed 5", differs)
    print("ties met: section 1, %s: %d in %d settings" % (shape[:6], ties, len(settings)))
    assert not failures, "\n".join(failures)


@pytest.mark.parametrize("name,K,M,ds,Lf,B,pool,env", cases.CHAIN_EXTRA, ids=[c[0] for c in cases.CHAIN_EXTRA])
def test_chain_of_the_dense_and_the_pooled_kernels(name, K, M, ds, Lf, B, pool, env, monkeypatch):
    from crbm_amd._lib import CrbmLaunchInfo
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    model, o = cases.spec_pair(K, M, ds, Lf, B, **({"pooling": pool} if pool > 1 else {}))
    _assert_route(model, True)
    info = CrbmLaunchInfo()
    model._check(model._lib.crbm_get_launch_info(model._h(), ctypes.byref(info)))
    assert info.gibbs_sparse == (0 if env.get("CRBM_TOPDOWN") == "dense" else 1)
    h0, hp0 = cases.pooled_h0(K, ds, Lf, B, pool) if pool > 1 else cases.chain_h0(K, ds, Lf, B)
    _launches(model, o, "ALL", h0, hp0, cases.CHAIN_LAUNCHES)
    ties = _against_oracle(model, o, "ALL", h0, hp0, sum(cases.CHAIN_LAUNCHES))
    print("ties met: section 1, %s: %d" % (name, ties))


# ---- 2. the chain on the other routes ------------------------------------------------------------------------------------
@pytest.mark.parametrize("setting", cases.BOTH)
@pytest.mark.parametrize("name", cases.ROUTE_CLASSES)
def test_chain_of_the_slab_and_generic_routes(name, setting, monkeypatch):
    cls = cases.route_class(name)
    model, o = _model(cls, monkeypatch, batchsize=cases.ROUTE_B, seed=SEED_HI)          # (_assert_route inside)
    h0, hp0 = cases.route_h0(cls)
    seed, step0, offset = _install(model, o, setting, h0, hp0)
    model.gibbsSteps(1)
    model.gibbsSteps(2)
    ties = _against_oracle(model, o, setting, h0, hp0, cases.ROUTE_STEPS)
    # ... and step by step from identical states
    _install(model, o, setting, h0, hp0)
    ties += assert_chain_steps(model, o, cases.ROUTE_STEPS)
    assert model.get_rng()[:2] == (seed, (step0 + cases.ROUTE_STEPS) & MASK32)
    print("ties met: section 2, %s %s: %d" % (name, setting, ties))


# ---- 3. partitioned launches at full width -------------------------------------------------------------------------------
def _part_model(chains, offset):
    m = _cfg2_model(chains, offset, seed=SEED_HI)
    m.set_rng(gibbs_step=cases.PART_STEP)
    return m


def _partition(m):
    """(partitions, chains per partition) of the handle's plain launches, from crbm_get_launch_info: the partitions are
    whole tiles of gibbs_seqs_per_tile chains (crbm_plan.h, plan_chain_parts)"""
    from crbm_amd._lib import CrbmLaunchInfo
    info = CrbmLaunchInfo()
    m._check(m._lib.crbm_get_launch_info(m._h(), ctypes.byref(info)))
    S, parts = info.gibbs_seqs_per_tile, info.chain_parts
    tiles = -(-cases.PART_CHAINS // S)
    return parts, -(-tiles // parts) * S


@pytest.mark.parametrize("offset,cross,oracle", [(cases.PART_OFFSET, 2**16 - cases.PART_OFFSET, True),
                                                 (cases.PART_WRAP_OFFSET, 2**32 - cases.PART_WRAP_OFFSET, False)],
                         ids=["across_2p16", "across_2p32"])
def test_partitioned_launches_at_full_width(offset, cross, oracle):
    B = cases.PART_CHAINS
    a = _part_model(B, offset)
    parts, part_chains = _partition(a)
    assert parts > 1 and 0 < part_chains < B
    a.gibbsSteps(3)
    ha, va = a.get_fantasy()[0], a.get_fantasy_visible()
    b = _part_model(B, offset)
    b.gibbsSteps(1)
    b.gibbsSteps(2)
    np.testing.assert_array_equal(b.get_fantasy()[0], ha)
    np.testing.assert_array_equal(b.get_fantasy_visible(), va)
    assert a.get_rng() == b.get_rng() == (SEED_HI, (cases.PART_STEP + 3) & MASK32, 0)
    assert 0.001 < ha.mean() < 0.2
    ties = 0
    for start in cases.part_blocks(part_chains, cross):
        twin = _part_model(cases.PART_BLOCK, (offset + start) & MASK32)
        twin.gibbsSteps(3)
        sl = slice(start, start + cases.PART_BLOCK)
        np.testing.assert_array_equal(twin.get_fantasy()[0], ha[sl], err_msg="chains %d.. of the partitioned launch" % start)
        np.testing.assert_array_equal(twin.get_fantasy_visible(), va[sl], err_msg="letters of chains %d.." % start)
        if oracle:
            o = cases.part_oracle(start, offset)
            twin.set_rng(gibbs_step=cases.PART_STEP)
            met = assert_chain_steps(twin, o, 3)
            if met == 0:                                    # no tie met: the oracle's chain is the handle's
                np.testing.assert_array_equal(ha[sl], o.fantasy_h)
            ties += met
    print("ties met: section 3, offset %d (%d partitions of %d chains): %d" % (offset, parts, part_chains, ties))


# ---- 4. the training launch ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("entry", ["resident", "host"])
@pytest.mark.parametrize("setting", cases.BOTH)
def test_training_launch(setting, entry, monkeypatch):
    monkeypatch.setenv("CRBM_GIBBS_S", str(cases.TRAIN["S"]))
    seed, step0, offset = SETTINGS[setting]
    n, batches = cases.TRAIN["n"], cases.train_batches()

    def pair():
        m, o = cases.train_pair(setting)
        m._h()
        m._call("crbm_set_shard", offset)
        m.set_rng(gibbs_step=step0)
        return m, o

    def resident(m, D):
        m._upload(D, 0)
        m._call("crbm_train_step_resident", 0, n)

    def run(mode):
        monkeypatch.setenv("CRBM_GEOM", mode)
        model, o = pair()
        before = _launch_counts(model)[0]
        tied = assert_train_steps(model, o, batches, pair, step=resident if entry == "resident" else None)
        assert model.get_rng()[:2] == (seed, (step0 + cases.TRAIN["updates"] * cases.TRAIN["cd_k"]) & MASK32)
        out = [model.motifs.get_value(), model.bias.get_value(), model.c.get_value(), *model.get_velocities(), *_state(model)]
        return out, _launch_counts(model)[0] - before, tied

    compiled, n_compiled, tied = run("2")
    runtime, n_runtime, tied0 = run("0")
    assert n_runtime == 0 and n_compiled >= cases.TRAIN["updates"]
    _same(compiled, runtime)
    assert np.abs(compiled[-3]).sum() > 0
    print("ties met: section 4, %s %s: %d updates" % (setting, entry, tied + tied0))


# ---- 5. stand-alone samplers ---------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def api_model():
    m, o = cases.api_pair()
    m._h()
    m._call("crbm_set_shard", cases.API_OFFSET)
    return m, o


@pytest.mark.parametrize("R", cases.API_STEPS)
@pytest.mark.parametrize("flip", [False, True])
def test_stand_alone_hidden_sampler(api_model, flip, R):
    m, o = api_model
    data, P, u = cases.api_hidden_case(o, flip, R)
    p, h = m._computeHgivenV(data, flip, rng_step=R)
    np.testing.assert_allclose(p, P, rtol=RTOL, atol=1e-7)
    assert_samples(h, p.astype(np.float64), u)
    want = (P > u).astype(np.float32)
    assert np.all(np.abs(P - u)[h != want] < TIE), "sample differs from the oracle's away from a tie"
    print("ties met: section 5, hidden flip %d step %d: %d" % (flip, R, int((h != want).sum())))


@pytest.mark.parametrize("R", cases.API_STEPS)
@pytest.mark.parametrize("ds", [False, True])
def test_stand_alone_visible_sampler(api_model, ds, R):
    m, o = api_model
    h, hp, P, u, want = cases.api_visible_case(o, ds, R)
    p, sample = m._computeVgivenH(h, hp, rng_step=R)
    np.testing.assert_allclose(p, P, rtol=1e-5, atol=1e-5)
    np.testing.assert_array_equal(sample.sum(axis=2), 1.0)
    bad = (sample != want).any(axis=2)[:, 0]
    gap = np.min(np.abs(np.cumsum(P[:, 0], axis=1) - u[:, None, :]), axis=1)          # the cumulative-gap rule of test_topdown
    assert np.all(gap[bad] < TIE), "visible sample differs away from a tie"
    assert bad.sum() <= 1
    print("ties met: section 5, visible ds %d step %d: %d" % (ds, R, int(bad.sum())))


# ---- 6. the evaluation sample at high row indices ------------------------------------------------------------------------
def _eval_resident(m, lo, hi):
    mfe, nmh = ctypes.c_float(), ctypes.c_float()
    m._call("crbm_eval_data_resident", lo, hi, ctypes.byref(mfe), ctypes.byref(nmh))
    return mfe.value, nmh.value


@pytest.fixture(scope="module")
def eval_case():
    m, o = cases.eval_pair()
    _assert_route(m, True)                                  # the specialised h|v kernel, not a slab or generic route
    codes = cases.eval_codes()
    m._upload(codes, 0)
    m._call("crbm_dataset_select", 0)
    counts = {step: cases.eval_counts(o, codes, SEED_HI, step) for step in cases.EVAL_STEPS}     # computed once, never changed
    data = cases.onehot(codes)
    fe = float(np.mean(np.concatenate([o.freeEnergy(data[a:a + 10000].astype(np.float64)) for a in range(0, len(codes), 10000)])))
    return m, o, codes, data, counts, fe


@pytest.mark.parametrize("step", cases.EVAL_STEPS)
def test_evaluation_sample_past_row_65536(eval_case, step, monkeypatch):
    m, o, codes, data, counts, fe = eval_case
    E = cases.EVAL
    n, split, K, L = E["n"], E["split"], E["K"], E["L"]
    units = K * (L - E["M"] + 1)
    ones, near = counts[step]
    assert ones[split:].sum() > 0 and near.sum() <= cases.chain_cap(n * units)
    ties = 0
    for src, in_bytes in (("onehot", 4 * 4 * L), ("resident", 0)):
        # slabs with a boundary below and one above row 65536 (starts 51000 and 68000: a launch whose first row is past
        # 2^16), slabs one of which starts at row 65535, then the default budget (one slab)
        for rows in E["slabs"] + (None,):
            _budget(monkeypatch, in_bytes + (K + 1) * 4, rows)
            m.set_rng(gibbs_step=0, eval_step=step)
            mfe, nmh = m._evaluateData(data) if src == "onehot" else _eval_resident(m, 0, n)
            assert m.get_rng()[2] == (step + 1) & MASK32
            assert abs(mfe - fe) <= RTOL * abs(fe) + 1e-6
            total = int(round(float(nmh) * n * units))
            assert abs(total - ones.sum()) <= near.sum(), (src, rows, total, int(ones.sum()))
            ties += abs(total - int(ones.sum()))
            if src == "onehot":
                continue
            # Rows 65536.. on their own.  A resident range draws with the row's index WITHIN the call, so the tail of the
            # set as a call of its own would draw rows 0..4463; the head [0, 65536) has the indices it has in the whole
            # call, and the whole call's count less the head's is the count of rows 65536..69999 at those indices.
            m.set_rng(gibbs_step=0, eval_step=step)
            head = int(round(float(_eval_resident(m, 0, split)[1]) * split * units))
            assert abs(head - ones[:split].sum()) <= near[:split].sum()
            assert abs((total - head) - ones[split:].sum()) <= near[split:].sum(), (rows, total - head, int(ones[split:].sum()))
    # Mini-batches: batch b draws with step + b (modulo 2^32), rows indexed from 0 within the batch.  The loop over
    # crbm_eval_data_resident gives every batch's count as an integer (a batch has 1.6e6 units: exact in a float), held to
    # the oracle's by the near-tie rule; the one-call epoch evaluation must then be that loop's mean bit for bit.
    _budget(monkeypatch, 0, None)
    bs = 20000
    nb = -(-n // bs)
    m.set_rng(gibbs_step=0, eval_step=step)
    sfe = snmh = 0.0
    for i in range(nb):
        rows = codes[i * bs:(i + 1) * bs]
        o1, n1 = cases.eval_counts(o, rows, SEED_HI, (step + i) & MASK32)
        bfe, bnmh = _eval_resident(m, i * bs, i * bs + rows.shape[0])
        assert m.get_rng()[2] == (step + i + 1) & MASK32
        got = int(round(float(bnmh) * rows.shape[0] * units))
        assert abs(got - o1.sum()) <= n1.sum(), (i, got, int(o1.sum()))
        ties += abs(got - int(o1.sum()))
        sfe, snmh = sfe + bfe, snmh + bnmh
    m.set_rng(gibbs_step=0, eval_step=step)
    a, b = ctypes.c_double(), ctypes.c_double()
    m._call("crbm_eval_epoch_resident", bs, ctypes.byref(a), ctypes.byref(b))
    assert m.get_rng()[2] == (step + nb) & MASK32
    assert a.value == sfe / nb and b.value == snmh / nb and b.value > 0
    print("ties met: section 6, eval_step %d: %d units" % (step, ties))


def test_evaluation_sample_of_a_slab_model(monkeypatch):
    cls = cases.route_class(cases.EVAL_SLAB_CLASS)
    name, K, M, ds, A, pool, Lf, L, env, spec = cls
    m, o = _model(cls, monkeypatch, seed=SEED_HI)
    n, step = cases.EVAL_SLAB_ROWS, 2**32 - 1
    codes = cases.eval_codes(n, L)
    data = cases.onehot(codes)
    ones, near = cases.eval_counts(o, codes, SEED_HI, step)
    units = K * (L - M + 1)
    _budget(monkeypatch, 4 * A * L + (K + 1) * 4, cases.EVAL_SLAB_SLAB)
    m.set_rng(gibbs_step=0, eval_step=step)
    mfe, nmh = m._evaluateData(data)
    assert m.get_rng()[2] == 0
    total = int(round(float(nmh) * n * units))
    assert ones.sum() > 0 and abs(total - ones.sum()) <= near.sum(), (total, int(ones.sum()))
    print("ties met: section 6, slab model: %d units" % abs(total - int(ones.sum())))


# ---- 7. annealed importance sampling -------------------------------------------------------------------------------------
@pytest.mark.parametrize("run_offset", cases.AIS_OFFSETS)
def test_ais_run_indices(run_offset):
    m, o = cases.ais_pair()
    L, runs, T = cases.AIS["L"], cases.AIS["runs"], cases.AIS["T"]
    cA = cases.ais_base(run_offset)
    betas = np.linspace(0.0, 1.0, T + 1).astype(np.float32)
    tied, worst = ref.check_against_yardstick(segment_of(m, L, runs, betas, cA, SEED_HI, run_offset), o, L, runs, betas,
                                              cA.astype(np.float64), SEED_HI, RTOL, max_tied=cases.AIS["max_tied"],
                                              run_offset=run_offset, label="run_offset %d" % run_offset)
    rc, s0, w0 = crbm_ais(m, L, runs, betas, 0, T, cA, SEED_HI, run_offset=run_offset)
    m._check(rc)
    rc, s5, w5 = crbm_ais(m, L, runs, betas, 0, 5, cA, SEED_HI, run_offset=run_offset)              # the ladder over two calls
    rc2, s16, w16 = crbm_ais(m, L, runs, betas, 5, T, cA, SEED_HI, state=s5, logw=w5, run_offset=run_offset)
    assert rc == 0 and rc2 == 0 and np.array_equal(s0, s16) and _bits(w0, w16)
    rc, sa, wa = crbm_ais(m, L, 40, betas, 0, T, cA, SEED_HI, run_offset=run_offset)                # the runs over two calls
    rc2, sb, wb = crbm_ais(m, L, 24, betas, 0, T, cA, SEED_HI, run_offset=(run_offset + 40) & MASK32)
    assert rc == 0 and rc2 == 0
    assert np.array_equal(s0, np.concatenate([sa, sb])) and _bits(w0, np.concatenate([wa, wb]))
    rc, s1, w1 = crbm_ais(m, L, runs, betas, 0, T, cA, 5, run_offset=run_offset)                    # the seed's low word alone
    assert rc == 0 and not np.array_equal(s0, s1), "the runs of SEED_HI are the runs of seed 5: the high key word is dropped"
    print("ties met: section 7, run_offset %d: %d runs set aside" % (run_offset, tied))


# ---- 8. counter bookkeeping across entry points --------------------------------------------------------------------------
def test_counter_bookkeeping_across_entry_points():
    """One handle at ALL: after every call crbm_get_rng equals the tally kept by hand -- no counter skipped, none used twice
    -- and the chain is the oracle's after the same chain steps (tests/test_rng_counter_cases.py: no draw of that chain
    is on a tie)."""
    m, o = cases.book_pair()
    seed, step0, offset = SETTINGS["ALL"]
    h0, hp0 = cases.chain_h0(cases.BOOK["K"], True, cases.BOOK["Lf"], cases.BOOK["B"])
    D, n = cases.book_data(), 13
    m._h()
    m._call("crbm_set_shard", offset)
    m.set_fantasy(h0, hp0)
    tally = {"g": step0, "e": 2**32 - 1}
    m.set_rng(seed, tally["g"], tally["e"])

    def check(what, g=0, e=0):
        tally["g"], tally["e"] = tally["g"] + g, tally["e"] + e
        assert m.get_rng() == (seed, tally["g"] & MASK32, tally["e"] & MASK32), what

    def chain_is_the_oracles(what):
        h, hp = m.get_fantasy()
        np.testing.assert_array_equal(h, o.fantasy_h, err_msg=what)
        np.testing.assert_array_equal(hp, o.fantasy_h_prime, err_msg=what)
        np.testing.assert_array_equal(m.get_fantasy_visible(), o.last_v_model, err_msg=what)

    check("at the start")
    m.gibbsSteps(3)
    check("gibbsSteps(3)", g=3)
    m._call("crbm_gibbs_steps_async", 2)
    m._call("crbm_sync")
    check("crbm_gibbs_steps_async(2)", g=2)
    o.gibbs_steps(cases.BOOK["first"])
    chain_is_the_oracles("after 5 steps")
    m._upload(D, 0)
    m._call("crbm_dataset_select", 0)
    m._call("crbm_train_step_resident", 0, n)
    check("crbm_train_step_resident", g=cases.BOOK["cd_k"])
    o.train_step(D)
    chain_is_the_oracles("after the update")
    ms = ctypes.c_float()
    k, launches = cases.BOOK["timed"]
    m._call("crbm_time_gibbs", k, launches, ctypes.byref(ms))
    check("crbm_time_gibbs", g=k * launches)
    o.gibbs_steps(k * launches)
    m._evaluateData(D)
    check("_evaluateData", e=1)
    r = m.logPartition(D.shape[3], runs=8, betas=4)
    assert np.isfinite(r["logZ"])
    check("logPartition")
    assert np.all(np.isfinite(m.freeEnergy(D)))
    check("freeEnergy")
    chain_is_the_oracles("at the end")
    assert o.gibbs_step & MASK32 == tally["g"] & MASK32 and o.fantasy_h.sum() > 0


def test_checkpoint_keeps_a_64_bit_seed_and_a_high_step(tmp_path):
    """saveState / loadState at SEED_HI (bit 63 set) and gibbs_step >= 2^31: the counters come back as they were and the
    next steps are the same bits"""
    from crbm_amd import CRBM
    seed, step0, offset = SETTINGS["ALL31"]
    a, o = cases.spec_pair(6, 9, True, 40, 8, seed=seed)
    h0, hp0 = cases.chain_h0(6, True, 40, 8)
    _install(a, o, "ALL31", h0, hp0)
    a.set_rng(seed, step0, 2**32 - 1)
    a.gibbsSteps(3)
    fn = str(tmp_path / "state.pkl")
    a.saveState(fn)
    b = CRBM.loadState(fn)
    assert b.seed == seed
    b._h()
    b._call("crbm_set_shard", offset)
    assert a.get_rng() == b.get_rng() == (seed, (step0 + 3) & MASK32, 2**32 - 1) and b.get_rng()[1] >= 2**31
    a.gibbsSteps(2)
    b.gibbsSteps(2)
    _same(_state(a), _state(b))
    assert a.get_rng() == b.get_rng() == (seed, (step0 + 5) & MASK32, 2**32 - 1)
