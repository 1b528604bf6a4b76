"""The generic ("big") kernels against the float64 oracle at the geometry the host picks for them (crbm_plan.h:
big_hgv_geom, big_vgh_geom, big_stats_geom, vgh_dense_lds) beyond its first regime: h|v slabs of 16 and 8 motifs and the
merge of several slabs into one mask word, column slabs of the chain v|h filter, its position chunks, chunks / row stride
/ per-thread slots of the statistics kernel, many slabs and the constructor's limits, rows of 70 001 letters, the dense
v|h pass of every alphabet and of models whose filters exceed the LDS, and the update at other hyper-parameters.

tests/generic_geom_cases.py holds the shapes; tests/test_generic_geom_host.py holds each of them to the regime it is named
for on the CPU, so a case here cannot drift back into the first regime unnoticed.  DESIGN.md ("Generic kernels: the
geometry the tests reach") maps regime -> test.

Tolerances are the suite's own (RTOL = 1e-4, the atols of check_model_against_oracle, ties at |p - u| < 1e-6 and at most
1e-4 of the units + 2); filters of motifs beyond 15 letters are drawn with standard deviation 0.7 sqrt(15 / M)
(generic_geom_cases.wscale), so that activations keep the spread those tolerances were set for.  The cap on ties is
asserted on the oracle alone first (oracle_ties): the seeds were picked so that it holds.
"""
import copy
import hashlib
import re

import numpy as np
import pytest

from oracle.crbm_oracle import (synthetic_onehot, hidden_uniforms, visible_uniforms,
                                KIND_API_H, KIND_API_V, KIND_CHAIN_H, KIND_CHAIN_V)
from tests import generic_geom_cases as cases
from tests.test_gpu_parity import (make_pair, check_model_against_oracle, assert_chain_steps, assert_train_steps,
                                   assert_chain_equal_or_tied, assert_samples, _unpack_sums, RTOL, TIE)
from tests.test_gpu_sweeps import _assert_route

pytestmark = pytest.mark.gpu

ids = lambda cs: [c["id"] for c in cs]


def model_kw(c):
    kw = {}
    if c["A"] != 4:
        kw["input_dims"] = c["A"]
    if c["pool"] > 1:
        kw["pooling"] = c["pool"]
    return kw


def oracle_ties(o, steps, width=TIE):
    """On the oracle alone: the samples of `steps` chain steps that lie within `width` of their uniform -- the only ones
    float32 arithmetic may decide differently -- number at most what assert_chain_steps lets differ."""
    o = copy.deepcopy(o)
    ds, pool = o.doublestranded, int(o.pooling)
    B, K, _, Lf = o.fantasy_h.shape
    Lv = Lf + o.motif_length - 1
    idx = np.arange(B) + o.seq_offset
    near = 0
    for _ in range(steps):
        t = o.gibbs_step
        uv = visible_uniforms(o.seed, t, idx, Lv, KIND_CHAIN_V)
        Pv, v = o._computeVgivenH(o.fantasy_h, o.fantasy_h_prime, uv)
        cum = np.cumsum(Pv[:, 0], axis=1)[:, :max(Pv.shape[2] - 1, 1)]
        near += int((np.min(np.abs(cum - uv[:, None, :]), axis=1) < width).sum())
        for strand in range(2 if ds else 1):
            u = hidden_uniforms(o.seed, t, idx, K, Lf, strand, KIND_CHAIN_H)
            P = o._computeHgivenV(v, strand == 1)[0]
            if pool == 1:
                near += int((np.abs(P - u) < width).sum())
            else:
                cg = np.cumsum(P.reshape(B, K, 1, Lf // pool, pool), axis=4)
                ug = u.reshape(B, K, 1, Lf // pool, pool)[..., :1]
                near += int((np.min(np.abs(cg - ug), axis=4) < width).sum())
        o.gibbs_steps(1)
    assert near <= 1e-4 * steps * B * K * Lf * (2 if ds else 1) + 2, near
    return near


def unpack_sums(buf, K, M, A):
    """the packed raw-sum buffer of include/crbm_amd.h for an alphabet of A letters -> dict of arrays"""
    if A == 4:
        return _unpack_sums(buf, K, M)
    KAM = K * A * M
    row = 3 * KAM + 3 * K + A
    d, m = buf[:row + 1], buf[row + 1:]
    return {"vh_d": d[0:KAM], "vh_dp": d[KAM:2 * KAM], "h_d": d[2 * KAM:2 * KAM + K], "h_dp": d[2 * KAM + K:2 * KAM + 2 * K],
            "sw": d[2 * KAM + 2 * K:3 * KAM + 2 * K], "sb": d[3 * KAM + 2 * K:3 * KAM + 3 * K],
            "v_d": d[3 * KAM + 3 * K:3 * KAM + 3 * K + A], "n_d": d[row],
            "vh_m": m[0:KAM], "vh_mp": m[KAM:2 * KAM], "h_m": m[2 * KAM:2 * KAM + K], "h_mp": m[2 * KAM + K:2 * KAM + 2 * K],
            "v_m": m[2 * KAM + 2 * K:2 * KAM + 2 * K + A], "n_m": m[2 * KAM + 2 * K + A]}


def check_raw_sums(c):
    """the packed raw sums of crbm_train_local, key by key against OracleCRBM.local_sums (as
    test_slabbed_statistics_of_generic_models does): the data half always, the model half from the chain both sampled"""
    from crbm_amd._lib import fptr
    A, K, M, ds, n, L = c["A"], c["K"], c["M"], c["ds"], c["n"], c["L"]
    m, o = make_pair(K, M, ds=ds, batchsize=c["B"], cd_k=2, Lf=c["Lf"], seed=9, wscale=cases.wscale(M), bshift=cases.bshift(M), rho=0.02,
                     **model_kw(c))
    _assert_route(m, False)
    D = synthetic_onehot(n, L, seed=17, A=A)
    buf = np.zeros(m._lib.crbm_sums_count(m._h()), dtype=np.float32)
    before = (m.get_fantasy()[0], m.get_fantasy()[1], o.gibbs_step)
    m._call("crbm_train_local", fptr(D), n, L, fptr(buf))
    got = unpack_sums(buf, K, M, A)
    P_m, P_mp, v_m = o.gibbs_steps(2)
    want = o.local_sums(D, P_m, P_mp, v_m)
    h1, h1p = m.get_fantasy()
    same = np.array_equal(h1, o.fantasy_h) and (not ds or np.array_equal(h1p, o.fantasy_h_prime))
    keys = ("vh_d", "h_d", "sw", "sb", "v_d") + (("vh_dp", "h_dp") if ds else ())
    if same:
        keys += ("vh_m", "h_m", "v_m") + (("vh_mp", "h_mp") if ds else ())
    for key in keys:
        atol = 1e-5 + (1.6e-6 * float(np.abs(want[key]).max()) if key.startswith(("vh", "sw")) else 0.0)
        np.testing.assert_allclose(got[key], np.ravel(want[key]), rtol=RTOL, atol=atol, err_msg=c["id"] + " " + key)
    assert got["n_d"] == n and got["n_m"] == c["B"] and np.abs(got["vh_d"]).max() > 0 and np.abs(got["sw"]).max() > 0
    if not same:      # legitimate only through a sample on a tie
        assert_chain_equal_or_tied(m, o, before, 2)


# ---- 1, 2, 4, 5: the full check per shape -----------------------------------------------------------------------------------
@pytest.mark.parametrize("c", cases.FULL, ids=ids(cases.FULL))
def test_full_check_in_the_regime(c):
    """activations of both strands, hit probabilities and summaries, free energy per sequence and per motif, two chain
    steps sample for sample and two PCD updates (check_model_against_oracle), on the generic route; off the slab route
    also the raw sums of crbm_train_local"""
    A, K, M = c["A"], c["K"], c["M"]
    assert c["B"] == 4                                        # what check_model_against_oracle runs and the host test checks
    ws = cases.wscale(M)
    _, o = make_pair(K, M, ds=c["ds"], batchsize=4, Lf=c["Lf"], cd_k=2, bshift=cases.bshift(M), wscale=ws, **model_kw(c))
    oracle_ties(o, 2)
    model = check_model_against_oracle(K, M, c["ds"], c["L"], c["n"], wscale=ws, bshift=cases.bshift(M), Lf=c["Lf"], **model_kw(c))
    _assert_route(model, False)
    if c["regime"].get("slab_n") == 0:
        del model
        check_raw_sums(c)


# ---- 3: chunks of the chain v|h ---------------------------------------------------------------------------------------------
def check_long_chains(c, Lf):
    K, M, ds, A = c["K"], c["M"], c["ds"], c["A"]
    twin = lambda: make_pair(K, M, ds=ds, batchsize=c["B"], cd_k=2, Lf=Lf, bshift=cases.bshift(M), wscale=cases.wscale(M), **model_kw(c))
    m, o = twin()
    _assert_route(m, False)
    # from a state with units on: the first v|h already walks masks in every chunk
    rng = np.random.default_rng(Lf)
    o.fantasy_h = rng.binomial(1, 0.05, size=o.fantasy_h.shape).astype(np.float64)
    if ds:
        o.fantasy_h_prime = rng.binomial(1, 0.05, size=o.fantasy_h.shape).astype(np.float64)
    oracle_ties(o, 2)
    assert_chain_steps(m, o, 2)
    assert o.fantasy_h[:, :, :, -c["M"]:].sum() > 0 and o.fantasy_h[:, :, :, :c["M"]].sum() > 0
    m.set_fantasy(o.fantasy_h.astype(np.float32), o.fantasy_h_prime.astype(np.float32) if ds else None)
    D = synthetic_onehot(c["n"], c["L"], seed=K + M, A=A)
    assert_train_steps(m, o, [D], twin, atol=5e-6)           # the model half takes its statistics from the long chains
    return m


CHAIN_CASES = [(c, Lf) for c, lengths in cases.CHAINS for Lf, _ in lengths]


@pytest.mark.parametrize("c,Lf", CHAIN_CASES, ids=["%s_Lv%d" % (c["id"], Lf + c["M"] - 1) for c, Lf in CHAIN_CASES])
def test_chain_vgh_chunks(c, Lf):
    check_long_chains(c, Lf)


def test_chain_vgh_chunks_on_a_model_the_specialised_kernels_take(monkeypatch):
    """10 x 15 under CRBM_FORCE_BIG=1 at Lv = 2049 (a second chunk of one position): against the oracle, and the
    specialised path gives the same chain up to ties"""
    c, ((Lf, _),) = cases.FORCED_CHAIN
    monkeypatch.setenv("CRBM_FORCE_BIG", "1")
    check_long_chains(c, Lf)
    pair = lambda: make_pair(c["K"], c["M"], ds=True, batchsize=c["B"], Lf=Lf, cd_k=2, bshift=3.0, wscale=0.7)
    slow, _ = pair()
    _assert_route(slow, False)
    monkeypatch.delenv("CRBM_FORCE_BIG")
    fast, _ = pair()
    _assert_route(fast, True)
    fast.gibbsSteps(2)
    slow.gibbsSteps(2)
    for a, b in zip(fast.get_fantasy(), slow.get_fantasy()):
        assert (a != b).mean() < 1e-3                              # identical up to p == u ties (float rounding of the two paths)
    assert (fast.get_fantasy_visible() != slow.get_fantasy_visible()).mean() < 1e-3
    assert fast.get_fantasy()[0].sum() > 0


# ---- 6: long rows -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("c", cases.LONG, ids=ids(cases.LONG))
def test_long_rows(c):
    """rows of 70 001 letters (one row per tile; byte rows of that length leave the letters' share of the LDS no row at
    all, the clamp gives one): activations, probabilities, samples, free energy"""
    A, K, M, ds, n, L = c["A"], c["K"], c["M"], c["ds"], c["n"], c["L"]
    m, o = make_pair(K, M, ds=ds, batchsize=c["B"], cd_k=2, Lf=c["Lf"], bshift=cases.bshift(M), wscale=cases.wscale(M), **model_kw(c))
    _assert_route(m, False)
    D = synthetic_onehot(n, L, seed=K + M, A=A)
    for flip in (False, True):
        np.testing.assert_allclose(m._bottomUpActivity(D, flip), o._bottomUpActivity(D, flip), rtol=1e-5, atol=2e-5)
        p, h = m._computeHgivenV(D, flip, rng_step=4)
        pref = o._computeHgivenV(D, flip)[0]
        np.testing.assert_allclose(p, pref, rtol=RTOL, atol=1e-7)
        assert_samples(h, pref, hidden_uniforms(m.seed, 4, np.arange(n), K, L - M + 1, 1 if flip else 0, KIND_API_H))
        assert h.sum() > 0
    np.testing.assert_allclose(m.motifHitProbs(D), o.motifHitProbs(D), rtol=RTOL, atol=1e-7)
    np.testing.assert_allclose(m.freeEnergy(D), o.freeEnergy(D), rtol=RTOL, atol=1e-6)
    np.testing.assert_allclose(m.freeEnergy(D, True), o.freeEnergy(D, True), rtol=RTOL, atol=2e-5)


def test_a_row_too_long_for_the_lds_is_refused_and_the_handle_lives_on():
    """64 letters, 3 x 32: a slab's filters take 96 KB, a row of 66 000 bytes does not fit beside them.  The h|v launch is
    refused (CRBM_ERR_INVALID: the sequence is too long for a model of this size), and the handle serves the next call."""
    from crbm_amd import _lib
    c = cases.REFUSED
    A, K, M, ds = c["A"], c["K"], c["M"], c["ds"]
    m, o = make_pair(K, M, ds=ds, batchsize=c["B"], cd_k=2, Lf=c["Lf"], bshift=cases.bshift(M), wscale=cases.wscale(M), **model_kw(c))
    D = synthetic_onehot(c["n"], c["L"], seed=3, A=A)
    with pytest.raises(Exception, match="sequence too long.*model of this size") as e:
        m._bottomUpActivity(D)
    assert int(re.search(r"\((-?\d+)\)", str(e.value)).group(1)) == _lib.ERR_INVALID
    assert "motif_length" not in str(e.value)
    short = synthetic_onehot(3, M + 28, seed=4, A=A)
    np.testing.assert_allclose(m._bottomUpActivity(short), o._bottomUpActivity(short), rtol=1e-5, atol=2e-5)
    np.testing.assert_allclose(m.freeEnergy(short), o.freeEnergy(short), rtol=RTOL, atol=1e-6)


# ---- 7: the dense v|h pass --------------------------------------------------------------------------------------------------
# sha256 of the activity, probability and sample bytes that the 10 x 15 case gave at the parent of the change that made
# vgh_dense_kernel stage its filters slab by slab (recorded on an MI355X from the inputs below)
DENSE_10x15_PARENT_SHA256 = "76d604b7038575bf5fe451b07a89b7f2f0b0f8e2b7a44118fff866212834fd75"


def dense_outputs(d):
    """the model and oracle of a dense v|h case, its hidden input and what the three API calls give for it"""
    name, A, K, M, ds, n, Lh, _ = d
    m, o = make_pair(K, M, ds=ds, batchsize=2, cd_k=2, Lf=4 if K > 1000 else 20, wscale=cases.wscale(M),
                     **({"input_dims": A} if A != 4 else {}))
    rng = np.random.default_rng(8 + K)
    density = min(0.1, 30.0 / (K * M))                         # a few dozen units on per visible position at most
    h = rng.binomial(1, density, size=(n, K, 1, Lh)).astype(np.float32)
    hp = rng.binomial(1, density, size=h.shape).astype(np.float32) if ds else None
    oa = m._topDownActivity(h, hp)
    op = m._topDownProbabilityOfHidden(h, hp)
    op2, sample = m._computeVgivenH(h, hp, rng_step=2)
    return m, o, h, hp, oa, op, op2, sample


def dense_digest(oa, op, sample):
    return hashlib.sha256(oa.tobytes() + op.tobytes() + sample.tobytes()).hexdigest()


@pytest.mark.parametrize("d", cases.DENSE, ids=[d[0] for d in cases.DENSE])
def test_dense_vgh(d, monkeypatch):
    """_topDownActivity, _topDownProbabilityOfHidden and _computeVgivenH: activity at the tolerance of test_topdown,
    probabilities at RTOL, samples against the oracle's on visible_uniforms(..., KIND_API_V) under its tie rule"""
    name, A, K, M, ds, n, Lh, _ = d
    L = Lh + M - 1
    if A == 4 and K > 64:
        monkeypatch.setenv("CRBM_SLAB_STATS", "0")             # (no slab model: this pass never takes one)
    m, o, h, hp, oa, op, op2, sample = dense_outputs(d)
    assert oa.shape == (n, 1, A, L) and op.shape == oa.shape and sample.shape == oa.shape
    np.testing.assert_equal(op, op2)
    ctrl = o._topDownActivity(h, hp)
    assert np.abs(ctrl - o.c.reshape(1, 1, A, 1)).max() > 0
    np.testing.assert_allclose(oa, ctrl, rtol=1e-5, atol=1e-5)
    ctrl_p = o._topDownProbability(ctrl)
    np.testing.assert_allclose(op, ctrl_p, rtol=RTOL, atol=1e-7)
    np.testing.assert_array_equal(sample.sum(axis=2), 1.0)
    u = visible_uniforms(m.seed, 2, np.arange(n), L, KIND_API_V)
    ref = o._topDownSample(ctrl_p, u)
    bad = (sample != ref).any(axis=2)[:, 0]
    gap = np.min(np.abs(np.cumsum(ctrl_p[:, 0], axis=1)[:, :max(A - 1, 1)] - u[:, None, :]), axis=1)
    assert (gap < TIE).sum() <= 1e-4 * n * L + 2                  # on the oracle alone: the cap can hold
    assert np.all(gap[bad] < TIE), "visible sample differs away from a tie"
    assert bad.sum() <= 1e-4 * n * L + 2
    if name == "dna_10x15_ds":
        assert dense_digest(oa, op, sample) == DENSE_10x15_PARENT_SHA256


# ---- 8: the update at other hyper-parameters --------------------------------------------------------------------------------
HYPER = [dict(momentum=0.0, learning_rate=0.1, lambda_rate=0.0, rho=0.02),
         dict(momentum=0.5, learning_rate=0.01, lambda_rate=1.0, rho=0.0)]          # rho = 0: the derived default
HYPER_MODELS = [("dna_10x15_ds", 4, 10, 15, True, True), ("dna_300x10_ss", 4, 300, 10, False, False), ("a3_6x5_ds", 3, 6, 5, True, False)]


@pytest.mark.parametrize("hyper", HYPER, ids=["mu0_lr.1_lambda0_rho.02", "mu.5_lr.01_lambda1_rho_derived"])
@pytest.mark.parametrize("name,A,K,M,ds,spec", HYPER_MODELS, ids=[h[0] for h in HYPER_MODELS])
def test_update_hyper_parameters(name, A, K, M, ds, spec, hyper):
    """two PCD updates on the specialised update (10 x 15), big_update_kernel behind the slabs (300 x 10) and another
    alphabet: every other training test runs momentum 0.95, learning rate 0.1, lambda 0.1"""
    kw = dict(hyper, **({"input_dims": A} if A != 4 else {}))
    twin = lambda: make_pair(K, M, ds=ds, batchsize=4, cd_k=2, Lf=51, bshift=3.0, wscale=0.7, **kw)
    m, o = twin()
    _assert_route(m, spec)
    want_rho = hyper["rho"] or 1.0 / (K * M) / (2.0 if ds else 1.0)
    assert o.rho == pytest.approx(want_rho) and m.rho == pytest.approx(want_rho)
    D = synthetic_onehot(4, M + 50, seed=K + M, A=A)
    W0 = o.W.copy()
    assert_train_steps(m, o, [D, D], twin, atol=5e-6)
    assert np.abs(o.W - W0).max() > 0
    if hyper["momentum"] == 0.0:
        # without momentum the velocity IS the last step
        np.testing.assert_allclose(m.get_velocities()[0], o.vW, rtol=RTOL, atol=5e-6)
