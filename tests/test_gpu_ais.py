"""Annealed importance sampling on the GPU (crbm_ais, CRBM.logPartition / logLikelihood) against the float64 yardstick
(tests/ais_reference.py, itself pinned by exact enumeration in tests/test_ais_reference.py).

Parity: the final letters of every run equal the yardstick's; a run that differs is replayed through one-step segments
from the yardstick's states and passes only with a demonstrated |p - u| < 1e-6 tie; at most MAX_TIED = 4 of the 64 runs
of a class may be set aside that way.  Log weights of the other runs:
|got - want| <= RTOL |want| + RTOL max_t |log p*_{betas[t+1]}(v_t)|, RTOL = 1e-4 of test_gpu_parity: the project's fp32
criterion at the scale of the quantities differenced.  A run has about 7e4 decisions at L = 200; a tie (width 2e-6)
flips only where float32 rounding lands on the other side of u, so well under one run per class is expected to differ.
The CPU emulation of the same kernel source in float32 (tests/emu/emu_ais.cpp; 64 runs x 16 temperatures, the models,
seed and base-rate models of this file) set aside, on the development machine: spec_10x15_ds (L = 200) 1 of 64 runs
with cA = c and 0 of 64 with a base-rate model of its own; 10 x 5 (L = 83) 0 and 0.  The other classes have no emulator
configuration.  Every figure the GPU run finds is printed by check_against_yardstick.
"""
import ctypes

import numpy as np
import pytest

from tests import ais_reference as ref
from tests.test_gpu_parity import make_pair, RTOL, _cfg2_model
from tests.test_gpu_sweeps import CLASSES, _model, _codes

pytestmark = pytest.mark.gpu

MAX_TIED = 4
U8P = ctypes.POINTER(ctypes.c_uint8)


def crbm_ais(m, L, runs, betas, t0, t1, cA=None, seed=0, state=None, logw=None, run_offset=0, want_state=True):
    """one crbm_ais call -> (rc, state or None, logw)"""
    from crbm_amd._lib import fptr
    betas = np.ascontiguousarray(betas, dtype=np.float32)
    st = None
    if state is not None:
        st = np.ascontiguousarray(state, dtype=np.uint8).copy()
    elif want_state:
        st = np.full((runs, L), 255, np.uint8)
    lw = np.full(runs, np.nan, np.float32) if logw is None else np.ascontiguousarray(logw, dtype=np.float32).copy()
    base = None if cA is None else np.ascontiguousarray(cA, dtype=np.float32)
    h = m._h()
    rc = m._lib.crbm_ais(h, L, runs, run_offset, fptr(betas), betas.size, t0, t1, fptr(base), seed,
                         None if st is None else st.ctypes.data_as(U8P), fptr(lw))
    return rc, st, lw


def segment_of(m, L, runs, betas, cA, seed, run_offset=0):
    def segment(t0, t1, state, logw):
        rc, st, lw = crbm_ais(m, L, runs, betas, t0, t1, cA, seed, state, logw, run_offset)
        m._check(rc)
        return st, lw
    return segment


def _bits(a, b):
    return a.shape == b.shape and np.array_equal(a.view(np.uint32), b.view(np.uint32))


def _oracle_of(m, ds):
    """an OracleCRBM with the parameters of a model that was built without one (config #2's)"""
    from oracle.crbm_oracle import OracleCRBM
    o = OracleCRBM(m.num_motifs, m.motif_length, doublestranded=ds, batchsize=4, cd_k=1, fantasy_hidden_len=8,
                   W=m.motifs.get_value())
    o.b, o.c = m.bias.get_value().astype(np.float64), m.c.get_value().astype(np.float64)
    return o


def _parity_pair(name):
    if name == "spec_10x15_ds":
        return make_pair(10, 15, ds=True, Lf=200, bshift=3.0, wscale=0.7) + (200,)
    if name == "cfg2":
        m = _cfg2_model(64)
        return m, _oracle_of(m, False), 200
    if name == "10x5_ss":
        return make_pair(10, 5, ds=False, Lf=60, bshift=3.0, wscale=0.7) + (83,)
    if name == "100x15_ss":
        return make_pair(100, 15, ds=False, Lf=90, bshift=3.0, wscale=0.7) + (120,)
    if name == "20x40_ds":
        return make_pair(20, 40, ds=True, Lf=70, bshift=3.0, wscale=0.7) + (150,)
    raise KeyError(name)


PARITY = ["spec_10x15_ds", "cfg2", "10x5_ss", "100x15_ss", "20x40_ds"]


@pytest.mark.parametrize("name", PARITY)
@pytest.mark.parametrize("own_base", [False, True], ids=["base_c", "base_own"])
def test_parity_with_the_yardstick(name, own_base):
    m, o, L = _parity_pair(name)
    runs, T, seed = 64, 16, 4242
    cA = np.log(np.array([0.3, 0.2, 0.15, 0.35])).astype(np.float32) if own_base else None
    betas = np.linspace(0.0, 1.0, T + 1).astype(np.float32)
    ref.check_against_yardstick(segment_of(m, L, runs, betas, cA, seed), o, L, runs, betas,
                                None if cA is None else cA.astype(np.float64), seed, RTOL, max_tied=MAX_TIED, label=name)


def _tiny(K, M, ds):
    """the DNA cases of tests/test_ais_reference.py on the GPU"""
    from crbm_amd import CRBM
    from tests.test_ais_reference import tiny
    o = tiny(K, M, ds)
    m = CRBM(K, M, doublestranded=ds, batchsize=4, cd_k=1, fantasy_hidden_len=8, seed=0)
    m.motifs.set_value(o.W.astype(np.float32))
    m.bias.set_value(o.b.astype(np.float32))
    m.c.set_value(o.c.astype(np.float32))
    return m, o


@pytest.mark.parametrize("K,M,ds", [(3, 3, True), (4, 4, False)])
def test_estimator_end_to_end_against_exact_enumeration(K, M, ds):
    L = 8
    m, o = _tiny(K, M, ds)
    exact = ref.exact_log_partition(o, L)
    r = m.logPartition(L, runs=1024, betas=400, return_runs=True)
    margin = 4 * r["stderr"] + RTOL * abs(exact)
    print("exact %.6f, logZ %.6f, stderr %.5f, ess %.0f, |diff| %.5f, margin %.5f"
          % (exact, r["logZ"], r["stderr"], r["ess"], abs(r["logZ"] - exact), margin))
    assert r["logw"].shape == (1024,) and r["logw"].dtype == np.float32
    np.testing.assert_allclose(r["logZ_base"], ref.log_partition_base(o, L), rtol=1e-12)
    assert abs(r["logZ"] - exact) <= margin
    # the log-likelihoods of all 65 536 sequences of length 8 sum to 1 in probability
    seqs = ref.all_sequences(4, L)
    ll = m.logLikelihood(seqs, logZ=r["logZ"])
    assert ll.shape == (4 ** L,) and ll.dtype == np.float32
    total = np.logaddexp.reduce(ll.astype(np.float64))
    print("logsumexp of logLikelihood over all sequences: %.6f" % total)
    assert abs(total) <= margin
    # logZ computed by the call itself: the same ladder, the same value
    ll2 = m.logLikelihood(seqs[:100], runs=1024, betas=400)
    assert _bits(ll2, ll[:100])


@pytest.mark.parametrize("ds", [False, True])
def test_closed_form_zero_filters(ds):
    """W = 0: every run has logw = S K-sum Lh (softplus(b) - ln 2) for cA = c; stderr below 1e-5"""
    m, o = make_pair(10, 5, ds=ds, Lf=60, bshift=3.0)
    W0 = np.zeros_like(m.motifs.get_value())
    m.motifs.set_value(W0)
    o.W[:] = 0.0
    L, runs, T = 83, 64, 16
    S, Lh = (2 if ds else 1), L - 5 + 1
    want = S * Lh * (np.logaddexp(0.0, o.b.ravel()) - np.log(2.0)).sum()
    scale = S * Lh * np.logaddexp(0.0, o.b.ravel()).sum() + L * np.abs(o.c).max()       # |log p*_1| at its largest
    r = m.logPartition(L, runs=runs, betas=T, seed=3, return_runs=True)
    err = np.abs(r["logw"].astype(np.float64) - want)
    print("closed form %.6f, worst error %.3g, bound %.3g, stderr %.3g" % (want, err.max(), RTOL * abs(want) + RTOL * scale, r["stderr"]))
    assert np.all(err <= RTOL * abs(want) + RTOL * scale)
    assert r["stderr"] < 1e-5


def test_closed_form_one_temperature_against_free_energy():
    """T = 1: logw_r = -L freeEnergy(v0_r) - sum_p cA[v0_r[p]] - S K Lh ln 2 with the shipped freeEnergy and v0 from the
    yardstick's base-rate draw (a run whose v0 sits on a tie of that draw is left to the parity test)"""
    m, o = make_pair(10, 15, ds=True, Lf=200, bshift=3.0, wscale=0.7)
    L, runs, seed = 200, 64, 99
    cA = np.log(np.array([0.2, 0.3, 0.3, 0.2])).astype(np.float32)
    idx = np.arange(runs)
    v0, P0, u0 = ref.base_draw(o, L, cA.astype(np.float64), seed, idx)
    clean = ~(ref._visible_gap(P0, u0) < ref.TIE).any(axis=1)
    rc, _, lw = crbm_ais(m, L, runs, [0.0, 1.0], 0, 1, cA, seed)
    m._check(rc)
    fe = m.freeEnergy(np.ascontiguousarray(v0, dtype=np.uint8)).astype(np.float64)
    want = -L * fe - cA.astype(np.float64)[v0].sum(axis=1) - 2 * 10 * (L - 14) * np.log(2.0)
    scale = np.abs(L * fe) + 2 * 10 * (L - 14) * np.log(2.0)
    err = np.abs(lw - want)
    print("T = 1: %d clean runs, worst error / bound %.3g" % (clean.sum(), (err / (RTOL * np.abs(want) + RTOL * scale))[clean].max()))
    assert clean.sum() >= runs - MAX_TIED
    assert np.all(err[clean] <= (RTOL * np.abs(want) + RTOL * scale)[clean])


def test_same_bits_for_every_cut_split_and_run(monkeypatch):
    m, o = make_pair(10, 15, ds=True, Lf=200, bshift=3.0, wscale=0.7)
    L, runs, T, seed = 200, 64, 16, 11
    betas = np.linspace(0.0, 1.0, T + 1).astype(np.float32)
    monkeypatch.delenv("CRBM_AIS_STEPS", raising=False)
    rc, s0, w0 = crbm_ais(m, L, runs, betas, 0, T, None, seed)
    m._check(rc)
    assert s0.max() <= 3 and np.all(np.isfinite(w0))
    rc, s1, w1 = crbm_ais(m, L, runs, betas, 0, T, None, seed)                   # a repeated call
    assert rc == 0 and np.array_equal(s0, s1) and _bits(w0, w1)
    for steps in ("1", "7"):                                                     # launches of 1 and of 7 steps
        monkeypatch.setenv("CRBM_AIS_STEPS", steps)
        rc, s1, w1 = crbm_ais(m, L, runs, betas, 0, T, None, seed)
        assert rc == 0 and np.array_equal(s0, s1) and _bits(w0, w1), steps
    monkeypatch.delenv("CRBM_AIS_STEPS")
    rc, sa, wa = crbm_ais(m, L, 40, betas, 0, T, None, seed)                     # the runs over two calls
    rc2, sb, wb = crbm_ais(m, L, 24, betas, 0, T, None, seed, run_offset=40)
    assert rc == 0 and rc2 == 0
    assert np.array_equal(s0, np.concatenate([sa, sb])) and _bits(w0, np.concatenate([wa, wb]))
    rc, s5, w5 = crbm_ais(m, L, runs, betas, 0, 5, None, seed)                   # the ladder over two calls
    rc2, s16, w16 = crbm_ais(m, L, runs, betas, 5, T, None, seed, state=s5, logw=w5)
    assert rc == 0 and rc2 == 0 and np.array_equal(s0, s16) and _bits(w0, w16)
    rc, s1, w1 = crbm_ais(m, L, runs, betas, 0, T, m.c.get_value().ravel(), seed)   # base_c = c against NULL
    assert rc == 0 and np.array_equal(s0, s1) and _bits(w0, w1)
    rc, s1, w1 = crbm_ais(m, L, runs, betas, 0, T, None, seed, want_state=False)  # state == NULL
    assert rc == 0 and s1 is None and _bits(w0, w1)
    rc, s1, w1 = crbm_ais(m, L, runs, betas, 0, T, None, seed + 1)               # another seed: other runs
    assert rc == 0 and not np.array_equal(s0, s1)


def test_the_handle_is_untouched():
    """two identical handles, one of which runs a ladder between two training steps: parameters, velocities, chains,
    the last visible sample, get_rng() and the next step's result are bit-equal"""
    from oracle.crbm_oracle import synthetic_onehot
    a, _ = make_pair(10, 15, ds=True, batchsize=16, Lf=60, bshift=3.0)
    b, _ = make_pair(10, 15, ds=True, batchsize=16, Lf=60, bshift=3.0)
    D1, D2 = synthetic_onehot(24, 90, seed=1), synthetic_onehot(24, 90, seed=2)
    codes = _codes(50, 90, 4, seed=3)
    for m in (a, b):
        m._upload(codes, 0)
        m._trainingFct(D1)
    r = a.logPartition(90, runs=128, betas=20, base=codes)
    assert np.isfinite(r["logZ"])

    def snapshot(m):
        fe = np.empty(50, np.float32)
        from crbm_amd._lib import fptr
        m._call("crbm_free_energy_resident", 0, 50, fptr(fe), None)
        return [m.motifs.get_value(), m.bias.get_value(), m.c.get_value(), *m.get_velocities(), *m.get_fantasy(),
                m.get_fantasy_visible(), fe], m.get_rng()
    for when in ("after the ladder", "after the next step"):
        (xa, ra), (xb, rb) = snapshot(a), snapshot(b)
        assert ra == rb, when
        for p, q in zip(xa, xb):
            assert _bits(p, q), when
        a._trainingFct(D2)
        b._trainingFct(D2)


def test_refusals(monkeypatch):
    from crbm_amd._lib import ERR_INVALID
    m, _ = make_pair(10, 15, ds=True, Lf=200, bshift=3.0)
    betas = np.linspace(0.0, 1.0, 9).astype(np.float32)
    ok_state = np.zeros((4, 50), np.uint8)

    def refused(needle, model=m, L=50, runs=4, b=betas, t0=0, t1=8, cA=None, state=None, logw=None, nb=None):
        from crbm_amd._lib import fptr
        b = np.ascontiguousarray(b, dtype=np.float32)
        lw = np.zeros(max(runs, 1), np.float32) if logw is None else logw
        base = None if cA is None else np.ascontiguousarray(cA, dtype=np.float32)
        h = model._h()
        rc = model._lib.crbm_ais(h, L, runs, 0, fptr(b), b.size if nb is None else nb, t0, t1, fptr(base), 1,
                                 None if state is None else state.ctypes.data_as(U8P), fptr(lw))
        msg = model._lib.crbm_last_error(h).decode()
        assert rc == ERR_INVALID and needle in msg, (rc, msg)

    refused("motif_length", L=14)
    refused("runs", runs=0)
    refused("runs", runs=-3)
    refused("nbetas", nb=1)
    refused("t0", t0=-1)
    refused("t0", t0=3, t1=3, state=ok_state)
    refused("t0", t1=9)
    refused("decrease", b=[0.0, 0.5, 0.4, 1.0], t1=3)
    refused("[0,1]", b=[0.0, 0.5, 1.5], t1=2)
    refused("[0,1]", b=[-0.1, 0.5, 1.0], t1=2)
    refused("finite", b=[0.0, np.nan, 1.0], t1=2)
    refused("state", t0=2)
    refused("letter code", t0=2, state=np.full((4, 50), 4, np.uint8))
    refused("finite", cA=[0.0, np.inf, 0.0, 0.0])
    refused("LDS", L=40000)                                                      # 320 KB of mask rows per run
    by_name = {c[0]: c for c in CLASSES}
    for cname, needle in (("slab_150x6_ds_pool2", "pooling"), ("slab_300x10_ss", "generic"), ("big_8x100_ds", "generic"),
                          ("alpha20_12x9_ss", "alphabet")):
        cls = by_name[cname]
        g, _ = _model(cls, monkeypatch)
        refused(needle, model=g, L=cls[7])
        with pytest.raises(Exception, match=needle):
            g.logPartition(cls[7], runs=4, betas=8)
        fe = g.freeEnergy(_codes(3, cls[7], cls[4], seed=1))                     # ... and the handle still works
        assert np.all(np.isfinite(fe))
    rc, st, lw = crbm_ais(m, 50, 4, betas, 0, 8, None, 1)                        # ... as does the one that refused all of the above
    assert rc == 0 and np.all(np.isfinite(lw)) and st.max() <= 3


def test_scale_cfg2_model():
    """config #2's model, L = 200, 8192 runs x 1000 temperatures, then logLikelihood of 65 536 rows of codes"""
    m = _cfg2_model(64)
    L = 200
    r = m.logPartition(L, runs=8192, betas=1000)
    assert np.isfinite(r["logZ"]) and np.isfinite(r["stderr"]) and 1.0 <= r["ess"] <= 8192.0
    codes = _codes(65536, L, 4, seed=12)
    ll = m.logLikelihood(codes, logZ=r["logZ"])
    assert ll.shape == (65536,) and np.all(np.isfinite(ll))
    print("logZ %.4f (base %.4f), stderr %.4g, ess %.1f of 8192, mean log-likelihood per base %.5f (uniform: %.5f)"
          % (r["logZ"], r["logZ_base"], r["stderr"], r["ess"], ll.mean() / L, -np.log(4.0)))
    m.motifs.set_value((0.5 * m.motifs.get_value()).astype(np.float32))          # the tables are rebuilt
    r2 = m.logPartition(L, runs=8192, betas=1000)
    assert np.isfinite(r2["logZ"]) and r2["logZ"] != r["logZ"]
