"""The analytic null on the GPU (crbm_amd.scoreDistribution, crbm_score_distribution) against tests/null_reference.py.

Device pmf against the reference's scatter programme: every cell the reference holds above 1e-280 agrees within a
relative (8 M + 128) 2^-53 -- one product rounding and three add roundings per position on either side, plus the final
sum over up to 85 contexts -- cells the reference holds at exactly 0 are exactly 0, and |sum pmf - sum init| stays within
the same bound.  Across tile lengths, row groups and both kernel variants the pmf of the same inputs has the same bits.
End to end, scoreDistribution's tail bounds enclose the oracle's enumeration of all 4^M windows (check_tails), and every
refusal of the entry point leaves the output untouched and the handle usable."""
import ctypes

import numpy as np
import pytest

from tests import null_reference as R
from tests.test_gpu_parity import make_pair

pytestmark = pytest.mark.gpu

_DP = ctypes.POINTER(ctypes.c_double)
TILE_DEFAULT = 1024
ENV = ("CRBM_NULL_TILE", "CRBM_NULL_BYTES", "CRBM_NULL_VARIANT")


@pytest.fixture(scope="module")
def model():
    """config #2's double-stranded model: it lends its device"""
    return make_pair(10, 15, ds=True, Lf=186, bshift=3.0, wscale=0.7)[0]


def device_pmf(model, q, order, P, init, G=None):
    from crbm_amd import _lib
    q = np.ascontiguousarray(q, np.int32)
    P, init = np.ascontiguousarray(P, np.float64), np.ascontiguousarray(init, np.float64)
    if G is None:
        G = int(q.max(axis=2).sum(axis=1).max()) + 1
    pmf = np.full((q.shape[0], G), 7.0)
    model._call("crbm_score_distribution", q.ctypes.data_as(_lib._I32P), q.shape[0], q.shape[1], order, P.ctypes.data_as(_DP),
                init.ctypes.data_as(_DP), G, pmf.ctypes.data_as(_DP))
    return pmf


def setting(monkeypatch, tile=None, budget=None, variant=None):
    for name, value in zip(ENV, (tile, budget, variant)):
        if value is None:
            monkeypatch.delenv(name, raising=False)
        else:
            monkeypatch.setenv(name, str(value))


def rows_of(Rn, M, seed, spread):
    """integer weights with min 0 per position, rows of different G_r, and one position of row 0 whose four weights are
    equal (zero shift)"""
    rng = np.random.default_rng(seed)
    q = rng.integers(0, spread, size=(Rn, M, 4))
    if Rn > 1:
        q[1:] = q[1:] * np.arange(Rn - 1, 0, -1)[:, None, None] // Rn
    q -= q.min(axis=2, keepdims=True)
    if M > 2:
        q[0, M // 2] = 0
    return q.astype(np.int32)


_WANT = {}


def reference(key, q, P, init, order):
    """the reference's pmf of every row, computed once per case and never written to"""
    if key not in _WANT:
        _WANT[key] = [R.dp(q[r], P, init, order) for r in range(q.shape[0])]
        for w in _WANT[key]:
            w.setflags(write=False)
    return _WANT[key]


def check(pmf, want, M, total):
    bound = (8 * M + 128) * 2.0 ** -53
    worst = 0.0
    for got, ref in zip(pmf, want):
        assert np.all(got[ref.size:] == 0.0), "mass beyond the row's own range"
        got = got[:ref.size]
        assert np.all(got[ref == 0.0] == 0.0), "a cell the reference holds at 0 is not 0"
        big = ref > 1e-280
        rel = np.abs(got[big] - ref[big]) / ref[big]
        worst = max(worst, float(rel.max()) / bound)
        assert np.all(rel <= bound), ("relative error / bound", worst)
        assert abs(got.sum() - total) <= bound * total, (got.sum(), total)
    return worst


def inits_of(P, order, seed):
    return (("stationary", R.start(P, order, "stationary")), ("run", R.start(P, order, "run")),
            ("dirichlet", np.random.default_rng(seed).dirichlet(np.ones(R.contexts(order)))))     # mass on partial contexts


@pytest.mark.parametrize("order", [0, 1, 2, 3])
def test_pmf_against_the_reference_and_the_same_bits_in_every_setting(model, monkeypatch, order):
    """six rows of different G_r, M = 7, the largest G about 2 500 (no multiple of any tile): three tiles of the default
    1024, and a halo below 600 cells, which the sibling variant stages at the default tile too (5 * 1623 * 8 bytes)"""
    M = 7
    q = rows_of(6, M, seed=40 + order, spread=600)
    Gr = q.max(axis=2).sum(axis=1) + 1
    G = int(Gr.max())
    assert len(set(Gr.tolist())) == 6 and 2 * TILE_DEFAULT < G and G % 64 != 0 and q.max() > 64 and np.all(q[0, M // 2] == 0)
    P = R.dirichlet_probabilities(order, 60 + order)
    per_row = 2 * R.contexts(order) * G * 8
    for name, init in inits_of(P, order, order):
        want = reference((order, name), q, P, init, order)
        setting(monkeypatch)
        base = device_pmf(model, q, order, P, init)
        check(base, want, M, init.sum())
        settings = [dict(variant=1), dict(tile=64), dict(tile=64, variant=1)] if name != "dirichlet" else [
            dict(variant=1), dict(tile=64), dict(tile=64, variant=1),             # a shift and a halo longer than a tile
            dict(tile=100, variant=1), dict(tile=4096),                           # one tile holds every cell
            dict(budget=per_row), dict(budget=per_row, variant=1, tile=64),       # one row per group
            dict(budget=4 * per_row + 100), dict(budget=4 * per_row + 100, variant=1)]   # groups of 4 and 2 rows
        for kw in settings:
            setting(monkeypatch, **kw)
            assert np.array_equal(device_pmf(model, q, order, P, init), base), (name, kw)
    setting(monkeypatch, tile=64, variant=1)
    wide = device_pmf(model, q, order, P, init, G=G + 77)                          # G beyond every row: zeros behind
    assert np.array_equal(wide[:, :G], base) and np.all(wide[:, G:] == 0.0)


@pytest.mark.parametrize("M", [1, 2, 3])
def test_single_rows_of_short_motifs(model, monkeypatch, M):
    """R = 1 and M below order + 1 for some order: the partial contexts carry the whole distribution"""
    for order in range(4):
        q = rows_of(1, M, seed=7 * M + order, spread=900)
        P = R.dirichlet_probabilities(order, 3 + order)
        for name, init in inits_of(P, order, 11):
            want = [R.dp(q[0], P, init, order)]
            setting(monkeypatch)
            base = device_pmf(model, q, order, P, init)
            check(base, want, M, init.sum())
            for kw in (dict(variant=1), dict(tile=64, variant=1), dict(tile=8)):
                setting(monkeypatch, **kw)
                assert np.array_equal(device_pmf(model, q, order, P, init), base), (order, name, kw)


def test_a_model_of_2_by_40(model, monkeypatch):
    """the weights of a double-stranded model of two motifs of length 40, quantised as scoreDistribution does: four
    rows, 40 launches"""
    from crbm_amd import null
    rng = np.random.default_rng(240)
    W = (rng.standard_normal((2, 4, 40)) * 0.7).astype(np.float32).astype(np.float64)
    w = np.stack([W.transpose(0, 2, 1), W[:, ::-1, ::-1].transpose(0, 2, 1)], axis=1).reshape(4, 40, 4)
    q, offset, err, Gr = null.quantise(w, np.zeros(4), 2.0 ** -5)
    assert 1500 < Gr.max() < 6000 and np.all(err <= 40 * 2.0 ** -6)
    P = R.dirichlet_probabilities(3, 77)
    init = R.start(P, 3, "stationary")
    want = [R.dp(q[r], P, init, 3) for r in range(4)]
    setting(monkeypatch)
    base = device_pmf(model, q, 3, P, init)
    worst = check(base, want, 40, 1.0)
    print("2 x 40: worst relative error / bound = %.3f" % worst)
    for kw in (dict(variant=1), dict(tile=64, variant=1), dict(budget=3 * 2 * 85 * int(Gr.max()) * 8)):
        setting(monkeypatch, **kw)
        assert np.array_equal(device_pmf(model, q, 3, P, init), base), kw


@pytest.mark.parametrize("ds", [True, False], ids=["double", "single"])
def test_end_to_end_against_the_oracles_enumeration(monkeypatch, ds):
    """fitBackground -> scoreDistribution(step = 2^-4) of a 3 x 6 model: the tail bounds of every motif and strand against
    all 4^6 windows scored by the oracle, under both starts"""
    from crbm_amd import fitBackground, scoreDistribution, null
    from tests import background_reference as B
    setting(monkeypatch)
    m, o = make_pair(3, 6, ds=ds, bshift=-2.0)
    data = B.sample(B.dirichlet_table(2, 41), 2, 5000, seed=1)
    markov = fitBackground(m, data, order=2)
    P = markov.probabilities(1.0)
    w, c = R.window_pwm(o)
    S = 2 if ds else 1
    for kind in ("stationary", "run"):
        d = scoreDistribution(m, markov, step=2 ** -4, start=kind)
        assert d.pmf.shape[:2] == (3, S) and d.pmf.dtype == np.float64 and d.step == 2 ** -4 and d.order == 2 and d.start == kind
        assert d.doublestranded == ds and np.all(d.err <= 6 * 2.0 ** -5) and np.abs(d.pmf.sum(axis=2) - 1.0).max() < 1e-13
        init = R.start(P, 2, kind)
        for k in range(3):
            for s in range(S):
                r = k * S + s
                x, p = R.enumerate_windows(w[r], c[r], P, init, 2)
                t = np.linspace(x.min() - 1.0, x.max() + 1.0, 200)
                bounds = [d.tail_bounds(v) for v in t]
                lower, upper = np.array([b[0][k, s] for b in bounds]), np.array([b[1][k, s] for b in bounds])
                R.check_tails(lower, upper, x, p, t, d.err[k, s])
        assert null.last_device_ms(m) > 0.0
    thr, resolved = d.thresholds(1e-3)
    assert thr.shape == (3, S) and thr.dtype == np.float32 and resolved.all() and np.all((thr > 0) & (thr < 1))
    sites = m.scanSites(data, threshold=0.5)
    if sites.size:
        pv = d.pvalues(sites)
        assert pv.shape == sites.shape and np.all((pv >= 0) & (pv <= 1))


def test_refusals_leave_the_output_untouched_and_the_handle_usable(model, monkeypatch):
    from crbm_amd import _lib
    setting(monkeypatch)
    lib, h = model._lib, model._h()
    P = R.dirichlet_probabilities(1, 0)
    init = R.start(P, 1, "run")
    q = rows_of(2, 3, seed=1, spread=50)
    G = int(q.max(axis=2).sum(axis=1).max()) + 1
    pmf = np.full(2 * G + 5, 9.0)
    ip, dp = _lib._I32P, _DP

    def call(q_=q, R_=2, M_=3, order=1, P_=P, init_=init, G_=G, pmf_=pmf):
        ptr = lambda a, t: None if a is None else np.ascontiguousarray(a).ctypes.data_as(t)
        keep = [None if a is None else np.ascontiguousarray(a) for a in (q_, P_, init_)]
        return lib.crbm_score_distribution(h, ptr(keep[0], ip), R_, M_, order, ptr(keep[1], dp), ptr(keep[2], dp), G_,
                                           None if pmf_ is None else pmf_.ctypes.data_as(dp))

    def refused(rc, why):
        assert rc == _lib.ERR_INVALID and why in lib.crbm_last_error(h).decode(), (rc, lib.crbm_last_error(h))
        assert np.all(pmf == 9.0)

    for kw in (dict(q_=None), dict(P_=None), dict(init_=None), dict(pmf_=None)):
        refused(call(**kw), "null")
    refused(call(R_=0), "R must")
    for M in (0, 513):
        refused(call(M_=M), "M must")
    for order in (-1, 4):
        refused(call(order=order), "order")
    bad = q.copy()
    bad[1, 2, 3] = -1
    refused(call(q_=bad), "negative")
    bad = q.copy()
    bad[1, 2] += 1
    refused(call(q_=bad), "smallest q")
    refused(call(G_=G - 1), "largest G_r")
    huge = q.copy()
    huge[0, 0] = [0, 2 ** 24, 0, 0]
    refused(call(q_=huge), "2^24")
    for value in (-0.1, np.nan, np.inf):
        T = P.copy()
        T[3, 1] = value
        refused(call(P_=T), "negative or not finite")
        i = init.copy()
        i[2] = value
        refused(call(init_=i), "negative or not finite")
    T = P.copy()
    T[2, 0] += 1e-8
    refused(call(P_=T), "sum to 1")
    monkeypatch.setenv("CRBM_NULL_BYTES", str(2 * 5 * G * 8 - 1))
    refused(call(), "larger step")
    monkeypatch.setenv("CRBM_NULL_BYTES", str(2 * 5 * G * 8))      # and the handle still serves: one row per group
    assert call() == 0 and np.all(pmf[2 * G:] == 9.0)
    want = [R.dp(q[r], P, init, 1) for r in range(2)]
    check(pmf[:2 * G].reshape(2, G), want, 3, 1.0)
    ms = ctypes.c_float(-1.0)
    assert lib.crbm_null_ms(h, ctypes.byref(ms)) == 0 and ms.value > 0.0
