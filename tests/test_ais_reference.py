"""The yardstick of annealed importance sampling (tests/ais_reference.py) against exact enumeration, before anything is
compared with it: for models small enough that all A^L sequences can be summed, the estimate of log Z must lie within
4 standard errors of the exact value and the standard error must be below 0.02 (1024 runs, 100 and 400 temperatures,
the default seed).  Closed forms: W = 0 gives every run the same weight; one temperature step is plain importance
sampling from the base-rate model."""
import numpy as np
import pytest

from oracle.crbm_oracle import OracleCRBM
from tests import ais_reference as ref

RUNS = 1024


def tiny(K, M, ds, A=4, wseed=11, c=None):
    rng = np.random.default_rng(wseed)
    kw = {"input_dims": A} if A != 4 else {}
    o = OracleCRBM(K, M, doublestranded=ds, batchsize=4, cd_k=1, fantasy_hidden_len=8,
                   W=rng.standard_normal((K, 1, A, M)).astype(np.float32), **kw)
    o.b = np.linspace(-2.0, -3.0, K).astype(np.float32).astype(np.float64).reshape(1, K)
    if c is not None:
        o.c = np.asarray(c, dtype=np.float32).astype(np.float64).reshape(1, A)
    return o


# (name, K, M, ds, A, L)
CASES = [("3x3_ds_L8", 3, 3, True, 4, 8), ("4x4_ss_L8", 4, 4, False, 4, 8), ("3x3_ds_alpha3_L10", 3, 3, True, 3, 10)]


@pytest.mark.parametrize("T", [100, 400])
@pytest.mark.parametrize("case", CASES, ids=[c[0] for c in CASES])
def test_estimate_against_exact_enumeration(case, T):
    name, K, M, ds, A, L = case
    o = tiny(K, M, ds, A)
    exact = ref.exact_log_partition(o, L)
    r = ref.ais(o, L, RUNS, T)
    est = ref.estimate(r["logw"], ref.log_partition_base(o, L))
    print("%s T=%d: exact %.6f, estimate %.6f, stderr %.5f, |diff|/stderr %.2f, ess %.0f"
          % (name, T, exact, est["logZ"], est["stderr"], abs(est["logZ"] - exact) / est["stderr"], est["ess"]))
    assert est["stderr"] <= 0.02
    assert abs(est["logZ"] - exact) <= 4 * est["stderr"]


def test_estimate_with_a_base_rate_model_of_its_own():
    """c != 0 and cA != c (log letter frequencies): the (1 - beta) cA term of log p* and of the visible sampler"""
    o = tiny(3, 3, True, c=[0.3, -0.2, 0.1, -0.4])
    cA = np.log(np.array([0.4, 0.1, 0.2, 0.3]))
    exact = ref.exact_log_partition(o, 8)
    r = ref.ais(o, 8, RUNS, 100, cA=cA)
    est = ref.estimate(r["logw"], ref.log_partition_base(o, 8, cA))
    print("exact %.6f, estimate %.6f, stderr %.5f" % (exact, est["logZ"], est["stderr"]))
    assert est["stderr"] <= 0.02
    assert abs(est["logZ"] - exact) <= 4 * est["stderr"]


@pytest.mark.parametrize("ds", [False, True])
def test_zero_filters_give_every_run_the_same_weight(ds):
    K, M, L = 4, 3, 9
    o = tiny(K, M, ds)
    o.W[:] = 0.0
    S, Lh = (2 if ds else 1), L - M + 1
    want = S * Lh * (np.logaddexp(0.0, o.b.ravel()) - np.log(2.0)).sum()
    r = ref.ais(o, L, 64, 20)
    np.testing.assert_allclose(r["logw"], want, rtol=0, atol=1e-12)
    # and the estimate is the exact partition function of independent letters and units
    exact = L * np.logaddexp.reduce(o.c.ravel()) + S * Lh * np.logaddexp(0.0, o.b.ravel()).sum()
    est = ref.estimate(r["logw"], ref.log_partition_base(o, L))
    np.testing.assert_allclose(est["logZ"], exact, rtol=0, atol=1e-10)
    assert est["stderr"] < 1e-12


def test_one_temperature_step_is_plain_importance_sampling():
    o = tiny(3, 3, True, c=[0.2, -0.1, 0.0, 0.1])
    L, runs = 8, 256
    cA = np.log(np.array([0.25, 0.35, 0.15, 0.25]))
    r = ref.ais(o, L, runs, 1, cA=cA, states=True)
    v0 = r["trajectory"][0]
    want = ref.log_p_star(o, v0, 1.0, cA) - ref.log_p_star(o, v0, 0.0, cA)
    np.testing.assert_allclose(r["logw"], want, rtol=0, atol=1e-11)
    # log p*_0 is the base-rate model's: sum_p cA[v_p] + S K Lh ln 2
    np.testing.assert_allclose(ref.log_p_star(o, v0, 0.0, cA), cA[v0].sum(axis=1) + 2 * 3 * (L - 2) * np.log(2.0), atol=1e-12)
    # and v_0 follows softmax(cA): letter frequencies of 2048 draws within 5 binomial standard deviations
    freq = np.bincount(v0.ravel(), minlength=4) / v0.size
    p = np.exp(cA)
    assert np.all(np.abs(freq - p) < 5 * np.sqrt(p * (1 - p) / v0.size))


def test_runs_are_keyed_by_their_global_index():
    o = tiny(3, 3, True)
    a = ref.ais(o, 8, 12, 10)
    b = ref.ais(o, 8, 7, 10, run_offset=5)
    np.testing.assert_array_equal(a["logw"][5:], b["logw"])
    np.testing.assert_array_equal(a["v"][5:], b["v"])
