"""Pins tests/tsne_reference.py, the yardstick of the t-SNE tests: to scikit-learn's private functions where they import
(its P at k = n - 1, its KL and gradient, 1e-9 relative), to a central finite difference of its own KL, and to the planted
three-cluster set, whose conditions it must hold itself over the seeds of tests/test_gpu_tsne.py (which quotes the band
of its final KL)."""
import numpy as np
import pytest

from tests import tsne_reference as R
from tests.test_emu_tsne import step_inputs
from tests.test_gpu_tsne import PLANTED_SEEDS, PLANTED_BAND


def _sklearn():
    try:
        from sklearn.manifold import _t_sne
    except Exception:                                             # not installed, or a version without the module
        return None
    return _t_sne if hasattr(_t_sne, "_joint_probabilities") and hasattr(_t_sne, "_kl_divergence") else None


@pytest.mark.parametrize("n,scale", [(65, 10.0), (257, 1e-4), (257, 10.0)])
def test_against_scikit_learn(n, scale):
    sk = _sklearn()
    if sk is None:
        pytest.skip("sklearn.manifold._t_sne with _joint_probabilities and _kl_divergence is not available")
    from scipy.spatial.distance import squareform
    X = R.feature_rows(n, 10, seed=n + 1, duplicates=0)             # the rows of test_emu_tsne.step_inputs(n, ., seed=n)
    idx, d2 = R.neighbors(X, n - 1)
    # scikit-learn stops a row's bisection once |H - log(perplexity)| <= 1e-5; with that stop the reference walks the
    # same betas (the kernel and the reference's default run all 100 evaluations)
    P = R.symmetrize_dense(idx, R.affinities(d2, 30.0, tol=1e-5)[1])
    theirs = sk._joint_probabilities(R.d2_matrix(X), 30.0, 0)
    mine = squareform(P, checks=False)
    assert np.allclose(P, P.T, rtol=0, atol=0) and abs(P.sum() - 1.0) < 1e-12
    assert np.abs(np.maximum(mine, np.finfo(np.float64).eps) - theirs).max() <= 1e-9 * theirs.max()
    y = (scale * np.random.default_rng(n).standard_normal((n, 2)))
    full = squareform(theirs)
    ref = R.kl_gradient(full, y)
    kl, grad = sk._kl_divergence(y.ravel().copy(), theirs, 1.0, n, 2)
    assert abs(ref["kl"] - kl) <= 1e-9 * abs(kl)
    assert np.abs(ref["grad"].ravel() - grad).max() <= 1e-9 * np.abs(grad).max()


@pytest.mark.parametrize("scale,ex", [(1e-4, 1.0), (10.0, 1.0), (1.0, 1.0)])
def test_gradient_is_the_derivative_of_the_kl(scale, ex):
    _, P, y, _, _ = step_inputs(65, scale, seed=65)
    y = y.astype(np.float64)
    g = R.kl_gradient(P, y, ex)["grad"]
    # w = 1 / (1 + d^2) varies on a length of 1 whatever the scale of y: the step is 1e-4 of max(scale, 1), the central
    # difference's truncation (h^2 / 6 times the third derivative) then of the order 1e-8 of the gradient; two float64 KL
    # values of a few eps each add 8 eps |KL| / h
    h = 1e-4 * max(scale, 1.0)
    kl0 = R.kl_gradient(P, y)["kl"]
    for i, c in ((0, 0), (7, 1), (33, 0), (64, 1)):
        up, down = y.copy(), y.copy()
        up[i, c] += h
        down[i, c] -= h
        fd = (R.kl_gradient(P, up)["kl"] - R.kl_gradient(P, down)["kl"]) / (2 * h)
        assert abs(fd - g[i, c]) <= 1e-5 * np.abs(g).max() + 8 * 2.2e-16 * abs(kl0) / h, (i, c, fd, g[i, c])


def test_exaggeration_scales_the_attraction_only():
    _, P, y, _, _ = step_inputs(65, 10.0, seed=65)
    a, b = R.kl_gradient(P, y, 1.0), R.kl_gradient(P, y, 12.0)
    assert np.allclose(b["grad"] - a["grad"], 4.0 * 11.0 * a["A"], rtol=1e-12, atol=0) and a["kl"] == b["kl"]


def test_neighbours_break_ties_by_index():
    X = R.feature_rows(65, 1, seed=66, eighths=True)
    idx, d2 = R.neighbors(X, 64)
    assert np.all(np.sort(idx, axis=1) == np.delete(np.tile(np.arange(65), (65, 1)), np.arange(65) * 66).reshape(65, 64))
    same = d2[:, 1:] == d2[:, :-1]
    assert same.any() and np.all(d2[:, 1:] >= d2[:, :-1]) and np.all(idx[:, 1:][same] > idx[:, :-1][same])


def test_planted_set_holds_for_the_reference_alone():
    """every seed: each point's nearest neighbour in the plane carries its own label, and the final KL lies in the band
    tests/test_gpu_tsne.py quotes, widened by its width on either side -- the conditions of the GPU test.  (The band was
    measured with this loop; the trajectory is chaotic, so a machine whose exp differs in the last place spreads
    elsewhere inside it and is not held to its ends.)"""
    X, labels = R.planted(300, 10, 0)
    kls = []
    for seed in PLANTED_SEEDS:
        y, kl, _ = R.embed(X, perplexity=30.0, max_iter=1000, seed=seed)
        assert R.neighbour_purity(y, labels) == 1.0, seed
        kls.append(kl)
    print("final KL per seed:", " ".join("%.4f" % v for v in kls))
    lo, hi = PLANTED_BAND
    assert lo - (hi - lo) <= min(kls) and max(kls) <= hi + (hi - lo)
