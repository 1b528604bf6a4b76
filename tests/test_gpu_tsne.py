"""t-SNE on the GPU (crbm_tsne_neighbors / _affinities / _descend through crbm_amd.tsne, tsneEmbed, runTSNE) against the
float64 reference of tests/tsne_reference.py: neighbours bit for bit, the three conditions on the affinities, one descent
step at two scales of y and two exaggerations (dense P, CSR rows of unequal length, an empty row), the same bits in two
runs, the planted three-cluster set end to end, runTSNE, and the refusals of the entry points themselves.

Affinities, condition (i): a row with m distances tied for the smallest has entropy >= log m whatever beta is
(tsne_reference.reachable), so with the twelve copies of one row (m = 11) and perplexity 5 no beta exists; such rows are
held to what the kernel documents instead (finite beta, p uniform over the tied) and every other row to 1e-4."""
import numpy as np
import pytest

from tests import tsne_reference as R
from tests.test_emu_tsne import check_affinities, step_inputs, settle, check_step

pytestmark = pytest.mark.gpu

# The planted set (tsne_reference.planted(300, 10, 0), perplexity 30, 1000 iterations, init 'random'): final KL of the
# float64 reference over these seeds, re-measured by tests/test_tsne_reference.py; every run had neighbour purity 1.0.
PLANTED_SEEDS = tuple(range(8))
PLANTED_BAND = (0.6055, 0.6158)


@pytest.fixture(scope="module")
def model():
    from crbm_amd import CRBM
    return CRBM(num_motifs=10, motif_length=15, seed=3)


KNN_CASES = [(2, 1, 1, False), (65, 1, 64, True), (257, 10, 90, False), (1000, 67, 90, False), (300, 10, 299, False),
             (257, 10, 11, False)]
_KNN = {}


def knn_reference(case):
    if case not in _KNN:
        n, D, k, eighths = case
        X = R.feature_rows(n, D, seed=n + D, eighths=eighths)
        _KNN[case] = (X,) + R.neighbors(X, k)
    return _KNN[case]


@pytest.mark.parametrize("case", KNN_CASES, ids=lambda c: "%dx%d_k%d" % c[:3])
def test_neighbours_equal_the_reference_bit_for_bit(model, case):
    from crbm_amd import tsne
    X, ridx, rd2 = knn_reference(case)
    idx, d2 = tsne.neighbors(model, X, case[2])
    assert idx.dtype == np.int32 and d2.dtype == np.float32
    assert np.array_equal(idx, ridx) and np.array_equal(d2.view(np.uint32), rd2.view(np.uint32))
    if case[0] >= 65:
        assert (rd2 == 0).any() and (rd2[:, 1:] == rd2[:, :-1]).any()          # zero distances and ties by index


@pytest.mark.parametrize("perplexity", [5.0, 30.0])
@pytest.mark.parametrize("case", KNN_CASES, ids=lambda c: "%dx%d_k%d" % c[:3])
def test_affinities(model, case, perplexity):
    from crbm_amd import tsne
    k = case[2]
    _, _, d2 = knn_reference(case)
    if not perplexity < k + 1:
        with pytest.raises(ValueError, match="perplexity"):
            tsne.affinities(model, d2, perplexity)
        return
    p, beta = tsne.affinities(model, d2, perplexity)
    equal, stuck = check_affinities(d2, perplexity, p, beta)
    if k == 11:
        assert equal >= 12                                    # the twelve copies of one row: all-equal at k = 11
    if case[0] >= 257 and perplexity == 5.0 and k > 11:
        assert stuck >= 12


STEP_CASES = [(2, None, 1e-4, 12.0, False), (2, None, 10.0, 12.0, False), (65, None, 1e-4, 1.0, False), (65, None, 10.0, 12.0, False),
              (257, None, 10.0, 1.0, False), (257, 90, 1e-4, 12.0, False), (257, 90, 10.0, 1.0, True),
              (1000, None, 1e-4, 12.0, False), (1000, 90, 10.0, 1.0, False), (1000, 90, 10.0, 12.0, True)]


@pytest.mark.parametrize("n,k,scale,ex,empty", STEP_CASES)
def test_one_descent_step(model, n, k, scale, ex, empty):
    from crbm_amd import tsne
    csr, P, y, vel, gains = step_inputs(n, scale, seed=n, k=k, empty_row=empty)
    if k is not None:
        assert np.unique(np.diff(csr[0])).size > 1            # rows of unequal length
    if empty:
        assert csr[0][8] == csr[0][7]
    vel = settle(P, y, vel, ex)
    y1, v1, g1 = y.copy(), vel.copy(), gains.copy()
    got = tsne.descend(model, csr, y1, v1, g1, 1, ex, 50.0, 0.5, want_grad=True, want_kl=True)
    got.update(y=y1, velocity=v1, gains=g1)
    share = check_step(got, P, y, vel, gains, ex, 50.0, 0.5)
    print("gradient error as a share of its bound: %.3g" % share)


def test_same_bits_in_two_runs(model):
    from crbm_amd import tsne
    csr, _, y, vel, gains = step_inputs(1000, 1.0, seed=1000, k=90)
    runs = []
    for _ in range(2):
        state = [y.copy(), vel.copy(), gains.copy()]
        tsne.descend(model, csr, state[0], state[1], state[2], 50, 4.0, 50.0, 0.8)
        runs.append(state)
    assert np.isfinite(runs[0][0]).all() and not np.array_equal(runs[0][0], y)
    for a, b in zip(*runs):
        assert np.array_equal(a.view(np.uint32), b.view(np.uint32))


def test_planted_clusters_end_to_end(model):
    from crbm_amd import tsneEmbed
    X, labels = R.planted(300, 10, 0)
    y, info = tsneEmbed(model, X, perplexity=30.0, max_iter=1000, init="random", seed=0, return_info=True)
    assert y.shape == (300, 2) and y.dtype == np.float32 and np.isfinite(y).all() and info["k"] == 90
    assert R.neighbour_purity(y, labels) == 1.0
    idx, d2 = R.neighbors(X, 90)
    P = R.symmetrize_dense(idx, R.affinities(d2, 30.0)[1])
    kl = R.kl_gradient(P, y.astype(np.float64))["kl"]
    lo, hi = PLANTED_BAND
    print("KL of the returned y by the reference: %.4f (the library's own: %.4f); band %.4f .. %.4f" % (kl, info["kl"][-1][1], lo, hi))
    assert lo - (hi - lo) <= kl <= hi + (hi - lo)
    assert abs(info["kl"][-1][1] - kl) <= 1e-3 * kl and info["kl"][-1][0] == 1000 and len(info["kl"]) == 21
    assert set(info["seconds"]) == {"neighbors", "affinities", "symmetrize", "descend"}
    again = tsneEmbed(model, X, perplexity=30.0, max_iter=1000, init="random", seed=0)       # one call per phase: the same bits
    assert np.array_equal(again.view(np.uint32), y.view(np.uint32))


def test_run_tsne(model):
    from crbm_amd import runTSNE, tsneEmbed, codesToOneHot
    codes = np.random.default_rng(11).integers(0, 4, size=(300, 60), dtype=np.uint8)
    feats = model.motifHitSummary(codes, position_mean=False)["max"]
    want = tsneEmbed(model, feats, max_iter=300, seed=4, init="random")
    for seqs in (codes, codesToOneHot(codes)):
        y = runTSNE(model, seqs, max_iter=300, seed=4, init="random")
        assert y.shape == (300, 2) and y.dtype == np.float32 and np.isfinite(y).all()
        assert np.array_equal(y.view(np.uint32), want.view(np.uint32))
    assert runTSNE(model, codes, max_iter=260).shape == (300, 2)                              # the defaults: init 'pca'


def test_the_entry_points_refuse(model):
    """the C side itself (crbm_amd.tsne checks the same before it calls): CRBM_ERR_INVALID and a reason"""
    from crbm_amd import _lib
    lib, h = _lib.load(), model._h()
    X = R.feature_rows(20, 3, seed=1)
    idx, d2 = np.zeros((20, 5), np.int32), np.zeros((20, 5), np.float32)

    def knn(n, D, k, X=X):
        return lib.crbm_tsne_neighbors(h, _lib.fptr(X), n, D, k, idx.ctypes.data_as(_lib._I32P), _lib.fptr(d2))
    for n, D, k in ((1, 3, 1), (20, 0, 5), (20, 257, 5), (20, 3, 0), (20, 3, 20), (2000, 3, 1025)):
        assert knn(n, D, k) == _lib.ERR_INVALID and lib.crbm_last_error(h)
    bad = X.copy()
    bad[4, 1] = np.nan
    assert knn(20, 3, 5, bad) == _lib.ERR_INVALID and b"finite" in lib.crbm_last_error(h)
    assert knn(20, 3, 5) == 0
    p, beta = np.zeros((20, 5), np.float32), np.zeros(20, np.float32)
    for perplexity in (0.0, -2.0, 6.0, np.inf, np.nan):
        assert lib.crbm_tsne_affinities(h, _lib.fptr(d2), 20, 5, perplexity, _lib.fptr(p), _lib.fptr(beta)) == _lib.ERR_INVALID
    assert lib.crbm_tsne_affinities(h, _lib.fptr(d2), 20, 20, 3.0, _lib.fptr(p), _lib.fptr(beta)) == _lib.ERR_INVALID
    assert lib.crbm_tsne_affinities(h, _lib.fptr(d2), 20, 5, 3.0, _lib.fptr(p), _lib.fptr(beta)) == 0
    (indptr, indices, values), _, y, vel, gains = step_inputs(20, 1.0, seed=2, k=5)

    def descend(indptr, indices, iterations=1, n=20):
        indptr, indices = np.ascontiguousarray(indptr, np.int64), np.ascontiguousarray(indices, np.int32)
        return lib.crbm_tsne_descend(h, n, indptr.ctypes.data_as(_lib._I64P), indices.ctypes.data_as(_lib._I32P), _lib.fptr(values),
                                     _lib.fptr(y), _lib.fptr(vel), _lib.fptr(gains), iterations, 1.0, 1.0, 0.5, None, None, None)
    before = y.copy()
    assert descend(indptr, indices, iterations=-1) == _lib.ERR_INVALID
    assert descend(indptr, indices, n=1) == _lib.ERR_INVALID
    assert descend(indptr + (np.arange(21) == 0), indices) == _lib.ERR_INVALID
    swapped = indptr.copy()
    swapped[3], swapped[4] = indptr[4] + 1, indptr[3]
    assert descend(swapped, indices) == _lib.ERR_INVALID and b"ascend" in lib.crbm_last_error(h)
    for wrong in (-1, 20):
        other = indices.copy()
        other[-1] = wrong
        assert descend(indptr, other) == _lib.ERR_INVALID and b"outside" in lib.crbm_last_error(h)
    assert np.array_equal(before, y)                           # refused before anything ran
    assert descend(indptr, indices) == 0 and not np.array_equal(before, y)
