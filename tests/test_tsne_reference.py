"""Pins tests/tsne_reference.py, the yardstick of the t-SNE tests: to scikit-learn's private functions where they import
(its P at k = n - 1, its KL and gradient, 1e-9 relative), to a central finite difference of its own KL, and to the planted
three-cluster set, whose conditions it must hold itself over the seeds of tests/test_gpu_tsne.py (which quotes the band
of its final KL).  kl_gradient_csr and kl_gradient_grouped are pinned to the dense kl_gradient at 1e-12, sparse_joint to what
it promises, the restated host rules to crbm_tsne.h itself, and the reference alone is held to the affinity conditions on
the k = 1024 inputs of the GPU test."""
import numpy as np
import pytest

from tests import tsne_reference as R
from tests.test_emu_tsne import step_inputs, check_affinities
from tests.test_gpu_tsne import PLANTED_SEEDS, PLANTED_BAND, K1024_CASES, AFFINITY_CAP_CASES, knn_reference


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


def _agree(a, b):
    """every entry to 1e-12 of the array's largest"""
    for key in ("A", "R", "grad"):
        assert a[key].shape == b[key].shape and np.abs(a[key] - b[key]).max() <= 1e-12 * np.abs(b[key]).max(), key
    assert abs(a["z"] - b["z"]) <= 1e-12 * b["z"] and abs(a["kl"] - b["kl"]) <= 1e-12 * abs(b["kl"])


@pytest.mark.parametrize("n,k,scale,ex,empty", [(2, None, 10.0, 12.0, False), (65, None, 1e-4, 1.0, False), (257, 90, 10.0, 1.0, True),
                                                (1000, 90, 1e-4, 12.0, False), (1000, 90, 10.0, 12.0, True)])
def test_csr_gradient_equals_the_dense_one(n, k, scale, ex, empty):
    """kl_gradient_csr (row blocks, no n x n P) against kl_gradient on the inputs of the descent tests, an empty row
    among them; a block of 96 rows leaves a short last block"""
    csr, P, y, _, _ = step_inputs(n, scale, seed=n, k=k, empty_row=empty)
    if empty:
        assert csr[0][8] == csr[0][7]
    dense = R.kl_gradient(P, y.astype(np.float64), ex)
    _agree(R.kl_gradient_csr(csr, y, ex), dense)
    _agree(R.kl_gradient_csr(csr, y, ex, block=96), dense)
    _agree(R.at_exaggeration(R.kl_gradient_csr(csr, y, 1.0), ex), dense)
    assert R.kl_gradient_csr(csr, y, ex, want_kl=False)["kl"] is None


def test_sparse_joint():
    for n, empty in ((16385, 300), (1000, None), (700, 7)):
        indptr, indices, values = R.sparse_joint(n, seed=n, empty_row=empty)
        assert indptr.dtype == np.int64 and indices.dtype == np.int32 and values.dtype == np.float32
        assert indptr[0] == 0 and indptr[-1] == indices.size == values.size and 0 <= indices.min() and indices.max() < n
        rows = np.repeat(np.arange(n), np.diff(indptr))
        assert np.all(rows != indices) and (values > 0).all()
        key = rows * n + indices
        assert np.all(np.diff(key) > 0)                                       # rows in order, columns ascend, none twice
        back = np.searchsorted(key, indices.astype(np.int64) * n + rows)       # the transposed entry: there, with the same value
        assert np.array_equal(key[back], indices.astype(np.int64) * n + rows) and np.array_equal(values[back], values)
        assert np.unique(np.diff(indptr)).size > 1
        assert indices[indptr[1] - 1] == n - 1 and indices[indptr[n - 1]] == 0  # rows 0 and n - 1 reach the other's tile
        assert abs(values.astype(np.float64).sum() - 1.0) < 1e-6
        if empty is not None:
            assert indptr[empty + 1] == indptr[empty] and not (indices == empty).any()
        if n <= 1000:                                                         # and the dense reference reads it as such a P
            P = R.csr_to_dense(n, indptr, indices, values.astype(np.float64))
            assert np.array_equal(P, P.T)


def test_grouped_gradient_equals_the_csr_one():
    """n = 2000 rows on G = 37 positions (about 54 coincident rows each): kl_gradient_grouped against kl_gradient_csr at
    y = points[group], with an empty row"""
    n, G = 2000, 37
    rng = np.random.default_rng(37)
    points = (10.0 * rng.standard_normal((G, 2))).astype(np.float32)
    group = rng.integers(0, G, size=n)
    assert np.unique(group).size == G
    csr = R.sparse_joint(n, seed=5, empty_row=11)
    for ex in (1.0, 12.0):
        _agree(R.kl_gradient_grouped(csr, points, group, ex), R.kl_gradient_csr(csr, points[group], ex))


def test_the_restated_host_rules_are_the_header(tmp_path):
    """slice_tiles, slices, sum_chunks and knn_lds_bytes of tests/tsne_reference.py against crbm_tsne.h itself (a host
    program against the emulation's shim), the eight-or-four-waves rule against the text of crbm_tsne_neighbors, and the
    figures the large tests of tests/test_gpu_tsne.py rely on"""
    import os
    import re
    import subprocess
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    ns = [2, 255, 256, 257, 1000, 11520, 11521, 16384, 16385, 16640, 20000, 65536, 65537, 100000, 131073, 524288, 524289, 1 << 20, (1 << 30) - 1, 1 << 30]
    dk = [(1, 1), (1, 1024), (3, 63), (64, 65), (255, 512), (255, 1024), (256, 891), (256, 892), (256, 1024)]
    src = tmp_path / "rules.cpp"
    src.write_text('#include "crbm_tsne.h"\n#include "emu_launch.h"\n#include <cstdio>\n#include <cstdlib>\n'
                   'const bool emu::concurrent_blocks = false;\nusing namespace crbm::tsne;\n'
                   'int main(int argc, char** argv) {\n'
                   '  printf("%d %d %d %d\\n", TJ, SUM_CHUNK, MAX_SLICES, KNN_TILE);\n'
                   '  for (int a = 1; a < argc; ++a) {\n'
                   '    long long n = atoll(argv[a]);\n'
                   '    if (n > 0) printf("%d %d %lld\\n", slice_tiles(n), slices(n), (long long)sum_chunks(n));\n'
                   '    else { int D = (int)(-n >> 16), k = (int)(-n & 0xffff);\n'
                   '      for (int w = 1; w <= 8; w *= 2) printf("%zu ", knn_lds_bytes(D, k, w));\n'
                   '      printf("\\n"); }\n'
                   '  }\n  return 0;\n}\n')
    exe = str(tmp_path / "rules")
    emu = os.path.join(root, "tests", "emu")
    subprocess.check_call(["g++", "-std=c++17", "-O0", "-mf16c", "-I", os.path.join(emu, "shim"), "-I", emu, "-I", os.path.join(root, "crbm_amd", "csrc"),
                           str(src), "-o", exe, "-lpthread"])
    out = subprocess.check_output([exe] + [str(n) for n in ns] + [str(-((D << 16) | k)) for D, k in dk], text=True).splitlines()
    assert [int(v) for v in out[0].split()] == [R.TJ, R.SUM_CHUNK, R.MAX_SLICES, R.KNN_TILE]
    for n, line in zip(ns, out[1:]):
        assert [int(v) for v in line.split()] == [R.slice_tiles(n), R.slices(n), R.sum_chunks(n)], n
        assert R.slices(n) <= R.MAX_SLICES and R.slices(n) * R.slice_tiles(n) * R.TJ >= n > (R.slices(n) - 1) * R.slice_tiles(n) * R.TJ
    for (D, k), line in zip(dk, out[1 + len(ns):]):
        assert [int(v) for v in line.split()] == [R.knn_lds_bytes(D, k, w) for w in (1, 2, 4, 8)], (D, k)
    api = open(os.path.join(root, "crbm_amd", "csrc", "crbm_api.hip")).read()
    rule = re.search(r"int waves = (\d+);[^\n]*\n\s*while \(waves > 1 && tsne::knn_lds_bytes\(D, k, waves\) > (\d+) \* 1024\) waves >>= 1;", api)
    assert rule and rule.groups() == ("8", "128")
    assert R.knn_launch(256, 1024) == (4, 102672) and R.knn_launch(256, 891) == (8, 131040) and R.knn_launch(256, 892)[0] == 4
    assert R.knn_launch(255, 1024)[0] == 4 and R.knn_launch(255, 512) == (8, 106208)
    assert (R.slice_tiles(11520), R.slices(11520)) == (1, 45) and (R.slice_tiles(11521), R.slices(11521)) == (2, 23)
    assert (R.slice_tiles(16384), R.slices(16384)) == (2, 32) and (R.slice_tiles(16385), R.slices(16385)) == (3, 22)
    assert (R.slice_tiles(65537), R.slices(65537), R.sum_chunks(65537)) == (33, 8, 257)
    assert (R.slice_tiles(131073), R.slices(131073), R.sum_chunks(131073)) == (129, 4, 513)


@pytest.mark.parametrize("case", K1024_CASES, ids=lambda c: "%dx%d_k%d_%s" % c)
def test_affinity_conditions_hold_for_the_reference_at_k_1024(case):
    """the inputs of tests/test_gpu_tsne.py::test_affinities_at_the_cap: the reference's own beta and p, rounded to float32
    as the kernel returns them, meet conditions (i) to (iii) of check_affinities, so the test asks nothing of the kernel
    that these data rule out (rows that cannot reach the entropy, tsne_reference.reachable, are held to the uniform p)"""
    _, _, d2 = knn_reference(case)
    for perplexity in [p for c, p in AFFINITY_CAP_CASES if c == case]:
        beta, _ = R.affinities(d2, perplexity)
        beta = beta.astype(np.float32)
        assert np.isfinite(beta).all()
        equal, stuck = check_affinities(d2, perplexity, R.conditional(d2, beta).astype(np.float32), beta)
        assert R.reachable(d2, perplexity).any()
        print(case, perplexity, "rows of equal distances: %d, rows that cannot reach the entropy: %d" % (equal, stuck))
