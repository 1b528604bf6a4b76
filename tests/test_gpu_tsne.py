"""t-SNE on the GPU (crbm_tsne_neighbors / _affinities / _descend through crbm_amd.tsne, tsneEmbed, runTSNE) against the
float64 reference of tests/tsne_reference.py: neighbours bit for bit, the three conditions on the affinities, one descent
step at two scales of y and two exaggerations (dense P, CSR rows of unequal length, an empty row), the same bits in two
runs, the planted three-cluster set end to end, runTSNE, and the refusals of the entry points themselves.  And the limits
the entry points accept: neighbours at k = 1024 and D = 256 (above 64 KB of LDS, eight and four waves per block), the
descent past one tile per slice (n = 11 521, 16 384, 16 385) and past 256 chunk sums (n = 65 537, 131 073), tsneEmbed at k = 1024;
each of these asserts through the host rules restated in tests/tsne_reference.py that its shape takes that path.

Affinities, condition (i): a row with m distances tied for the smallest has entropy >= log m whatever beta is
(tsne_reference.reachable), so with the twelve copies of one row (m = 11) and perplexity 5 no beta exists; such rows are
held to what the kernel documents instead (finite beta, p uniform over the tied) and every other row to 1e-4."""
import numpy as np
import pytest

from tests import tsne_reference as R
from tests.test_emu_tsne import check_affinities, step_inputs, settle, check_step, dense_reference, grad_bound, large_inputs

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
        X = R.descending_rows(n) if eighths == "descending" else R.feature_rows(n, D, seed=n + D, eighths=eighths)
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


# ---- the neighbour kernel at the limits crbm_tsne_neighbors accepts ------------------------------------------------------
# (n, D, k, data) and the launch the driver must choose for it (waves per block, bytes of LDS; None: not asserted)
CAP_CASES = [((1101, 256, 1024, False), (4, 102672)),       # four waves; the last block has three waves without a row
             ((1100, 256, 891, False), (8, 131040)),        # the largest eight-wave request
             ((1100, 256, 892, False), (4, None)),          # the first k that drops to four waves
             ((1027, 255, 1024, False), (4, None)),         # odd D: the row stride equals D
             ((600, 255, 512, False), (8, 106208))]         # eight waves above the 64 KB that need hipFuncSetAttribute
TIE_CASE = (1100, 1, 1024, True)                            # multiples of 1/8 in one dimension: ties across the whole list
HEAD_CASES = [(1100, 1, 1024, "descending"), (200, 1, 65, "descending")]   # every candidate displaces the head of the list
EDGE_CASES = [(130, D, 65, False) for D in (64, 65, 128, 129)] + [(n, 3, n - 1, False) for n in (63, 64, 128)]
TIE3_CASE = (1100, 3, 1024, True)                           # the same in three dimensions: see AFFINITY_CAP_CASES
K1024_CASES = [CAP_CASES[0][0], CAP_CASES[3][0], TIE_CASE, TIE3_CASE, HEAD_CASES[0]]
# Affinities on the d2 of every k = 1024 case at perplexities 1.5, 341 and 1000, but for TIE_CASE at 1.5: its 1100 rows
# take nine values, every row has a hundred or so zero distances, so no row can reach an entropy of log 1.5
# (tsne_reference.reachable) and condition (i) of check_affinities has no row to hold.  TIE3_CASE stands in: the same
# multiples of 1/8 in three dimensions, where a third of the rows have exactly one copy, hence a single smallest distance.
AFFINITY_CAP_CASES = [(c, p) for c in K1024_CASES for p in (1.5, 341.0, 1000.0) if (c, p) != (TIE_CASE, 1.5)]


def _neighbours_equal(model, case):
    from crbm_amd import tsne
    X, ridx, rd2 = knn_reference(case)
    idx, d2 = tsne.neighbors(model, X, case[2])
    assert idx.dtype == np.int32 and d2.dtype == np.float32
    assert np.array_equal(idx, ridx) and np.array_equal(d2.view(np.uint32), rd2.view(np.uint32))
    return ridx, rd2


@pytest.mark.parametrize("case,launch", CAP_CASES, ids=lambda c: "%dx%d_k%d" % c[:3] if len(c) == 4 else "")
def test_neighbours_at_the_caps(model, case, launch):
    """the first launches of tsne_knn_kernel above 64 KB of LDS, with four waves per block, with rows longer than two
    64-lane passes and with lists of more than five 64-entry shift steps to be held to the reference"""
    n, D, k, _ = case
    waves, lds = R.knn_launch(D, k)
    assert waves == launch[0] and lds > 64 * 1024 and (launch[1] is None or lds == launch[1]) and D > 128 and k > 5 * 64
    if case == CAP_CASES[0][0]:
        assert n % waves == 1                                 # waves without a row in the last block
    if case == CAP_CASES[2][0]:
        assert R.knn_launch(D, k - 1)[0] == 8 and R.knn_lds_bytes(D, k, 8) > 128 * 1024
    if D == 255:
        assert (D | 1) == D
    _, rd2 = _neighbours_equal(model, case)
    assert (rd2 == 0).any()                                   # the twelve copies of one row


@pytest.mark.parametrize("case", [TIE_CASE, TIE3_CASE], ids=lambda c: "%dx%d_k%d" % c[:3])
def test_neighbours_tied_across_the_whole_list(model, case):
    _, rd2 = _neighbours_equal(model, case)
    assert np.unique(rd2).size <= (9 if case[1] == 1 else 193) and ((rd2[:, 1:] == rd2[:, :-1]).mean(axis=1) > 0.8).all()


@pytest.mark.parametrize("case", HEAD_CASES, ids=lambda c: "%dx%d_k%d" % c[:3])
def test_every_candidate_displaces_the_head_of_the_list(model, case):
    """tsne_reference.descending_rows: for the rows i > k the first i candidates each go to place 0, so knn_insert shifts
    the whole list -- 16 full steps at k = 1024; at k = 65 one full step and a last step of one entry"""
    n, _, k, _ = case
    assert (k - 1) % 64 == (63 if k == 1024 else 0)
    ridx, _ = _neighbours_equal(model, case)
    assert np.array_equal(ridx[n - 1], n - 2 - np.arange(k))  # the last row: its list is the scan's order reversed


@pytest.mark.parametrize("case", EDGE_CASES, ids=lambda c: "%dx%d_k%d" % c[:3])
def test_neighbours_at_row_load_and_tile_edges(model, case):
    """D on either side of one and two 64-lane passes of the row load; n one short of, equal to and twice the candidate tile"""
    _neighbours_equal(model, case)


@pytest.mark.parametrize("case,perplexity", AFFINITY_CAP_CASES, ids=lambda c: "%dx%d_k%d_%s" % c if isinstance(c, tuple) else str(c))
def test_affinities_at_the_cap(model, case, perplexity):
    """k = 1024: tests/test_tsne_reference.py holds the reference alone to the same conditions on these inputs"""
    from crbm_amd import tsne
    _, _, d2 = knn_reference(case)
    p, beta = tsne.affinities(model, d2, perplexity)
    check_affinities(d2, perplexity, p, beta)


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
    vel = settle(dense_reference(P), y, vel, ex)
    y1, v1, g1 = y.copy(), vel.copy(), gains.copy()
    got = tsne.descend(model, csr, y1, v1, g1, 1, ex, 50.0, 0.5, want_grad=True, want_kl=True)
    got.update(y=y1, velocity=v1, gains=g1)
    share = check_step(got, dense_reference(P), y, vel, gains, ex, 50.0, 0.5)
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


# ---- the descent past one tile per slice and past one pass of the final sum -----------------------------------------------
def _one_step(model, csr, y, vel, gains, ex):
    from crbm_amd import tsne
    y1, v1, g1 = y.copy(), vel.copy(), gains.copy()
    got = tsne.descend(model, csr, y1, v1, g1, 1, ex, 50.0, 0.5, want_grad=True, want_kl=True)
    got.update(y=y1, velocity=v1, gains=g1)
    return got


def _same_bits(a, b):
    for key in ("y", "velocity", "gains", "grad"):
        assert np.array_equal(a[key].view(np.uint32), b[key].view(np.uint32)), key
    assert a["kl"] == b["kl"] and a["z"] == b["z"]


def _large_step(model, n, scale, ex):
    csr, y, vel, gains, ref1 = large_inputs(n, scale)
    assert csr[0][301] == csr[0][300]                         # the empty row
    ref = R.at_exaggeration(ref1, ex)
    vel = settle(ref, y, vel, ex)
    got = _one_step(model, csr, y, vel, gains, ex)
    share = check_step(got, ref, y, vel, gains, ex, 50.0, 0.5)
    print("n = %d, scale %g, exaggeration %g: gradient error as a share of its bound: %.3g" % (n, scale, ex, share))
    return csr, y, vel, gains, got


@pytest.mark.parametrize("scale,ex", [(10.0, 12.0), (10.0, 1.0), (1e-4, 12.0), (1e-4, 1.0)])
def test_one_descent_step_with_three_tiles_per_slice(model, scale, ex):
    """n = 16 385, the first run of tsne_repulsion_kernel's tile loop against a reference: 65 tiles in 22 slices of 3, so
    the block's own tile is the first, second or third of its slice; the last slice has two tiles, the second of one
    point; the last row block has one live row.  Twice: the same bits."""
    n = 16385
    tiles = (n + R.TJ - 1) // R.TJ
    assert tiles == 65 and R.slice_tiles(n) == 3 and R.slices(n) == 22
    assert tiles - 21 * 3 == 2 and n - 64 * R.TJ == 1 and n % 256 == 1 and R.sum_chunks(n) == 65
    csr, y, vel, gains, got = _large_step(model, n, scale, ex)
    _same_bits(got, _one_step(model, csr, y, vel, gains, ex))


def test_iterations_resume_with_three_tiles_per_slice(model):
    """three iterations in one call = one and then two in two calls, bit for bit, at n = 16 385"""
    from crbm_amd import tsne
    n = 16385
    assert R.slice_tiles(n) >= 2
    csr, y, vel, gains, _ = large_inputs(n, 10.0)
    whole = [y.copy(), vel.copy(), gains.copy()]
    w = tsne.descend(model, csr, whole[0], whole[1], whole[2], 3, 12.0, 50.0, 0.5, want_grad=True, want_kl=True)
    parts = [y.copy(), vel.copy(), gains.copy()]
    tsne.descend(model, csr, parts[0], parts[1], parts[2], 1, 12.0, 50.0, 0.5)
    p = tsne.descend(model, csr, parts[0], parts[1], parts[2], 2, 12.0, 50.0, 0.5, want_grad=True, want_kl=True)
    assert np.isfinite(whole[0]).all() and not np.array_equal(whole[0], y)
    for a, b in zip(whole + [w["grad"]], parts + [p["grad"]]):
        assert np.array_equal(a.view(np.uint32), b.view(np.uint32))
    assert w["kl"] == p["kl"] and w["z"] == p["z"]


@pytest.mark.parametrize("n,tiles,per,count", [(16384, 64, 2, 32), (11520, 45, 1, 45), (11521, 46, 2, 23)])
def test_one_descent_step_where_the_tiles_per_slice_change(model, n, tiles, per, count):
    """n = 16 384: 64 whole tiles in 32 slices of two (slice_tiles aims at 2048 blocks, so it leaves one tile per slice
    after 45 tiles, not after 64).  n = 11 520: 45 whole tiles, the last n with one tile per slice.  n = 11 521: the first
    with two, 23 whole slices, the last tile of one point."""
    assert (n + R.TJ - 1) // R.TJ == tiles and R.slice_tiles(n) == per and R.slices(n) == count and per * count == tiles
    assert n % R.TJ == (1 if n == 11521 else 0)
    _large_step(model, n, 10.0, 12.0)


_GROUPED = {}


def grouped_inputs(n):
    """n rows on G = 257 float32 positions at scale 10, assigned at random (every tile mixes groups), so that the float64
    reference is kl_gradient_grouped: exact, and O(G^2) where the blocked one would take minutes"""
    if n not in _GROUPED:
        G = 257
        rng = np.random.default_rng(n)
        points = (10.0 * rng.standard_normal((G, 2))).astype(np.float32)
        group = rng.integers(0, G, size=n)
        assert np.unique(points, axis=0).shape[0] == G and np.unique(group).size == G
        assert min(np.unique(group[t:t + R.TJ]).size for t in range(0, n - 1, R.TJ)) > 100
        csr = R.sparse_joint(n, seed=n, empty_row=300)
        y = np.ascontiguousarray(points[group])
        vel = (rng.standard_normal((n, 2))).astype(np.float32)
        gains = rng.choice(np.array([0.01, 0.5, 1.0, 1.2, 2.4], np.float32), size=(n, 2))
        _GROUPED[n] = dict(csr=csr, y=y, vel=vel, gains=gains, ref=R.kl_gradient_grouped(csr, points, group, 1.0))
    return _GROUPED[n]


@pytest.mark.parametrize("n,chunks,per,count,last", [(65537, 257, 33, 8, 26), (131073, 513, 129, 4, 126)])
def test_descent_with_more_than_256_chunk_sums(model, n, chunks, per, count, last):
    """The first runs of tsne_final_sum_kernel's strided loop past one value per slot, for Z and for the KL, and of slices
    of tens of tiles.  n = 65 537: 257 chunk sums, so slot 0 adds two values; 8 slices of 33 tiles, the last of 26.  That
    257th chunk holds one row, 1.5e-5 of Z and of the KL, which the 1e-4 of check_step does not see (a final sum that
    dropped it was tried in the emulation and passed), so n = 131 073 as well: 513 chunk sums, three values in slot 0
    and two in every other, half of Z behind the first pass; 4 slices of 129 tiles, the last of 126.  One evaluation
    (iterations = 0) and one step against kl_gradient_grouped at the bounds of check_step; the step twice: the same bits."""
    from crbm_amd import tsne
    tiles = (n + R.TJ - 1) // R.TJ
    assert R.sum_chunks(n) == chunks > R.SUM_CHUNK and R.slice_tiles(n) == per and R.slices(n) == count
    assert tiles - (count - 1) * per == last and n % R.TJ == 1
    g = grouped_inputs(n)
    csr, y, gains = g["csr"], g["y"], g["gains"]
    for ex in (12.0, 1.0):
        ref = R.at_exaggeration(g["ref"], ex)
        y0, v0, g0 = y.copy(), g["vel"].copy(), gains.copy()
        at = tsne.descend(model, csr, y0, v0, g0, 0, ex, 50.0, 0.5, want_grad=True, want_kl=True)
        assert np.array_equal(y0, y) and np.array_equal(v0, g["vel"]) and np.array_equal(g0, gains)       # nothing moved
        err, bound = np.abs(at["grad"] - ref["grad"]).max(), grad_bound(ref, ex)
        print("n = %d, exaggeration %g: gradient error as a share of its bound: %.3g" % (n, ex, err / bound))
        assert err <= bound
        assert abs(at["z"] - ref["z"]) <= 1e-4 * ref["z"] and abs(at["kl"] - ref["kl"]) <= 1e-4 * abs(ref["kl"])
    ref = R.at_exaggeration(g["ref"], 12.0)
    vel = settle(ref, y, g["vel"], 12.0)
    got = _one_step(model, csr, y, vel, gains, 12.0)
    check_step(got, ref, y, vel, gains, 12.0, 50.0, 0.5)
    _same_bits(got, _one_step(model, csr, y, vel, gains, 12.0))


def test_end_to_end_at_the_largest_k(model):
    """tsneEmbed with k = 1024: the four stages together at the cap of the neighbour list.  The library's last KL against
    the float64 reference at the returned y (its own neighbours, affinities and P); a second call: the same bits.  No
    cluster purity: whether the float64 reference separates this set at that perplexity has not been measured."""
    from crbm_amd import tsneEmbed
    X, _ = R.planted(1500, 10, 0)
    y, info = tsneEmbed(model, X, perplexity=341.5, max_iter=300, init="random", seed=0, return_info=True)
    assert info["k"] == 1024 and y.shape == (1500, 2) and y.dtype == np.float32 and np.isfinite(y).all()
    idx, d2 = R.neighbors(X, 1024)
    csr = R.dense_to_csr(R.symmetrize_dense(idx, R.affinities(d2, 341.5)[1]))
    kl = R.kl_gradient_csr(csr, y.astype(np.float64))["kl"]
    print("KL of the returned y by the reference: %.5f (the library's own: %.5f)" % (kl, info["kl"][-1][1]))
    assert info["kl"][-1][0] == 300 and abs(info["kl"][-1][1] - kl) <= 1e-3 * kl
    again = tsneEmbed(model, X, perplexity=341.5, max_iter=300, init="random", seed=0)
    assert np.array_equal(again.view(np.uint32), y.view(np.uint32))
