"""The t-SNE kernels (crbm_amd/csrc/crbm_tsne.h) on CPU threads under AddressSanitizer + UBSan: tests/emu/tsne_main.cpp,
a stand-alone program built here and run directly (no preloaded runtime).  Neighbours equal tests/tsne_reference.py bit for
bit; affinities and one descent step are held to it at the tolerances of tests/test_gpu_tsne.py; several grid and block
sizes give the same bits; what the entry points refuse is refused (the checks are the header's); guard words around
every output must be intact.  The edges of the row load, the candidate tile and the list's shift, and one descent step
with three tiles per slice (n = 16 385), run here with the LDS and every buffer sized to the byte."""
import os
import subprocess

import numpy as np
import pytest

from tests import tsne_reference as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GUARD, GUARD_WORD = 8, 0xA5A5BEEF


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    path = str(tmp_path_factory.mktemp("emu_tsne") / "tsne_main")
    emu = os.path.join(ROOT, "tests", "emu")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g1", "-fsanitize=address,undefined", "-fno-omit-frame-pointer",
                           "-fno-sanitize-recover=undefined", "-ffp-contract=off", "-mf16c", "-I", os.path.join(emu, "shim"),
                           "-I", emu, "-I", os.path.join(ROOT, "crbm_amd", "csrc"), os.path.join(emu, "tsne_main.cpp"), "-o", path,
                           "-lpthread"])
    return path


def _run(exe, tmp_path, header, payload, outputs, refused=None):
    """runs one case; `outputs`: (dtype, count) per output array, returned with their guard words checked"""
    fin, fout = str(tmp_path / "in.bin"), str(tmp_path / "out.bin")
    with open(fin, "wb") as f:
        f.write(np.array(list(header) + [0] * (8 - len(header)), np.int32).tobytes())
        for a in payload:
            f.write(np.ascontiguousarray(a).tobytes())
    r = subprocess.run([exe, fin, fout], capture_output=True, text=True, timeout=900)      # the inherited environment, as it is
    if refused is not None:
        assert r.returncode == 3 and refused in r.stderr, (r.returncode, r.stderr[-2000:])
        return None
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    words = np.fromfile(fout, np.uint32)
    got, at = [], 0
    for dtype, count in outputs:
        size = count * np.dtype(dtype).itemsize // 4
        assert np.all(words[at:at + GUARD] == GUARD_WORD) and np.all(words[at + GUARD + size:at + 2 * GUARD + size] == GUARD_WORD), "a guard word was written"
        got.append(words[at + GUARD:at + GUARD + size].view(dtype))
        at += 2 * GUARD + size
    assert at == words.size
    return got


def knn(exe, tmp_path, X, k, grid=2, threads=128, **kw):
    n, D = X.shape
    out = _run(exe, tmp_path, [0, n, D, k, grid, threads], [X.astype(np.float32)], [(np.int32, n * k), (np.float32, n * k)], **kw)
    return None if out is None else (out[0].reshape(n, k), out[1].reshape(n, k))


def affinity(exe, tmp_path, d2, perplexity, grid=2, threads=64, **kw):
    n, k = d2.shape
    out = _run(exe, tmp_path, [1, n, 0, k, grid, threads], [np.float32(perplexity), d2.astype(np.float32)],
               [(np.float32, n * k), (np.float32, n)], **kw)
    return None if out is None else (out[0].reshape(n, k), out[1])


def descend(exe, tmp_path, csr, y, vel, gains, iterations, ex, lr, mom, grid=2, threads=128, **kw):
    n = y.shape[0]
    indptr, indices, values = csr
    out = _run(exe, tmp_path, [2, n, iterations, 0, grid, threads, 3],
               [np.array([ex, lr, mom], np.float32), np.asarray(indptr, np.int64), np.asarray(indices, np.int32),
                np.asarray(values, np.float32), y.astype(np.float32), vel.astype(np.float32), gains.astype(np.float32)],
               [(np.float32, 2 * n)] * 5 + [(np.float64, 2)], **kw)
    if out is None:
        return None
    y1, _, v1, g1, grad, scal = out
    return {"y": y1.reshape(n, 2), "velocity": v1.reshape(n, 2), "gains": g1.reshape(n, 2), "grad": grad.reshape(n, 2),
            "kl": scal[1], "z": scal[0]}


@pytest.mark.parametrize("n,D,k,eighths", [(2, 1, 1, False), (65, 1, 64, True), (257, 10, 90, False), (70, 3, 69, False),
                                           (70, 67, 11, False)])
def test_neighbours_equal_the_reference_bit_for_bit(exe, tmp_path, n, D, k, eighths):
    X = R.feature_rows(n, D, seed=n + D, eighths=eighths)
    idx, d2 = knn(exe, tmp_path, X, k)
    ridx, rd2 = R.neighbors(X, k)
    assert np.array_equal(idx, ridx) and np.array_equal(d2.view(np.uint32), rd2.view(np.uint32))
    if n == 65:                                              # other grids and block sizes: the same bits
        for grid, threads in ((1, 64), (3, 256), (5, 512)):
            other = knn(exe, tmp_path, X, k, grid=grid, threads=threads)
            assert np.array_equal(other[0], idx) and np.array_equal(other[1].view(np.uint32), d2.view(np.uint32)), (grid, threads)


EDGE_SHAPES = [(130, D, 65) for D in (64, 65, 128, 129)] + [(n, 3, n - 1) for n in (63, 64, 128)]
LIMIT_CASES = [(n, D, k, False, grid, threads) for n, D, k in EDGE_SHAPES for grid, threads in ((2, 128), (3, 512))] + [
    (70, 256, 11, False, 2, 128), (70, 255, 69, False, 3, 512),             # the longest row; odd D: the stride equals D
    (140, 2, 135, False, 2, 128), (140, 2, 135, False, 3, 512),             # three shift steps, the last of six entries
    (140, 1, 130, "descending", 3, 512), (200, 1, 65, "descending", 2, 128)]  # every candidate shifts the whole list


@pytest.mark.parametrize("n,D,k,data,grid,threads", LIMIT_CASES)
def test_neighbours_at_the_edges_of_the_row_load_the_tile_and_the_shift(exe, tmp_path, n, D, k, data, grid, threads):
    """The emulator sizes the LDS to the byte, so here an overrun of the row load (D on either side of one and two
    64-lane passes, D = 256 and 255), of the candidate tile (n = 63, 64, 128) or of knn_insert's shift (k = 65: a last
    step of one entry; k above 128) shows; two and eight waves per block.

    Times on the CPU machine (8 cores): the slowest case of this file before these was [257-10-90-False] at 28 s; the
    slowest new ones are (200, 1, 65, descending) at 14 s, (140, *, 13x) at 12 to 13 s and (128, 3, 127) at 10 s, the
    others 2 to 7 s.

    k near 1024 is not affordable here: every shift step of knn_insert is two emulated wave barriers, each a pthread
    barrier of 64 OS threads, about 0.25 ms a step.  On descending rows (n, k) = (130, 65), (140, 130), (280, 260) took
    6.5, 13 and 76 s for about 26, 50 and 350 thousand steps: linear in the steps, so the emulator is slow there, not
    stalled.  (1100, 256, 1024) is some 10^7 steps, most of an hour.  tests/test_gpu_tsne.py is the only cover of k
    above 135 and of the four-wave launch."""
    X = R.descending_rows(n) if data == "descending" else R.feature_rows(n, D, seed=n + D, eighths=data)
    idx, d2 = knn(exe, tmp_path, X, k, grid=grid, threads=threads)
    ridx, rd2 = R.neighbors(X, k)
    assert np.array_equal(idx, ridx) and np.array_equal(d2.view(np.uint32), rd2.view(np.uint32))


def check_affinities(d2, perplexity, p, beta):
    """the three conditions of the affinity kernel, shared with tests/test_gpu_tsne.py"""
    k = d2.shape[1]
    assert np.isfinite(beta).all() and (beta > 0).all() and np.isfinite(p).all()
    ok = R.reachable(d2, perplexity)
    H = R.entropy(d2[ok], beta[ok])
    assert np.abs(H - np.log(perplexity)).max() < 1e-4                                   # (i)
    want = R.conditional(d2, beta)
    assert np.all(np.abs(p - want) <= k * 2.0 ** -23 * want.max(axis=1, keepdims=True))  # (ii)
    equal = (d2 == d2[:, :1]).all(axis=1)
    assert np.all(p[equal] == np.float32(1.0 / k))                                       # (iii)
    # a row that cannot reach the entropy (tsne_reference.reachable): p is uniform over those tied for the smallest d2
    tied = d2 == d2.min(axis=1, keepdims=True)
    stuck = tied.sum(axis=1) >= perplexity
    # (m = perplexity is reached only in the limit: beta stops where float64 no longer tells, the others at e^-40 or so)
    assert np.abs(p - tied / tied.sum(axis=1, keepdims=True))[stuck].max(initial=0.0) <= 1e-6
    return int(equal.sum()), int(stuck.sum())


def test_affinities(exe, tmp_path):
    X = R.feature_rows(257, 10, seed=267)
    for k, perplexity, equal_rows in ((90, 30.0, 0), (90, 5.0, 0), (11, 5.0, 12)):
        _, d2 = R.neighbors(X, k)
        p, beta = affinity(exe, tmp_path, d2, perplexity)
        equal = check_affinities(d2, perplexity, p, beta)[0]
        assert equal >= equal_rows and (equal_rows or not equal)      # the twelve copies, and rows whose nearest they are
        for grid, threads in ((1, 128), (5, 64)):
            other = affinity(exe, tmp_path, d2, perplexity, grid=grid, threads=threads)
            assert np.array_equal(other[0].view(np.uint32), p.view(np.uint32)) and np.array_equal(other[1], beta)
    _, d2 = R.neighbors(R.feature_rows(65, 1, seed=66, eighths=True), 64)                # ties everywhere
    p, beta = affinity(exe, tmp_path, d2, 30.0)
    check_affinities(d2, 30.0, p, beta)


_JOINT = {}


def joint(n, seed, k):
    """the reference's dense P of n feature rows at k neighbours, computed once"""
    if (n, seed, k) not in _JOINT:
        idx, d2 = R.neighbors(R.feature_rows(n, 10, seed=seed + 1, duplicates=0), k)
        _JOINT[n, seed, k] = R.symmetrize_dense(idx, R.affinities(d2, min(30.0, k / 3.0 + 0.5))[1])
    return _JOINT[n, seed, k]


def step_inputs(n, scale, seed, k=None, empty_row=False):
    """P (CSR, float32 values, and dense float64 of those values), y at `scale`, a non-trivial velocity and gains"""
    rng = np.random.default_rng(seed)
    P = joint(n, seed, n - 1 if k is None else min(k, n - 1)).copy()
    if empty_row:
        P[7, :] = 0.0
        P[:, 7] = 0.0
        P /= P.sum()
    indptr, indices, values = R.dense_to_csr(P)
    values = values.astype(np.float32)
    y = (scale * rng.standard_normal((n, 2))).astype(np.float32)
    vel = (scale * 0.1 * rng.standard_normal((n, 2))).astype(np.float32)
    gains = rng.choice(np.array([0.01, 0.5, 1.0, 1.2, 2.4], np.float32), size=(n, 2))
    return (indptr, indices, values), R.csr_to_dense(n, indptr, indices, values.astype(np.float64)), y, vel, gains


_LARGE = {}


def large_inputs(n, scale):
    """sparse P with an empty row, distinct random y at `scale`, velocity and gains as in step_inputs, and the float64
    reference at exaggeration 1 (blocked, some seconds at n = 16 385) -- computed once and never written to"""
    if (n, scale) not in _LARGE:
        rng = np.random.default_rng(n + (scale > 1.0))
        csr = R.sparse_joint(n, seed=n, empty_row=300)
        y = (scale * rng.standard_normal((n, 2))).astype(np.float32)
        assert np.unique(y, axis=0).shape[0] == n
        vel = (scale * 0.1 * rng.standard_normal((n, 2))).astype(np.float32)
        gains = rng.choice(np.array([0.01, 0.5, 1.0, 1.2, 2.4], np.float32), size=(n, 2))
        _LARGE[n, scale] = (csr, y, vel, gains, R.kl_gradient_csr(csr, y, 1.0))
    return _LARGE[n, scale]


def grad_bound(ref, ex):
    """1e-4 of the largest 4 exaggeration |A_i| + 4 |R_i| / Z: the two terms of the gradient cancel, and it carries their rounding"""
    return 1e-4 * (4.0 * ex * np.abs(ref["A"]) + 4.0 * np.abs(ref["R"]) / ref["z"]).max()


def reference_at(ref, y, ex):
    """`ref`: the dict of tsne_reference.kl_gradient (or _csr, _grouped) at y and ex, or a callable (y float64, ex) that gives it"""
    return ref(y.astype(np.float64), ex) if callable(ref) else ref


def dense_reference(P):
    return lambda y, ex: R.kl_gradient(P, y, ex)


def settle(ref, y, vel, ex):
    """the velocity with an exact zero wherever the reference's gradient is within four bounds of zero: there the sign of
    velocity * g would hang on the gradient's rounding; a zero product is no such decision (0 < 0 is false whatever g is)"""
    ref = reference_at(ref, y, ex)
    out = vel.copy()
    out[np.abs(ref["grad"]) <= 4.0 * grad_bound(ref, ex)] = 0.0
    assert (out != 0).mean() > 0.9
    return out


def check_step(got, ref, y, vel, gains, ex, lr, mom):
    """one step against the reference at the tolerances of the issue; returns the gradient's error as a share of its bound"""
    ref = reference_at(ref, y, ex)
    bound = grad_bound(ref, ex)
    err = np.abs(got["grad"] - ref["grad"]).max()
    assert err <= bound, (err, bound)
    assert abs(got["z"] - ref["z"]) <= 1e-4 * ref["z"] and abs(got["kl"] - ref["kl"]) <= 1e-4 * abs(ref["kl"])
    # a velocity * g product within the gradient's tolerance of zero is a sign decision that rounding may flip: the
    # inputs must have none, so that gains can be compared exactly
    v64 = vel.astype(np.float64)
    assert np.all((v64 == 0.0) | (np.abs(ref["grad"]) > bound)), "an input whose gain decision hangs on rounding"
    y1, v1, g1 = R.update(y.astype(np.float64), v64, gains.astype(np.float64), ref["grad"], lr, mom)
    # exactly: the reference's decisions, the kernel's float32 arithmetic on them
    g32 = np.maximum(np.where(v64 * ref["grad"] < 0.0, gains + np.float32(0.2), gains * np.float32(0.8)), np.float32(0.01))
    assert g32.dtype == np.float32 and np.array_equal(got["gains"], g32) and np.allclose(g32, g1, rtol=1e-6, atol=0)
    # 1e-4 relative: of the array's largest entry (a component near zero has no scale of its own)
    assert np.abs(got["velocity"] - v1).max() <= 1e-4 * np.abs(v1).max()
    assert np.abs(got["y"] - y1).max() <= 1e-4 * np.abs(y1).max()
    return err / bound


@pytest.mark.parametrize("n,k,scale,ex", [(2, None, 1e-4, 12.0), (2, None, 10.0, 12.0), (65, None, 10.0, 12.0),
                                          (257, 90, 1e-4, 12.0), (257, 90, 10.0, 1.0), (300, None, 10.0, 1.0)])
def test_one_descent_step(exe, tmp_path, n, k, scale, ex):
    csr, P, y, vel, gains = step_inputs(n, scale, seed=n, k=k, empty_row=(n == 257 and ex == 1.0))
    if k is not None:
        assert np.unique(np.diff(csr[0])).size > 1                                   # rows of unequal length
    vel = settle(dense_reference(P), y, vel, ex)
    got = descend(exe, tmp_path, csr, y, vel, gains, 1, ex, 50.0, 0.5)
    check_step(got, dense_reference(P), y, vel, gains, ex, 50.0, 0.5)
    if n == 257:
        for grid, threads in ((1, 64), (5, 256), (3, 512)):
            other = descend(exe, tmp_path, csr, y, vel, gains, 1, ex, 50.0, 0.5, grid=grid, threads=threads)
            for key in ("y", "velocity", "gains", "grad"):
                assert np.array_equal(other[key].view(np.uint32), got[key].view(np.uint32)), (key, grid, threads)
            assert other["kl"] == got["kl"] and other["z"] == got["z"]


@pytest.mark.parametrize("grid,threads", [(2, 256), (3, 128)])
def test_one_descent_step_with_three_tiles_per_slice(exe, tmp_path, grid, threads):
    """n = 16 385 (tests/test_gpu_tsne.py has the shape's facts): the tile loop of tsne_repulsion_kernel, the short last
    slice and the one-point last tile with every buffer sized exactly; with 128 threads a block's rows are half a tile,
    and the grid-stride loops over row blocks and chunks run many times.  Both geometries: the same bits.
    Times on the CPU machine: 9 s a run and 8 s once for the reference, against 28 s for the file's slowest case."""
    n = 16385
    assert R.slice_tiles(n) == 3 and R.slices(n) == 22 and n % R.TJ == 1
    csr, y, vel, gains, ref1 = large_inputs(n, 10.0)
    ref = R.at_exaggeration(ref1, 12.0)
    vel = settle(ref, y, vel, 12.0)
    got = descend(exe, tmp_path, csr, y, vel, gains, 1, 12.0, 50.0, 0.5, grid=grid, threads=threads)
    check_step(got, ref, y, vel, gains, 12.0, 50.0, 0.5)
    key = tuple(got[name].tobytes() for name in ("y", "velocity", "gains", "grad")) + (got["kl"], got["z"])
    assert _LARGE.setdefault("bits", key) == key


def test_iterations_resume_and_evaluate(exe, tmp_path):
    """three iterations in one call = one and two in two calls, bit for bit; iterations = 0 moves nothing and returns the
    gradient, KL and Z at y"""
    csr, P, y, vel, gains = step_inputs(257, 1.0, seed=5, k=30)
    whole = descend(exe, tmp_path, csr, y, vel, gains, 3, 4.0, 20.0, 0.8)
    a = descend(exe, tmp_path, csr, y, vel, gains, 1, 4.0, 20.0, 0.8)
    b = descend(exe, tmp_path, csr, a["y"], a["velocity"], a["gains"], 2, 4.0, 20.0, 0.8, grid=3, threads=64)
    for key in ("y", "velocity", "gains", "grad"):
        assert np.array_equal(whole[key].view(np.uint32), b[key].view(np.uint32)), key
    assert whole["kl"] == b["kl"] and whole["z"] == b["z"]
    at = descend(exe, tmp_path, csr, b["y"], b["velocity"], b["gains"], 0, 1.0, 20.0, 0.8)
    assert np.array_equal(at["y"], b["y"]) and np.array_equal(at["gains"], b["gains"])
    ref = R.kl_gradient(P, b["y"].astype(np.float64))
    assert abs(at["kl"] - ref["kl"]) <= 1e-4 * abs(ref["kl"]) and abs(at["z"] - ref["z"]) <= 1e-4 * ref["z"]


def test_refusals(exe, tmp_path):
    X = R.feature_rows(20, 3, seed=1)
    knn(exe, tmp_path, X[:1], 1, refused="at least two rows")
    knn(exe, tmp_path, X, 0, refused="[1, n - 1]")
    knn(exe, tmp_path, X, 20, refused="[1, n - 1]")
    _run(exe, tmp_path, [0, 20, 0, 3, 1, 64], [X], [], refused="D must be at least 1")
    _run(exe, tmp_path, [0, 20, 257, 3, 1, 64], [X], [], refused="D above 256")
    _run(exe, tmp_path, [0, 2000, 3, 1025, 1, 64], [X], [], refused="k above 1024")
    d2 = R.neighbors(X, 6)[1]
    for bad in (0.0, -1.0, 7.0, np.inf, np.nan):
        affinity(exe, tmp_path, d2, bad, refused="perplexity")
    affinity(exe, tmp_path, d2[:1], 1.0, refused="at least two rows")
    csr, _, y, vel, gains = step_inputs(20, 1.0, seed=2, k=5)
    indptr, indices, values = csr
    descend(exe, tmp_path, csr, y, vel, gains, -1, 1.0, 1.0, 0.5, refused="iterations")
    descend(exe, tmp_path, (indptr + (np.arange(21) == 0), indices, values), y, vel, gains, 1, 1.0, 1.0, 0.5, refused="start at 0")
    swapped = indptr.copy()
    swapped[3], swapped[4] = indptr[4] + 1, indptr[3]
    descend(exe, tmp_path, (swapped, indices, values), y, vel, gains, 1, 1.0, 1.0, 0.5, refused="ascend")
    for bad in (-1, 20):
        wrong = indices.copy()
        wrong[-1] = bad
        descend(exe, tmp_path, (indptr, wrong, values), y, vel, gains, 1, 1.0, 1.0, 0.5, refused="outside [0, n)")
