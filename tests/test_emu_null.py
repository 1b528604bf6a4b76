"""The analytic-null kernels (crbm_amd/csrc/crbm_null.h) on CPU threads under AddressSanitizer + UBSan:
tests/emu/null_main.cpp, a stand-alone program built here and run directly (no preloaded runtime).  The pmf agrees with
the scatter programme of tests/null_reference.py within the rounding of the two summation orders, cells the reference
holds at exactly 0 are exactly 0, and tile lengths, row groups, block sizes and both kernel variants give the same bits;
the header's predecessor table is next_context's inverse; what the entry point refuses is refused (the checks are the
header's); guard words around every output must be intact, every buffer and the LDS are sized to the byte, and the state
buffers start out as garbage (nothing relies on a cleared buffer)."""
import os
import subprocess

import numpy as np
import pytest

from tests import null_reference as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GUARD, GUARD_WORD = 8, 0xA5A5BEEF
GIB = 1 << 30


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    path = str(tmp_path_factory.mktemp("emu_null") / "null_main")
    emu = os.path.join(ROOT, "tests", "emu")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g1", "-fsanitize=address,undefined", "-fno-omit-frame-pointer",
                           "-fno-sanitize-recover=undefined", "-ffp-contract=off", "-mf16c", "-I", os.path.join(emu, "shim"),
                           "-I", emu, "-I", os.path.join(ROOT, "crbm_amd", "csrc"), os.path.join(emu, "null_main.cpp"),
                           "-o", path, "-lpthread"])
    return path


def run(exe, tmp_path, q, order, trans, init, G=None, op=0, variant=0, threads=4, budget=GIB, tile=64, refused=None, R_=None, M_=None):
    q = np.ascontiguousarray(q, np.int32)
    Rn, M = (q.shape[0], q.shape[1]) if R_ is None else (R_, M_)
    if G is None:
        G = int(q.max(axis=2).sum(axis=1).max()) + 1
    fin, fout = str(tmp_path / "in.bin"), str(tmp_path / "out.bin")
    if os.path.exists(fout):
        os.unlink(fout)
    with open(fin, "wb") as f:
        f.write(np.array([op, Rn, M, order, variant, threads, 0, 0], np.int32).tobytes())
        f.write(np.array([G, budget, tile, 0], np.int64).tobytes())
        f.write(q.tobytes())
        f.write(np.ascontiguousarray(trans, np.float64).tobytes())
        f.write(np.ascontiguousarray(init, np.float64).tobytes())
    r = subprocess.run([exe, fin, fout], capture_output=True, text=True, timeout=600)      # the inherited environment, as it is
    if refused is not None:
        assert r.returncode == 3 and refused in r.stderr, (r.returncode, r.stderr[-2000:])
        assert not os.path.exists(fout)                          # nothing was written
        return None
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    raw = np.fromfile(fout, np.uint8)
    count = Rn * G if op == 0 else R.contexts(order) * 5 * 3
    assert raw.size == 8 * GUARD + 8 * count
    guards = np.concatenate([raw[:4 * GUARD], raw[4 * GUARD + 8 * count:]]).view(np.uint32)
    assert np.all(guards == GUARD_WORD), "a guard word was written"
    out = raw[4 * GUARD:4 * GUARD + 8 * count].copy().view(np.float64)
    return out.reshape(Rn, G) if op == 0 else out.reshape(R.contexts(order), 5, 3)


def rows_of(Rn, M, seed, spread=40):
    """integer weights with min 0 per position; one position of row 0 whose four weights are equal (zero shift)"""
    rng = np.random.default_rng(seed)
    q = rng.integers(0, spread, size=(Rn, M, 4))
    q[1:] = q[1:] // np.arange(2, Rn + 1)[:, None, None]          # rows of different G_r
    q -= q.min(axis=2, keepdims=True)
    q[0, M // 2] = 0
    return q.astype(np.int32)


def check(pmf, q, P, init, order):
    """the device contract of tests/test_gpu_null.py: relative (8 M + 128) 2^-53 above 1e-280, exact zeros, the total"""
    M = q.shape[1]
    bound = (8 * M + 128) * 2.0 ** -53
    for r in range(q.shape[0]):
        want = R.dp(q[r], P, init, order)
        got = pmf[r]
        assert np.all(got[want.size:] == 0.0)
        got = got[:want.size]
        assert np.all(got[want == 0.0] == 0.0)
        big = want > 1e-280
        assert np.all(np.abs(got[big] - want[big]) <= bound * want[big]), float((np.abs(got[big] - want[big]) / want[big]).max() / bound)
        assert abs(got.sum() - init.sum()) <= bound * max(init.sum(), 1.0)


@pytest.mark.parametrize("order", [0, 1, 2, 3])
def test_table_is_the_inverse_of_next_context(exe, tmp_path, order):
    P = R.dirichlet_probabilities(order, order)
    table = run(exe, tmp_path, np.zeros((1, 1, 4)), order, P, np.ones(R.contexts(order)), op=1)
    pairs = set()
    for t in range(R.contexts(order)):
        used = [(int(s), int(a)) for s, a, p in table[t] if p != 0.0]
        assert used == sorted(used) and all(p == 0.0 for _, _, p in table[t][len(used):])     # a fixed order, unused slots behind
        for s, a in used:
            assert R.next_context(order, s, a) == t and table[t][used.index((s, a))][2] == P[s, a]
        pairs |= {(s, a) for s, a in used}
    assert pairs == {(s, a) for s in range(R.contexts(order)) for a in range(4)}              # every pair, once
    base = (4 ** order - 1) // 3
    for t0 in range(base, R.contexts(order), 4) if order else []:                             # siblings: the same sources, letter a
        for a in range(4):
            assert np.array_equal(table[t0 + a][:, 0], table[t0][:, 0]) and np.all(table[t0 + a][:, 1] == a)


@pytest.mark.parametrize("order", [0, 1, 2, 3])
def test_pmf_against_the_reference_and_the_same_bits_everywhere(exe, tmp_path, order):
    M = 3 if order == 3 else 4                                   # (order 3: M below order + 1)
    q = rows_of(3, M, seed=order, spread=(40, 40, 20, 16)[order])        # (the wide orders on short scores: a lane is an OS thread)
    assert q.max() > 8                                           # a shift and a halo longer than the shortest tile
    P = R.dirichlet_probabilities(order, 10 + order)
    rng = np.random.default_rng(order)
    for init in (R.start(P, order, "stationary"), R.start(P, order, "run"), rng.dirichlet(np.ones(R.contexts(order)))):
        base = run(exe, tmp_path, q, order, P, init, tile=64)
        check(base, q, P, init, order)
        assert np.array_equal(run(exe, tmp_path, q, order, P, init, tile=64, variant=1), base)
    G = base.shape[1]
    per_row = 2 * R.contexts(order) * G * 8
    for kw in (dict(tile=8, variant=0), dict(tile=8, variant=1),                   # shifts longer than a tile; halos longer than a tile
               dict(tile=37, threads=64, variant=1), dict(tile=1024, threads=32, variant=1),
               dict(tile=64, budget=per_row), dict(tile=64, budget=2 * per_row + 5, variant=1),      # one row per group; two groups, the last partial
               dict(tile=16, G=G + 11)):                                           # G beyond every row: zeros behind
        other = run(exe, tmp_path, q, order, P, init, **kw)
        assert np.array_equal(other[:, :G], base) and np.all(other[:, G:] == 0.0), kw


def test_single_row_and_short_motifs(exe, tmp_path):
    for order, M in ((3, 1), (3, 2), (2, 1), (1, 7)):
        q = rows_of(1, M, seed=9 + M, spread=25)
        P = R.dirichlet_probabilities(order, 5)
        for kind in ("stationary", "run"):
            init = R.start(P, order, kind)
            got = run(exe, tmp_path, q, order, P, init, tile=16, variant=1)
            check(got, q, P, init, order)
            assert np.array_equal(run(exe, tmp_path, q, order, P, init, tile=256), got)


def test_zero_probabilities_give_exact_zeros(exe, tmp_path):
    """a chain that never draws C or G: every score that needs one is exactly 0"""
    P = np.tile([0.5, 0.0, 0.0, 0.5], (R.contexts(2), 1))
    q = rows_of(2, 5, seed=3)
    init = R.start(P, 2, "run")
    for variant in (0, 1):
        got = run(exe, tmp_path, q, 2, P, init, tile=16, variant=variant)
        check(got, q, P, init, 2)
        uniform = R.dp(q[0], np.full_like(P, 0.25), init, 2)
        assert (got[0, :uniform.size] == 0.0).sum() > (uniform == 0.0).sum()


def test_refusals(exe, tmp_path):
    P = R.dirichlet_probabilities(1, 0)
    init = R.start(P, 1, "run")
    q = rows_of(2, 3, seed=1)
    ok = dict(order=1, trans=P, init=init)
    run(exe, tmp_path, q, refused="R must be at least 1", R_=0, M_=3, **ok)
    for M in (0, 513):
        run(exe, tmp_path, q, refused="M must lie in [1, 512]", R_=2, M_=M, G=10, **ok)
    for order in (-1, 4):
        run(exe, tmp_path, q, order, P, init, refused="order must lie in [0, 3]")
    bad = q.copy()
    bad[1, 2, 3] = -1
    run(exe, tmp_path, bad, G=200, refused="must not be negative", **ok)
    bad = q.copy()
    bad[1, 2] += 1
    run(exe, tmp_path, bad, refused="smallest q of every position must be 0", **ok)
    G = int(q.max(axis=2).sum(axis=1).max()) + 1
    run(exe, tmp_path, q, G=G - 1, refused="at least the largest G_r", **ok)
    run(exe, tmp_path, q, G=-1, refused="at least the largest G_r", **ok)
    huge = q.copy()
    huge[0, 0] = [0, 2 ** 24, 0, 0]
    run(exe, tmp_path, huge, G=1000, refused="at most 2^24", **ok)
    for value in (-0.1, np.nan, np.inf):
        T = P.copy()
        T[3, 1] = value
        run(exe, tmp_path, q, 1, T, init, refused="negative or not finite")
        i = init.copy()
        i[2] = value
        run(exe, tmp_path, q, 1, P, i, refused="negative or not finite")
    T = P.copy()
    T[2, 0] += 1e-8
    run(exe, tmp_path, q, 1, T, init, refused="does not sum to 1")
    T[2, 0] = P[2, 0] + 1e-11                                    # within 1e-9: served
    assert run(exe, tmp_path, q, 1, T, init) is not None
    run(exe, tmp_path, q, budget=2 * 5 * G * 8 - 1, refused="CRBM_NULL_BYTES: use a larger step", **ok)
    assert run(exe, tmp_path, q, budget=2 * 5 * G * 8, **ok) is not None
