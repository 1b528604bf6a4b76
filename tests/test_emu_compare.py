"""The motif comparison kernels (crbm_amd/csrc/crbm_compare.h) on CPU threads under AddressSanitizer + UBSan:
tests/emu/compare_main.cpp, a stand-alone program built here and run directly (no preloaded runtime).  Counts, tails and
all five outputs have the bits of tests/compare_reference.py; thread counts, target tiles and query groups give the same
bits; what the entry points refuse is refused (the checks are the header's); guard words around every output must be
intact, every buffer and the LDS are sized to the byte, and the device buffers start out as garbage (only what the
driver clears is cleared)."""
import os
import subprocess

import numpy as np
import pytest

from tests import compare_reference as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GUARD, GUARD_WORD = 8, 0xA5A5BEEF
GIB = 1 << 30
OUTPUTS = (("p_min", np.float64), ("offset", np.int32), ("strand", np.int8), ("overlap", np.int32), ("n_off", np.int32))


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    path = str(tmp_path_factory.mktemp("emu_compare") / "compare_main")
    emu = os.path.join(ROOT, "tests", "emu")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g1", "-fsanitize=address,undefined", "-fno-omit-frame-pointer",
                           "-fno-sanitize-recover=undefined", "-ffp-contract=off", "-mf16c", "-I", os.path.join(emu, "shim"),
                           "-I", emu, "-I", os.path.join(ROOT, "crbm_amd", "csrc"), os.path.join(emu, "compare_main.cpp"),
                           "-o", path, "-lpthread"])
    return path


def pack(motifs):
    """quantised motifs -> (cols (total, 4) uint16, start (n + 1) int32)"""
    if not motifs:
        return np.zeros((0, 4), np.uint16), np.zeros(1, np.int32)
    start = np.concatenate([[0], np.cumsum([len(m) for m in motifs])]).astype(np.int32)
    return np.ascontiguousarray(np.concatenate(motifs, axis=0), np.uint16), start


def table_elems(B, m):
    return sum((m - l + 1) * (l * (B - 1) + 2) for l in range(1, m + 1))


def run(exe, tmp_path, queries, targets, bins=7, both=1, min_overlap=1, op=0, threads=8, tile=32, budget=GIB, refused=None,
        K=None, N=None, qstart=None, tstart=None, qcols=None, tcols=None, invC=None, null_mask=0):
    qc, qs = pack(queries)
    tc, ts = pack(targets)
    qc, qs = (qc if qcols is None else qcols), (qs if qstart is None else np.asarray(qstart, np.int32))
    tc, ts = (tc if tcols is None else tcols), (ts if tstart is None else np.asarray(tstart, np.int32))
    K = len(queries) if K is None else K
    N = len(targets) if N is None else N
    if invC is None:
        invC = 1.0 / (len(tc) * (2 if both else 1))
    fin, fout = str(tmp_path / "in.bin"), str(tmp_path / "out.bin")
    if os.path.exists(fout):
        os.unlink(fout)
    with open(fin, "wb") as f:
        f.write(np.array([op, K, N, bins, both, min_overlap, threads, tile, null_mask, len(qs), len(ts), 0], np.int32).tobytes())
        f.write(np.array([budget, len(qc), len(tc), 0], np.int64).tobytes())
        f.write(np.array([invC], np.float64).tobytes())
        f.write(qs.tobytes() + ts.tobytes() + np.ascontiguousarray(qc, np.uint16).tobytes() + np.ascontiguousarray(tc, np.uint16).tobytes())
    r = subprocess.run([exe, fin, fout], capture_output=True, text=True, timeout=600)      # the inherited environment, as it is
    if refused is not None:
        assert r.returncode == 3 and refused in r.stderr, (r.returncode, r.stderr[-2000:])
        assert not os.path.exists(fout)                          # nothing was written
        return None
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    raw = np.fromfile(fout, np.uint8)
    if op == 0:
        parts = [(name, dtype, K * N) for name, dtype in OUTPUTS]
    else:
        m = int(qs[1])
        parts = [("counts", np.uint32, m * bins), ("tail", np.float64, table_elems(bins, m))]
    out, at = {}, 0
    for name, dtype, count in parts:
        size = count * np.dtype(dtype).itemsize
        guards = np.concatenate([raw[at:at + 4 * GUARD], raw[at + 4 * GUARD + size:at + 8 * GUARD + size]]).copy().view(np.uint32)
        assert guards.size == 2 * GUARD and np.all(guards == GUARD_WORD), "a guard word was written"
        out[name] = raw[at + 4 * GUARD:at + 4 * GUARD + size].copy().view(dtype)
        at += 8 * GUARD + size
    assert at == raw.size
    if op == 0:
        out = {k: v.reshape(K, N) for k, v in out.items()}
    return out


def motifs_of(widths, seed):
    rng = np.random.default_rng(seed)
    return [R.quantise(R.dirichlet_motif(rng, w)) for w in widths]


def same(got, want):
    for name, _ in OUTPUTS:
        a, b = got[name], want[name]
        if name == "p_min":
            assert np.array_equal(a.view(np.uint64), np.ascontiguousarray(b).view(np.uint64)), name
        else:
            assert np.array_equal(a, b), (name, a, b)


QUERY_WIDTHS, TARGET_WIDTHS = (1, 2, 7, 5), (1, 3, 9, 4, 6, 2, 8)


@pytest.fixture(scope="module")
def case():
    queries, targets = motifs_of(QUERY_WIDTHS, 1), motifs_of(TARGET_WIDTHS, 2)
    targets[4] = R.reverse_complement(queries[2])[1:]            # found on strand -
    targets[3] = queries[3][1:].copy()                           # cut out of a query
    return queries, targets


@pytest.mark.parametrize("both", [1, 0])
def test_outputs_have_the_reference_bits_in_every_setting(exe, tmp_path, case, both):
    queries, targets = case
    B = 7
    want = R.compare(queries, targets, bins=B, both=bool(both), min_overlap=1)
    base = run(exe, tmp_path, queries, targets, bins=B, both=both)
    same(base, want)
    if both:
        assert base["strand"][2, 4] == -1 and base["offset"][2, 4] == 0 and base["overlap"][2, 4] == 6
    assert base["strand"][3, 3] == 1 and base["offset"][3, 3] == 1 and base["overlap"][3, 3] == 4
    per_query = [table_elems(B, w) * 8 + len(targets) * 21 for w in QUERY_WIDTHS]
    for kw in (dict(threads=1), dict(threads=64, tile=1), dict(threads=37, tile=3), dict(tile=7), dict(tile=6),
               dict(budget=max(per_query)),                                       # the widest query alone; the narrow ones together
               dict(budget=per_query[2] + per_query[3], tile=2)):                 # ... and the last group partial
        same(run(exe, tmp_path, queries, targets, bins=B, both=both, **kw), want)


@pytest.mark.parametrize("min_overlap", [3, 100])
def test_min_overlap(exe, tmp_path, case, min_overlap):
    queries, targets = case
    want = R.compare(queries, targets, bins=5, both=True, min_overlap=min_overlap)
    same(run(exe, tmp_path, queries, targets, bins=5, min_overlap=min_overlap, tile=4), want)
    if min_overlap == 100:                                        # beyond every width: the full overlaps only
        m, n = np.array(QUERY_WIDTHS)[:, None], np.array(TARGET_WIDTHS)[None, :]
        assert np.array_equal(want["n_off"], 2 * (np.abs(m - n) + 1)) and np.array_equal(want["overlap"], np.minimum(m, n))


@pytest.mark.parametrize("bins,width", [(2, 5), (256, 3), (16, 64)])
def test_counts_and_tails_of_one_query(exe, tmp_path, bins, width):
    """the limits of bins, and the widest query (64 columns: every counter row and 2080 tail arrays)"""
    query = motifs_of([width], 5)[0]
    targets = motifs_of((3, 64, 1, 11), 6)
    for both in (1, 0):
        pool = R.pool_of(targets, bool(both))
        counts = R.counts_of(query, pool, bins)
        want = R.packed(R.tails_of(counts, 1.0 / len(pool)), width)
        got = run(exe, tmp_path, [query], targets, bins=bins, both=both, op=1, threads=16)
        assert np.array_equal(got["counts"].reshape(width, bins), counts)
        assert np.array_equal(got["tail"].view(np.uint64), want.view(np.uint64))
    assert np.array_equal(run(exe, tmp_path, [query], targets, bins=bins, both=0, op=1, threads=3)["tail"].view(np.uint64), want.view(np.uint64))


def test_palindrome_ties_go_to_strand_plus(exe, tmp_path):
    half = motifs_of([3], 8)[0]
    pal = np.concatenate([half, R.reverse_complement(half)])
    assert np.array_equal(R.reverse_complement(pal), pal)
    targets = motifs_of((4, 5), 9) + [pal]
    got = run(exe, tmp_path, [pal, half], targets, bins=9, tile=2)
    same(got, R.compare([pal, half], targets, bins=9))
    assert got["strand"][0, 2] == 1 and got["offset"][0, 2] == 0 and got["overlap"][0, 2] == 6
    assert got["strand"][1, 2] == 1 and got["offset"][1, 2] == 0          # (the same placements on either strand)


def test_refusals(exe, tmp_path, case):
    queries, targets = case
    qc, qs = pack(queries)
    tc, ts = pack(targets)
    for mask in (1, 2, 4, 8, 16):
        run(exe, tmp_path, queries, targets, null_mask=mask, refused="null argument")
    run(exe, tmp_path, queries, targets, K=0, refused="K and N must be at least 1")
    run(exe, tmp_path, queries, targets, N=0, refused="K and N must be at least 1")
    for bins in (1, 257):
        run(exe, tmp_path, queries, targets, bins=bins, refused="bins must lie in [2, 256]")
    run(exe, tmp_path, queries, targets, min_overlap=0, refused="min_overlap must be at least 1")
    bad = qs.copy()
    bad[0] = 1
    run(exe, tmp_path, queries, targets, qstart=bad, refused="must begin at 0")
    bad = ts.copy()
    bad[2] = bad[1]                                              # a width of 0
    run(exe, tmp_path, queries, targets, tstart=bad, refused="must ascend")
    bad = ts.copy()
    bad[3] = bad[2] - 1
    run(exe, tmp_path, queries, targets, tstart=bad, refused="must ascend")
    wide = motifs_of([65], 3)
    run(exe, tmp_path, wide, targets, refused="a width must lie in [1, 64]")
    run(exe, tmp_path, queries, wide, refused="a width must lie in [1, 64]")
    for cols, name in ((qc, "qcols"), (tc, "tcols")):
        bad = cols.copy()
        bad[-1, 3] = 4097
        run(exe, tmp_path, queries, targets, refused="an entry lies above 4096", **{name: bad})
    for invC in (0.0, -0.5, 1.5, np.nan, np.inf):
        run(exe, tmp_path, queries, targets, invC=invC, refused="invC must lie in (0, 1]")
    assert run(exe, tmp_path, queries, targets, invC=1.0) is not None
    need = table_elems(7, 7) * 8 + len(targets) * 21
    run(exe, tmp_path, queries, targets, budget=need - 1, refused="do not fit CRBM_COMPARE_BYTES")
    assert run(exe, tmp_path, queries, targets, budget=need) is not None
    run(exe, tmp_path, [queries[2]], targets, op=1, budget=need - 1, refused="do not fit CRBM_COMPARE_BYTES")


def test_a_pool_beyond_int32_is_refused(exe, tmp_path, case):
    """2^24 targets of 64 columns on both strands: 2^31 pool columns.  The starts alone say so; no column is read."""
    queries, _ = case
    ts = (np.arange((1 << 24) + 1, dtype=np.int64) * 64).astype(np.int32)
    tiny = np.zeros((1, 4), np.uint16)
    run(exe, tmp_path, queries, [], N=1 << 24, tstart=ts, tcols=tiny, both=1, invC=0.5, refused="more than 2^31 - 1 columns")
