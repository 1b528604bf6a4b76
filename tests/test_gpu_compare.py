"""Motif comparison on the GPU (crbm_amd.compareMotifs, crbm_motif_compare, crbm_motif_compare_null) against
tests/compare_reference.py.

The pipeline is integers up to the counts and one pinned float64 summation order from there, so nothing is compared within
a tolerance: counts are exactly equal, tails and p_min have the reference's bits (np.array_equal on the uint64 view), and
offset, strand, overlap and n_off are exactly equal.  Pools hold between 50 and 1000 columns, so that (1 / C)^64 stays
above 1e-200 and nothing is subnormal.  The reference of every case is computed once per module and never written to."""
import ctypes
import os
import re

import numpy as np
import pytest

from tests import compare_reference as R
from tests.test_gpu_parity import make_pair

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_DP = ctypes.POINTER(ctypes.c_double)
ENV = ("CRBM_COMPARE_TILE", "CRBM_COMPARE_BYTES")
FIELDS = ("p_min", "offset", "strand", "overlap", "n_off")


@pytest.fixture(scope="module")
def model():
    """config #2's double-stranded model: it lends its device"""
    return make_pair(10, 15, ds=True, Lf=186, bshift=3.0, wscale=0.7)[0]


def setting(monkeypatch, tile=None, budget=None):
    for name, value in zip(ENV, (tile, budget)):
        if value is None:
            monkeypatch.delenv(name, raising=False)
        else:
            monkeypatch.setenv(name, str(value))


def matrices_of(widths, seed):
    rng = np.random.default_rng(seed)
    return [R.dirichlet_motif(rng, int(w)) for w in widths]


def as_set(mats, prefix):
    from crbm_amd import MotifSet
    return MotifSet(["%s%d" % (prefix, i) for i in range(len(mats))], mats)


_WANT = {}


def reference(key, queries, targets, **kw):
    """R.compare of the quantised matrices, once per case"""
    if key not in _WANT:
        out = R.compare([R.quantise(m) for m in queries], [R.quantise(m) for m in targets], **kw)
        for f in FIELDS:
            out[f].setflags(write=False)
        _WANT[key] = out
    return _WANT[key]


def same(got, want):
    """got: a MotifComparison or a dict of arrays"""
    for f in FIELDS:
        a = getattr(got, f) if not isinstance(got, dict) else got[f]
        if f == "p_min":
            assert a.dtype == np.float64 and np.array_equal(a.view(np.uint64), want[f].view(np.uint64)), \
                (f, np.argwhere(a.view(np.uint64) != want[f].view(np.uint64))[:5])
        else:
            assert np.array_equal(a, want[f]), (f, np.argwhere(a != want[f])[:5])


def pool_size(targets, both=True):
    return sum(m.shape[1] for m in targets) * (2 if both else 1)


def tile_of():
    from crbm_amd import motifs
    source = open(os.path.join(ROOT, "crbm_amd", "csrc", "crbm_compare.h")).read()
    assert int(re.search(r"TILE_DEFAULT\s*=\s*(\d+)", source).group(1)) == motifs.TARGET_TILE
    return motifs.TARGET_TILE


# queries of the widths 1, 2, 7, 15 and 64; targets narrower and wider than each, among them a query itself, the reverse
# complement of one and a palindrome
def wide_case():
    queries = matrices_of((1, 2, 7, 15, 64), 11)
    targets = matrices_of((1, 3, 20, 64, 5, 9), 12)
    half = matrices_of([4], 13)[0]
    targets += [queries[3].copy(), queries[2][::-1, ::-1].copy(), np.concatenate([half, half[::-1, ::-1]], axis=1)]
    return queries, targets


@pytest.mark.parametrize("strands", ["both", "given"])
def test_every_width_in_one_call(model, monkeypatch, strands):
    """bins = 16 keeps the reference of the 64-column query to seconds.  The same bits with the widest query in a group of
    its own, with one target per block, with a tile that does not divide N and with all targets in one block; and twice."""
    from crbm_amd import compareMotifs, motifs
    queries, targets = wide_case()
    both = strands == "both"
    assert 50 <= pool_size(targets, both) <= 1000
    want = reference(("wide", strands), queries, targets, bins=16, both=both)
    setting(monkeypatch)
    q, t = as_set(queries, "q"), as_set(targets, "t")
    base = compareMotifs(model, q, t, bins=16, strands=strands)
    same(base, want)
    assert base.queries == q.names and base.targets == t.names and base.p_min.shape == (5, 9)
    assert base.offset[3, 6] == 0 and base.strand[3, 6] == 1 and base.overlap[3, 6] == 15 and np.argmin(base.p_min[3]) == 6     # the query itself
    if both:
        assert base.strand[2, 7] == -1 and base.offset[2, 7] == 0 and base.overlap[2, 7] == 7
    pv, ev, qv = R.derive(want["p_min"], want["n_off"])
    assert np.array_equal(base.pvalue, pv) and np.array_equal(base.evalue, ev) and np.allclose(base.qvalue, np.minimum(qv, 1.0), rtol=1e-15)
    total, stages = motifs.last_device_ms(model)
    assert total > 0.0 and all(s > 0.0 for s in stages) and abs(sum(stages) - total) <= 1e-3 * total
    same(compareMotifs(model, q, t, bins=16, strands=strands), want)                    # twice: the same bits
    table = lambda w: sum((w - l + 1) * (l * 15 + 2) for l in range(1, w + 1)) * 8 + 9 * 21
    for tile, budget in ((None, table(64)), (1, table(64)),                  # the narrow four together, then the widest alone
                         (4, None), (64, None)):                             # a tile that does not divide N; all targets in one block
        setting(monkeypatch, tile=tile, budget=budget)
        same(compareMotifs(model, q, t, bins=16, strands=strands), want)


def test_query_groups(model, monkeypatch):
    """five queries of one width: every query a group of its own; groups of two, the last one partial; one group"""
    from crbm_amd import compareMotifs
    queries, targets = matrices_of((7,) * 5, 61), matrices_of((6, 20, 9, 3, 12, 15, 8), 62)
    want = reference("groups", queries, targets, bins=100, both=True)
    q, t = as_set(queries, "q"), as_set(targets, "t")
    one = sum((7 - l + 1) * (l * 99 + 2) for l in range(1, 8)) * 8 + 7 * 21
    for budget in (None, one, 2 * one, 2 * one + one // 2, 5 * one - 1):
        setting(monkeypatch, budget=budget)
        same(compareMotifs(model, q, t), want)
    from crbm_amd import motifs
    setting(monkeypatch)
    monkeypatch.setattr(motifs, "OUTPUT_BYTES", 2 * 7 * 21)      # ... and the queries cut into C calls of two, two and one
    same(compareMotifs(model, q, t), want)


@pytest.mark.parametrize("N", ["one", "tile-1", "tile", "tile+1"])
def test_around_the_target_tile(model, monkeypatch, N):
    from crbm_amd import compareMotifs
    tile = tile_of()
    n = {"one": 1, "tile-1": tile - 1, "tile": tile, "tile+1": tile + 1}[N]
    queries = matrices_of((2, 7, 15), 21)
    widths = [64] if n == 1 else np.random.default_rng(22).integers(2, 13, size=n)
    targets = matrices_of(widths, 23)
    assert 50 <= pool_size(targets) <= 1000
    want = reference(("tile", N), queries, targets, bins=100, both=True)
    setting(monkeypatch)
    same(compareMotifs(model, as_set(queries, "q"), as_set(targets, "t")), want)         # the defaults: 100 bins, both strands


@pytest.mark.parametrize("bins", [2, 256])
def test_the_limits_of_bins(model, monkeypatch, bins):
    """256 bins with a query of width 15 (61 KB of counters in the LDS); the tables and counts of that query too"""
    from crbm_amd import compareMotifs, motifs
    queries, targets = matrices_of((15, 4), 31), matrices_of((6, 20, 9, 3, 12, 15, 8), 32)
    assert 50 <= pool_size(targets) <= 1000
    want = reference(("bins", bins), queries, targets, bins=bins, both=True)
    setting(monkeypatch)
    t = as_set(targets, "t")
    same(compareMotifs(model, as_set(queries, "q"), t, bins=bins), want)
    counts, tails = motifs.compareNull(model, queries[0], t, bins=bins)
    assert counts.dtype == np.uint32 and np.array_equal(counts, want["counts"][0])
    assert sorted(tails) == sorted(want["tails"][0])
    for key, tail in tails.items():
        assert np.array_equal(tail.view(np.uint64), want["tails"][0][key].view(np.uint64)), key


def test_counts_and_tails_of_the_widest_query(model, monkeypatch):
    from crbm_amd import motifs
    queries, targets = wide_case()
    want = reference(("wide", "both"), queries, targets, bins=16, both=True)
    setting(monkeypatch)
    counts, tails = motifs.compareNull(model, queries[4], as_set(targets, "t"), bins=16)
    assert np.array_equal(counts, want["counts"][4]) and np.all(counts.sum(axis=1) == pool_size(targets))
    assert len(tails) == 64 * 65 // 2
    for key, tail in tails.items():
        assert np.array_equal(tail.view(np.uint64), want["tails"][4][key].view(np.uint64)), key
    given, _ = motifs.compareNull(model, queries[2], as_set(targets, "t"), bins=16, strands="given")
    assert np.array_equal(given, R.counts_of(R.quantise(queries[2]), R.pool_of([R.quantise(m) for m in targets], False), 16))


@pytest.mark.parametrize("min_overlap", [1, 5, 100])
def test_min_overlap_and_the_palindrome(model, monkeypatch, min_overlap):
    """100 lies beyond every width: only the full overlaps count.  The palindromic target ties on both strands: +."""
    from crbm_amd import compareMotifs
    queries = matrices_of((2, 7, 15), 41)
    half = matrices_of([5], 42)[0]
    pal = np.concatenate([half, half[::-1, ::-1]], axis=1)
    targets = matrices_of((1, 3, 20, 64, 6), 43) + [pal]
    queries.append(pal.copy())
    want = reference(("overlap", min_overlap), queries, targets, bins=100, both=True, min_overlap=min_overlap)
    setting(monkeypatch)
    got = compareMotifs(model, as_set(queries, "q"), as_set(targets, "t"), min_overlap=min_overlap)
    same(got, want)
    assert got.strand[3, 5] == 1 and got.offset[3, 5] == 0 and got.overlap[3, 5] == 10
    if min_overlap == 100:
        m, n = np.array([2, 7, 15, 10])[:, None], np.array([1, 3, 20, 64, 6, 10])[None, :]
        assert np.array_equal(got.n_off, 2 * (np.abs(m - n) + 1)) and np.array_equal(got.overlap, np.minimum(m, n))


def test_the_models_own_motifs_find_themselves(model, monkeypatch):
    """compareMotifs(model): queries and targets are the model's PFMs; the diagonal is computed like any pair"""
    from crbm_amd import compareMotifs, MotifSet, saveMatches
    setting(monkeypatch)
    c = compareMotifs(model)
    own = MotifSet.from_model(model)
    K = model.num_motifs
    assert c.queries == c.targets == own.names and c.p_min.shape == (K, K)
    diag = np.arange(K)
    assert np.all(c.offset[diag, diag] == 0) and np.all(c.strand[diag, diag] == 1) and np.all(c.overlap[diag, diag] == model.motif_length)
    assert np.array_equal(np.argmin(c.p_min, axis=1), diag)
    off = c.p_min + np.where(np.eye(K) > 0, np.inf, 0.0)
    assert np.all(c.p_min[diag, diag] < off.min(axis=1))         # strictly the smallest of its row
    assert c.best()["target"].tolist() == diag.tolist() and np.all(c.qvalue[diag, diag] <= c.qvalue.min(axis=1))
    same(c, reference("own", own.matrices, own.matrices, bins=100, both=True))


def test_refusals_leave_the_outputs_untouched_and_the_handle_usable(model, monkeypatch):
    from crbm_amd import _lib
    setting(monkeypatch)
    lib, h = model._lib, model._h()
    queries, targets = matrices_of((3, 7), 51), matrices_of((6, 20, 9, 12, 8), 52)
    qs, ts = as_set(queries, "q"), as_set(targets, "t")
    qcols, qstart = qs.quantised()
    tcols, tstart = ts.quantised()
    K, N = 2, 5
    invC = 1.0 / (2 * len(tcols))
    outs = dict(p_min=np.full(K * N + 3, 9.0), offset=np.full(K * N + 3, 9, np.int32), strand=np.full(K * N + 3, 9, np.int8),
                overlap=np.full(K * N + 3, 9, np.int32), n_off=np.full(K * N + 3, 9, np.int32))
    types = dict(p_min=_DP, offset=_lib._I32P, strand=ctypes.POINTER(ctypes.c_int8), overlap=_lib._I32P, n_off=_lib._I32P)

    def call(qcols_=qcols, qstart_=qstart, K_=K, tcols_=tcols, tstart_=tstart, N_=N, bins=100, both=1, min_overlap=1, invC_=invC, null_out=None):
        keep = [None if a is None else np.ascontiguousarray(a) for a in (qcols_, qstart_, tcols_, tstart_)]
        ptr = lambda a, t: None if a is None else a.ctypes.data_as(t)
        out = [None if f == null_out else outs[f].ctypes.data_as(types[f]) for f in FIELDS]
        return lib.crbm_motif_compare(h, ptr(keep[0], _lib._U16P), ptr(keep[1], _lib._I32P), K_, ptr(keep[2], _lib._U16P), ptr(keep[3], _lib._I32P),
                                      N_, bins, both, min_overlap, invC_, *out)

    def refused(rc, why):
        assert rc == _lib.ERR_INVALID and why in lib.crbm_last_error(h).decode(), (rc, lib.crbm_last_error(h))
        assert all(np.all(a == 9) for a in outs.values())

    for kw in (dict(qcols_=None), dict(qstart_=None), dict(tcols_=None), dict(tstart_=None)) + tuple(dict(null_out=f) for f in FIELDS):
        refused(call(**kw), "null")
    refused(call(K_=0), "at least 1")
    refused(call(N_=0), "at least 1")
    for bins in (1, 257):
        refused(call(bins=bins), "bins must lie")
    refused(call(min_overlap=0), "min_overlap")
    bad = qstart.copy()
    bad[0] = 1
    refused(call(qstart_=bad), "begin at 0")
    bad = tstart.copy()
    bad[2] = bad[1]
    refused(call(tstart_=bad), "ascend")
    wide = as_set(matrices_of([64], 53), "w").quantised()[0]
    refused(call(qcols_=np.concatenate([wide, wide[:1]]), qstart_=np.array([0, 65], np.int32), K_=1), "[1, 64]")
    bad = tcols.copy()
    bad[-1, 0] = 4097
    refused(call(tcols_=bad), "above 4096")
    bad = qcols.copy()
    bad[0, 3] = 65535
    refused(call(qcols_=bad), "above 4096")
    for value in (0.0, -1.0, 1.0 + 1e-9, np.nan, np.inf):
        refused(call(invC_=value), "invC")
    starts = (np.arange((1 << 24) + 1, dtype=np.int64) * 64).astype(np.int32)        # 2^30 columns on two strands; no column is read
    refused(call(tstart_=starts, N_=1 << 24), "2^31 - 1")
    table = lambda w: sum((w - l + 1) * (l * 99 + 2) for l in range(1, w + 1)) * 8 + N * 21
    monkeypatch.setenv("CRBM_COMPARE_BYTES", str(table(7) - 1))
    refused(call(), "CRBM_COMPARE_BYTES")
    counts, tail = np.full(3 * 100, 9, np.uint32), np.full(table(3) // 8, 9.0)
    monkeypatch.setenv("CRBM_COMPARE_BYTES", str(table(3) - 1))
    rc = lib.crbm_motif_compare_null(h, qcols.ctypes.data_as(_lib._U16P), 3, tcols.ctypes.data_as(_lib._U16P), tstart.ctypes.data_as(_lib._I32P),
                                     N, 100, 1, invC, counts.ctypes.data_as(ctypes.POINTER(ctypes.c_uint32)), tail.ctypes.data_as(_DP))
    assert rc == _lib.ERR_INVALID and "CRBM_COMPARE_BYTES" in lib.crbm_last_error(h).decode() and np.all(counts == 9) and np.all(tail == 9.0)
    rc = lib.crbm_motif_compare_null(h, qcols.ctypes.data_as(_lib._U16P), 65, tcols.ctypes.data_as(_lib._U16P), tstart.ctypes.data_as(_lib._I32P),
                                     N, 100, 1, invC, counts.ctypes.data_as(ctypes.POINTER(ctypes.c_uint32)), tail.ctypes.data_as(_DP))
    assert rc == _lib.ERR_INVALID and "[1, 64]" in lib.crbm_last_error(h).decode() and np.all(counts == 9)
    monkeypatch.setenv("CRBM_COMPARE_BYTES", str(table(7)))          # and the handle still serves: every query a group of its own
    assert call() == 0
    want = reference("refusals", queries, targets, bins=100, both=True)
    same({f: outs[f][:K * N].reshape(K, N) for f in FIELDS}, want)
    assert all(np.all(a[K * N:] == 9) for a in outs.values())
    ms, stages = ctypes.c_float(-1.0), (ctypes.c_float * 3)()
    assert lib.crbm_compare_ms(h, ctypes.byref(ms), stages) == 0 and ms.value > 0.0
    assert lib.crbm_compare_ms(h, ctypes.byref(ms), None) == 0
