"""Record summaries (CRBM.recordSummary, crbm_scan_records_codes) on the GPU: every output against the float64
reference of tests/record_reference.py (check_fe: the derived free-energy tolerance; check_best: the best-site rule;
windows and letters exactly) on the specialised and slabbed model classes of test_gpu_sweeps; the same bits for every
CRBM_SLAB_BYTES and run; rows of A ++ [4] ++ B are the rows of A then of B; a code 4 changes one row; the cross-checks
against freeEnergy, motifBestSites and scanSites on equal-length records; the refusals, a bad code in the first and in
the last of 7 segments among them; and 2^22 letters in one record on config #2's double-stranded model."""
import numpy as np
import pytest

from tests.test_gpu_parity import make_pair, RTOL
from tests.test_gpu_sweeps import CLASSES, ids, _model
from tests.test_gpu_scan import gapped_stream, per_start
from tests.scan_reference import window_valid
from tests import record_reference as rr

pytestmark = pytest.mark.gpu

SERVED = [CLASSES[0], CLASSES[1], CLASSES[2], CLASSES[3]]   # 10 x 15 ds, 20 x 15 ds, 300 x 10 (five slabs), 257 x 1 (last slab moved back)
SEED = 2031
KEYS = ("windows", "letters", "fe", "per_motif", "start", "strand", "prob")


def _c_records(m, stream, offsets):
    """crbm_scan_records_codes itself over the whole stream (recordSummary would cut pieces by the accumulator budget
    first): the dict of recordSummary"""
    return m._records_call(np.ascontiguousarray(stream), np.ascontiguousarray(offsets, np.int64))


def _same(a, b):
    for k in KEYS:
        x, y = np.asarray(a[k]), np.asarray(b[k])
        assert x.shape == y.shape, k
        if x.dtype.kind == "f":
            assert np.array_equal(x.view(np.uint32), y.astype(x.dtype).view(np.uint32)), k
        else:
            assert np.array_equal(x, y.astype(x.dtype)), k
    assert a["unit"] == b["unit"]


def _rows(parts):
    out = {k: np.concatenate([np.asarray(p[k]) for p in parts]) for k in KEYS}
    out["unit"] = parts[0]["unit"]
    return out


@pytest.mark.parametrize("cls", SERVED, ids=ids(SERVED))
def test_records_against_reference_and_the_same_bits_for_every_segmenting(cls, monkeypatch):
    """(a) record_stream(2031, M): check_fe with the unit the call returned -- |got - ref| <= RTOL |ref| + windows unit / 2
    per cell of per_motif, the sum of a row's bounds plus RTOL sum_a letters |c_a| for fe, windows and letters exactly --
    and check_best, which caps the ambiguous cells at 1 %; the run prints its own share.
    (b) the same bits for the default CRBM_SLAB_BYTES (one segment), one that gives 7 segments, one whose segment edge
    falls inside a record and (M > 1) inside a window, and a second run."""
    name, K, M, ds, A, pool, Lf, L, env, spec = cls
    m, o = _model(cls, monkeypatch)
    stream, offsets = rr.record_stream(SEED, M)
    ref = rr.record_summary(o, stream, offsets)
    monkeypatch.delenv("CRBM_SLAB_BYTES", raising=False)
    got = m.recordSummary(stream, offsets)
    assert got["strand"].dtype == np.int8 and got["start"].dtype == np.int32 and got["windows"].dtype == np.int64
    assert 0 < got["unit"] <= 1.0 and np.log2(got["unit"]) == round(np.log2(got["unit"]))
    rr.check_fe(got, ref, RTOL, got["unit"], name)
    amb, cells, ties, mirror = rr.check_best(got, ref, RTOL, name)
    print("%s: %d of %d cells ambiguous (%.2f %%), %d exact ties, %d mirror ties" % (name, amb, cells, 100.0 * amb / cells, ties, mirror))
    _same(got, m.recordSummary(stream, offsets))
    _same(got, _c_records(m, stream, offsets))
    starts = stream.size - M + 1
    monkeypatch.setenv("CRBM_SLAB_BYTES", str(per_start(cls) * (starts // 7 + 1)))
    _same(got, _c_records(m, stream, offsets))
    _same(got, m.recordSummary(stream, offsets))             # (cut into pieces of records as well: the accumulator budget)
    edge = next(e for e in range(2500, 4000) if np.all(stream[e - M:e + M] < 4))      # letters all around: one record, M windows
    monkeypatch.setenv("CRBM_SLAB_BYTES", str(per_start(cls) * edge))
    _same(got, _c_records(m, stream, offsets))


@pytest.mark.parametrize("cls", [CLASSES[0], CLASSES[2]], ids=ids([CLASSES[0], CLASSES[2]]))
def test_rows_of_a_concatenation_and_a_gap_in_one_record(cls, monkeypatch):
    """rows of A ++ [4] ++ B are the rows of A followed by the rows of B, bit for bit; a code 4 written into one record
    changes that record's row alone, and lowers its windows by the valid windows that covered the position"""
    name, K, M, ds, A, pool, Lf, L, env, spec = cls
    m, o = _model(cls, monkeypatch)
    monkeypatch.delenv("CRBM_SLAB_BYTES", raising=False)
    stream, offsets = rr.record_stream(SEED, M)
    recs = rr.split_records(stream, offsets)
    whole = m.recordSummary(stream, offsets)
    _same(whole, _rows([m.recordSummary(*rr.make_stream(recs[:23])), m.recordSummary(*rr.make_stream(recs[23:]))]))
    r = int(np.argmax(whole["windows"][:-1]))                # the longest of the random records
    valid = window_valid(stream, M)
    inside = np.flatnonzero(valid[offsets[r]:offsets[r + 1] - M])
    p = int(offsets[r] + inside[inside.size // 2]) + M // 3
    covered = int(valid[max(int(offsets[r]), p - M + 1):p + 1].sum())
    assert covered > 0 and stream[p] < 4
    gap = stream.copy()
    gap[p] = 4
    g = m.recordSummary(gap, offsets)
    others = np.arange(len(recs)) != r
    for k in KEYS:
        assert np.array_equal(np.asarray(g[k])[others], np.asarray(whole[k])[others]), k
    assert g["windows"][r] == whole["windows"][r] - covered and g["letters"][r].sum() == whole["letters"][r].sum() - 1
    assert np.all(g["per_motif"][r] > whole["per_motif"][r])  # fewer softplus terms: every column moves up


@pytest.mark.parametrize("cls", SERVED[:3], ids=ids(SERVED[:3]))
def test_cross_checks_against_the_per_sequence_entry_points(cls, monkeypatch):
    """64 N-free records of 80 letters.  fe against 80 * freeEnergy(codes): both are held to the oracle, recordSummary
    by check_fe's bound and freeEnergy by RTOL |ref| (tests/test_gpu_parity.py), so they differ by at most the sum of
    the two.  prob equals the largest prob of scanSites(stream, 0.0) per (record, motif) bit for bit.  start / strand /
    prob equal motifBestSites(codes) bit for bit on the specialised models, where motifBestSites scores through
    window_strand_z as the stream kernels do; a generic model's motifBestSites runs on the generic kernels, whose sums
    round differently, so the slabbed class is held to it within 2 RTOL, and to the same site in 99 % of the cells."""
    name, K, M, ds, A, pool, Lf, L, env, spec = cls
    m, o = _model(cls, monkeypatch)
    monkeypatch.delenv("CRBM_SLAB_BYTES", raising=False)
    codes = np.random.default_rng(5).integers(0, 4, size=(64, 80), dtype=np.uint8)
    stream, offsets = rr.make_stream(list(codes))
    got = m.recordSummary(stream, offsets)
    ref = rr.record_summary(o, stream, offsets)
    rr.check_fe(got, ref, RTOL, got["unit"], name)
    assert np.all(got["windows"] == 80 - M + 1) and np.all(got["letters"].sum(axis=1) == 80)
    bound = (RTOL * np.abs(ref["per_motif"]) + ref["windows"][:, None] * got["unit"] / 2).sum(axis=1) \
        + RTOL * (ref["letters"] * np.abs(ref["c"])[None, :]).sum(axis=1) + RTOL * np.abs(ref["fe"])
    fe80 = 80.0 * m.freeEnergy(codes).astype(np.float64)
    err = np.abs(got["fe"].astype(np.float64) - fe80)
    print("%s: fe against 80 freeEnergy: max err %.3g, its bound %.3g" % (name, err.max(), bound[err.argmax()]))
    assert np.all(err <= bound)
    best = m.motifBestSites(codes)
    if spec:
        assert np.array_equal(got["start"], best["start"]) and np.array_equal(got["strand"], best["strand"])
        assert np.array_equal(got["prob"].view(np.uint32), best["prob"].view(np.uint32))
    else:
        np.testing.assert_allclose(got["prob"], best["prob"], rtol=2 * RTOL)          # each within RTOL of the oracle's maximum
        assert ((got["start"] == best["start"]) & (got["strand"] == best["strand"])).mean() > 0.99
    sites = m.scanSites(stream, 0.0, offsets=offsets)
    top = np.zeros((64, K), np.float32)
    np.maximum.at(top, (sites["seq"], sites["motif"]), sites["prob"])
    assert np.array_equal(got["prob"].view(np.uint32), top.view(np.uint32))


def test_refusals_and_the_handle_stays_usable(monkeypatch):
    """a pooled model; a rec_start that does not start at 0, does not ascend, does not end with T + 1, or whose joint
    is no code 4 (at the C entry point: the Python side would refuse first); no output at all; a code 5 in the last and
    in the first of 7 segments -- and after every refusal the same handle returns the same bits as before"""
    from crbm_amd import _lib
    stream, offsets = rr.record_stream(SEED, 6)
    m, o = _model(CLASSES[4], monkeypatch)
    with pytest.raises(Exception, match="pooling"):
        m.recordSummary(stream, offsets)
    cls = CLASSES[0]
    name, K, M, ds, A, pool, Lf, L, env, spec = cls
    m, o = _model(cls, monkeypatch)
    stream, offsets = rr.record_stream(SEED, M)
    R = offsets.size - 1
    starts = stream.size - M + 1
    seg = starts // 7 + 1
    assert -(-starts // seg) == 7
    monkeypatch.setenv("CRBM_SLAB_BYTES", str(per_start(cls) * seg))
    good = _c_records(m, stream, offsets)
    win = np.full(R, -7, np.int64)
    lib, h = m._lib, m._h()
    call = lambda st, off, w=win: lib.crbm_scan_records_codes(
        h, st.ctypes.data_as(_lib._U8P), st.size, np.ascontiguousarray(off, np.int64).ctypes.data_as(_lib._I64P), len(off) - 1,
        w.ctypes.data_as(_lib._I64P) if w is not None else None, None, None, None, None, None, None, None)
    for bad, word in ((offsets + 1, "start at 0"), (np.concatenate([offsets[:3], offsets[2:3], offsets[3:-1]]), "ascend"),
                      (np.concatenate([offsets[:-1], offsets[-1:] + 1]), r"T \+ 1"),
                      (np.concatenate([offsets[:20], offsets[20:21] - 1, offsets[21:]]), "code 4")):
        assert len(bad) == len(offsets)
        assert call(stream, bad) == _lib.ERR_INVALID
        with pytest.raises(Exception, match=word):
            m._check(call(stream, bad))
    assert call(stream, offsets, None) == _lib.ERR_INVALID     # no output
    assert np.all(win == -7)                                     # a refusal writes nothing
    _same(good, _c_records(m, stream, offsets))
    for p in (stream.size - 2, int(offsets[6]) + 1):           # read by the last segment alone; by the first alone (no joint)
        assert (p >= 6 * seg + M - 1 or p < seg) and stream[p] < 4
        bad = stream.copy()
        bad[p] = 5
        with pytest.raises(Exception, match=r"0\.\.4"):
            _c_records(m, bad, offsets)
        _same(good, _c_records(m, stream, offsets))
    monkeypatch.delenv("CRBM_SLAB_BYTES", raising=False)
    _same(good, m.recordSummary(stream, offsets))
    short = m.recordSummary(*rr.make_stream([np.array([0, 1, 4, 3], np.uint8), np.zeros(0, np.uint8)]))   # T < M
    assert short["letters"].tolist() == [[1, 1, 0, 1], [0, 0, 0, 0]] and not short["windows"].any() and np.all(short["start"] == -1)


def test_one_record_of_two_to_the_22_letters():
    """config #2's double-stranded model over 2^22 random letters with gap runs as ONE record: a wave keeps the record's
    sums and keys in registers over its whole run of tiles and flushes once.  windows and letters exactly; against the
    same stream as two records (a code 4 in the middle): the integer sums add, so per_motif of the whole is the float32
    of the sum of the halves' sums -- within the three float32 roundings involved, 3 * 2^-24 relative -- and the best
    site is the better of the halves' best sites, ties to the first half."""
    K, M = 10, 15
    T = 1 << 22
    m, o = make_pair(K, M, ds=True, Lf=186, bshift=3.0, wscale=0.7)
    stream = gapped_stream(T, 99, share=0.01, run=500)
    half = T // 2
    stream[half - 1] = stream[half + 1] = 2
    stream[half] = 4
    one = m.recordSummary(stream, np.array([0, T + 1]))
    two = m.recordSummary(stream, np.array([0, half + 1, T + 1]))
    n = int(window_valid(stream, M).sum())
    assert one["windows"].tolist() == [n] and two["windows"].sum() == n
    assert one["letters"][0].tolist() == np.bincount(stream[stream < 4], minlength=4).tolist()
    assert np.array_equal(two["letters"].sum(axis=0), one["letters"][0])
    want = two["per_motif"].astype(np.float64).sum(axis=0)
    assert np.all(np.abs(one["per_motif"][0] - want) <= 3 * 2.0 ** -24 * np.abs(want))
    assert np.all(one["per_motif"][0] < -1000.0)
    first = two["prob"][0] >= two["prob"][1]
    assert np.array_equal(one["prob"][0].view(np.uint32), np.where(first, two["prob"][0], two["prob"][1]).view(np.uint32))
    assert np.array_equal(one["start"][0], np.where(first, two["start"][0], two["start"][1] + half + 1))
    assert np.array_equal(one["strand"][0], np.where(first, two["strand"][0], two["strand"][1]))
