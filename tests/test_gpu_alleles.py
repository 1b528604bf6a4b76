"""The allele effects (CRBM.alleleEffects, crbm_allele_effects_codes) on the GPU, on the specialised and slabbed model
classes of test_gpu_sweeps (10 x 15 ds, 20 x 15 ds, 300 x 10 in five slabs, 257 x 1 with the moved-back last slab),
stream gapped_stream(5003, 2031), 1500 random alleles plus the forced ones of tests/allele_reference.py: against the
float64 reference by that module's criterion |got - want| <= RTOL |want| + RTOL max|want| + RTOL mass (dfe and per_motif
separately, windows and the exact zeros exactly); the same bits in a second run, in one chunk, in about 7 and about 40
chunks over both streams, at CRBM_SLAB_BYTES=1 and under a permutation; every output alone; (1, 1) alleles against
variantEffects; what an inserted gap changes; the refusals; a parameter change; and 2^18 alleles on 2^22 letters for
config #2's double-stranded model."""
import numpy as np
import pytest

from tests.test_gpu_parity import make_pair, RTOL
from tests.test_gpu_sweeps import CLASSES, ids, _model
from tests.test_gpu_scan import gapped_stream
from tests.allele_reference import allele_effects, allele_list, check, pack, strings

pytestmark = pytest.mark.gpu

SERVED = [CLASSES[0], CLASSES[1], CLASSES[2], CLASSES[3]]
T_A, SEED = 5003, 2031
KEYS = ("dfe", "per_motif", "windows")
_shared = {}


def the_list(cls):
    """(stream, pos, R, alts, want) of a model class: the list and its reference are made once and left unchanged"""
    name, K, M, ds, A, pool, Lf, L, env, spec = cls
    if name not in _shared:
        stream = gapped_stream(T_A, SEED)
        pos, R, alts = allele_list(stream, M, 1500, 77)
        _shared[name] = (stream, pos, R, alts)
    return _shared[name]


def reference(cls, o):
    name = cls[0]
    if ("want", name) not in _shared:
        stream, pos, R, alts = the_list(cls)
        _shared[("want", name)] = allele_effects(o, stream, pos, R, alts)
    return _shared[("want", name)]


def costs(cls, R, alts):
    """bytes the driver counts per variant (crbm_sweep.h, allele_plan)"""
    name, K, M, ds, A, pool, Lf, L, env, spec = cls
    n = np.asarray(R, np.int64) + np.array([len(a) for a in alts], np.int64) + 4 * M - 4
    return n + (3 * n + 7) // 8 + 16 + 4 * (K + 3)


def _same(a, b, label=""):
    for key in KEYS:
        assert a[key].dtype == b[key].dtype and a[key].tobytes() == b[key].tobytes(), (label, key)


def _c_call(m, stream, pos, R, alt_off, alt_codes, K, want=KEYS, fill=77, T=None, nvar=None):
    """crbm_allele_effects_codes with the outputs in `want` (the others NULL): (rc, outputs pre-filled with `fill`)"""
    from crbm_amd import _lib
    V = len(pos)
    out = {"dfe": np.full(V, fill, np.float32), "per_motif": np.full((V, K), fill, np.float32), "windows": np.full((V, 2), fill, np.int32)}
    pos, R = np.ascontiguousarray(pos, np.int64), np.ascontiguousarray(R, np.int32)
    alt_off, alt_codes = np.ascontiguousarray(alt_off, np.int64), np.ascontiguousarray(alt_codes, np.uint8)
    p = lambda key, ty: out[key].ctypes.data_as(ty) if key in want else None
    h = m._h()                                                     # (creates the handle and binds the library on first use)
    rc = m._lib.crbm_allele_effects_codes(h, stream.ctypes.data_as(_lib._U8P), stream.size if T is None else T,
                                          V if nvar is None else nvar, pos.ctypes.data_as(_lib._I64P), R.ctypes.data_as(_lib._I32P),
                                          alt_off.ctypes.data_as(_lib._I64P), alt_codes.ctypes.data_as(_lib._U8P),
                                          p("dfe", _lib._F), p("per_motif", _lib._F), p("windows", _lib._I32P))
    return rc, out


def _call(m, stream, pos, R, alts):
    """CRBM.alleleEffects on a list of the reference's form, untrimmed"""
    ref, alt = strings(stream, pos, R, alts)
    return m.alleleEffects(stream, pos, ref, alt, trim=False)


@pytest.mark.parametrize("cls", SERVED, ids=ids(SERVED))
def test_alleles_against_reference_and_the_same_bits_for_every_chunking(cls, monkeypatch):
    name, K, M, ds, A, pool, Lf, L, env, spec = cls
    m, o = _model(cls, monkeypatch)
    stream, pos, R, alts = the_list(cls)
    V = pos.size
    want = reference(cls, o)
    monkeypatch.delenv("CRBM_SLAB_BYTES", raising=False)
    got = _call(m, stream, pos, R, alts)                                                    # one chunk
    assert got["dfe"].shape == (V,) and got["per_motif"].shape == (V, K) and got["windows"].shape == (V, 2)
    check(got, want, RTOL, name)
    _same(got, _call(m, stream, pos, R, alts), "second run")
    total = int(costs(cls, R, alts).sum())
    for chunks in (7, 40):
        monkeypatch.setenv("CRBM_SLAB_BYTES", str(total // chunks))
        _same(got, _call(m, stream, pos, R, alts), "about %d chunks" % chunks)
    monkeypatch.setenv("CRBM_SLAB_BYTES", "1")
    _same(got, _call(m, stream, pos, R, alts), "one variant a chunk")
    monkeypatch.setenv("CRBM_SLAB_BYTES", str(total // 5))
    perm = np.random.default_rng(5).permutation(V)
    shuffled = _call(m, stream, pos[perm], R[perm], [alts[i] for i in perm])
    _same({k: got[k][perm] for k in KEYS}, shuffled, "permuted")


@pytest.mark.parametrize("cls", [CLASSES[0], CLASSES[3]], ids=ids([CLASSES[0], CLASSES[3]]))
def test_every_output_alone_gives_the_same_bits(cls, monkeypatch):
    name, K, M, ds, A, pool, Lf, L, env, spec = cls
    m, o = _model(cls, monkeypatch)
    stream, pos, R, alts = the_list(cls)
    off, codes = pack(alts)
    monkeypatch.setenv("CRBM_SLAB_BYTES", str(int(costs(cls, R, alts).sum()) // 3))
    rc, full = _c_call(m, stream, pos, R, off, codes, K)
    assert rc == 0
    check(full, reference(cls, o), RTOL, name)                                              # the C call takes the zero variants too
    for key in KEYS:
        rc, one = _c_call(m, stream, pos, R, off, codes, K, want=(key,))
        assert rc == 0 and one[key].tobytes() == full[key].tobytes(), key
        assert all(np.all(one[other] == 77) for other in KEYS if other != key)             # the NULL outputs' stand-ins: untouched


@pytest.mark.parametrize("cls", [CLASSES[0], CLASSES[2]], ids=ids([CLASSES[0], CLASSES[2]]))
def test_one_for_one_alleles_agree_with_variant_effects(cls, monkeypatch):
    """(1, 1) alleles against variantEffects within the criterion (both are within it of the reference; the two kernels
    add in different orders), windows[:, 0] == windows[:, 1] == the SNP's count"""
    name, K, M, ds, A, pool, Lf, L, env, spec = cls
    m, o = _model(cls, monkeypatch)
    monkeypatch.delenv("CRBM_SLAB_BYTES", raising=False)
    stream = gapped_stream(T_A, SEED)
    rng = np.random.default_rng(31)
    pos, alt = rng.integers(0, T_A, size=1000), rng.integers(0, 4, size=1000).astype(np.uint8)
    alts = [alt[i:i + 1] for i in range(1000)]
    snp = m.variantEffects(stream, pos, alt)
    got = _call(m, stream, pos, np.ones(1000, np.int32), alts)
    assert np.array_equal(got["windows"][:, 0], snp["windows"]) and np.array_equal(got["windows"][:, 1], snp["windows"])
    mass = allele_effects(o, stream, pos, np.ones(1000, np.int32), alts)["mass"]
    for key in ("dfe", "per_motif"):
        g, s = got[key].astype(np.float64), snp[key].astype(np.float64)
        err, bound = np.abs(g - s), RTOL * np.abs(s) + RTOL * np.abs(s).max() + RTOL * mass[key]
        print("%s %s vs variantEffects: max err %.3g, max|snp| %.4g" % (name, key, err.max(), np.abs(s).max()))
        assert np.all(err <= bound), key
    assert np.all(got["dfe"][stream[pos] > 3] == 0.0) and (stream[pos] > 3).any()


def _lost(pos, R, A, M, g):
    """the windows of (refhap, althap) of every variant that cover stream position g (none of the spans holds it)"""
    lost = np.zeros((pos.size, 2), np.int64)
    for i, (p, r, a) in enumerate(zip(pos.tolist(), R.tolist(), A.tolist())):
        for h, n in ((0, r), (1, a)):
            at = g - (p - (M - 1)) if g < p else (M - 1) + n + (g - (p + r))      # g in the haplotype's coordinates
            if 0 <= at < n + 2 * (M - 1):
                starts = np.arange(n + M - 1)
                lost[i, h] = ((starts <= at) & (at < starts + M)).sum()
    return lost


@pytest.mark.parametrize("cls", [CLASSES[0], CLASSES[2]], ids=ids([CLASSES[0], CLASSES[2]]))
def test_an_inserted_gap_removes_the_windows_that_cover_it_and_nothing_else(cls, monkeypatch):
    name, K, M, ds, A, pool, Lf, L, env, spec = cls
    m, o = _model(cls, monkeypatch)
    monkeypatch.delenv("CRBM_SLAB_BYTES", raising=False)
    stream = np.random.default_rng(8).integers(0, 4, size=600, dtype=np.uint8)
    rng = np.random.default_rng(18)
    pos = np.arange(100, 500, dtype=np.int64)
    R = rng.integers(0, 4, size=pos.size).astype(np.int32)
    alts = [rng.integers(0, 4, size=int(n)).astype(np.uint8) for n in rng.integers(0, 4, size=pos.size)]
    A = np.array([len(a) for a in alts])
    gaps = (300, 300 + M // 2, 299 + M, 250)
    R[np.array(gaps) - 100] = np.maximum(R[np.array(gaps) - 100], 1)     # every gap falls into a replaced span as well
    live = (R > 0) | (A > 0)
    before = _call(m, stream, pos, R, alts)
    assert np.array_equal(before["windows"][live], np.stack([R + M - 1, A + M - 1], axis=1)[live])
    for g in gaps:
        gapped = stream.copy()
        gapped[g] = 4
        keep = live & ~((pos <= g) & (g < pos + R))                       # (a span that holds the gap: zeros, checked below)
        after = m.alleleEffects(gapped, pos, strings(gapped, pos, R, alts)[0], strings(gapped, pos, R, alts)[1], trim=False)
        assert np.array_equal((before["windows"] - after["windows"])[keep], _lost(pos, R, A, M, g)[keep]), g
        far = (pos + R + M - 1 <= g) | (pos - (M - 1) > g)
        assert far.sum() > 300
        _same({k: before[k][far] for k in KEYS}, {k: after[k][far] for k in KEYS}, g)
        check(after, allele_effects(o, gapped, pos, R, alts), RTOL, "%s gap at %d" % (name, g))
        hit = (pos <= g) & (g < pos + R)
        assert hit.any() and np.all(after["dfe"][hit] == 0.0) and np.all(after["windows"][hit] == 0)


def test_refusals_leave_outputs_untouched_and_the_handle_usable(monkeypatch):
    from crbm_amd import _lib
    stream = gapped_stream(400, 3)
    pos, R, alts = allele_list(stream, 15, 50, 4)
    off, codes = pack(alts)
    ref, alt = strings(stream, pos, R, alts)
    for cls in (CLASSES[4], CLASSES[7], CLASSES[6]):                # pooled, 20 letters, motifs beyond 64 letters
        name, K, M, ds, A, pool, Lf, L, env, spec = cls
        m, o = _model(cls, monkeypatch)
        rc, out = _c_call(m, stream, pos, R, off, codes, K)
        assert rc == _lib.ERR_INVALID and all(np.all(out[k] == 77) for k in KEYS), name
        with pytest.raises(Exception, match="pooling|alphabet|generic"):
            m.alleleEffects(stream, pos, ref, alt)
    name, K, M, ds, A, pool, Lf, L, env, spec = CLASSES[0]
    m, o = _model(CLASSES[0], monkeypatch)
    monkeypatch.setenv("CRBM_SLAB_BYTES", str(int(costs(CLASSES[0], R, alts).sum()) // 4))
    rc, good = _c_call(m, stream, pos, R, off, codes, K)
    assert rc == 0
    check(good, allele_effects(o, stream, pos, R, alts), RTOL, "before the refusals")
    V = pos.size

    def changed(a, i, v):
        a = a.copy()
        a[i] = v
        return a
    bad_code = changed(stream, 399, 5)
    long_off = off.copy()
    long_off[-1] += 65536 - (off[-1] - off[-2])                     # the last alt: 65536 letters
    cases = {"pos + R > T": (stream, changed(pos, V - 1, stream.size - 1), R, off, codes, {}),
             "pos < 0": (stream, changed(pos, 0, -1), R, off, codes, {}),
             "pos = T, R = 1": (stream, changed(pos, 0, stream.size), changed(R, 0, 1), off, codes, {}),
             "ref_len < 0": (stream, pos, changed(R, 3, -1), off, codes, {}),
             "ref_len = 65536": (stream, pos, changed(R, 3, 65536), off, codes, {}),
             "alt_off[0] != 0": (stream, pos, R, off + 1, np.concatenate([codes, [0]]), {}),
             "alt_off descends": (stream, pos, R, changed(off, V // 2, off[-1] + 5), np.concatenate([codes, np.zeros(5)]), {}),
             "an alt of 65536 letters": (stream, pos, R, long_off, np.zeros(long_off[-1], np.uint8), {}),
             "an alt code 4": (stream, pos, R, off, changed(codes, codes.size - 1, 4), {}),
             "a code 5": (bad_code, pos, R, off, codes, {}), "all outputs NULL": (stream, pos, R, off, codes, {"want": ()}),
             "nvar < 0": (stream, pos, R, off, codes, {"nvar": -1}), "T < 0": (stream, pos, R, off, codes, {"T": -1}),
             "T = 2^31": (stream, pos, R, off, codes, {"T": 2 ** 31})}
    for what, (s, p, r, ao, ac, kw) in cases.items():
        rc, out = _c_call(m, s, p, r, ao, ac, K, **kw)
        assert rc == _lib.ERR_INVALID and all(np.all(out[k] == 77) for k in KEYS), what
        rc, again = _c_call(m, stream, pos, R, off, codes, K)
        assert rc == 0, what
        _same(good, again, what)
    rc, out = _c_call(m, stream, pos, R, off, codes, K, nvar=0)    # nvar == 0 succeeds and writes nothing
    assert rc == 0 and all(np.all(out[k] == 77) for k in KEYS)
    rc, out = _c_call(m, stream, [stream.size], [0], [0, 2], [1, 2], K)       # pos = T with R = 0: an insertion behind the last code
    assert rc == 0
    check(out, allele_effects(o, stream, np.array([stream.size]), np.array([0]), [np.array([1, 2], np.uint8)]), RTOL, "pos = T")


def test_a_parameter_change_between_two_calls_is_seen_by_the_second(monkeypatch):
    m, o = _model(CLASSES[0], monkeypatch)
    monkeypatch.delenv("CRBM_SLAB_BYTES", raising=False)
    stream = gapped_stream(1200, 6)
    pos, R, alts = allele_list(stream, 15, 300, 9)
    first = _call(m, stream, pos, R, alts)
    check(first, allele_effects(o, stream, pos, R, alts), RTOL, "before")
    W = (o.W * 0.5).astype(np.float32)
    b = (o.b - 1.0).astype(np.float32)
    c = (o.c + np.array([[0.3, -0.2, 0.1, 0.0]])).astype(np.float32)
    m.motifs.set_value(W)
    m.bias.set_value(b)
    m.c.set_value(c)
    o.W, o.b, o.c = W.astype(np.float64), b.astype(np.float64), c.astype(np.float64)
    second = _call(m, stream, pos, R, alts)
    check(second, allele_effects(o, stream, pos, R, alts), RTOL, "after")
    assert np.abs(second["dfe"] - first["dfe"]).max() > 0.1


def test_alleles_scale_cfg2_two_to_the_18_on_two_to_the_22():
    """config #2's double-stranded model, 2^18 random alleles (R and A from 0..3) on 2^22 letters with gap runs, through
    the C call: finite outputs, the first and the last 256 against the reference, and a repeat with the same bits"""
    K, M = 10, 15
    T, V = 1 << 22, 1 << 18
    m, o = make_pair(K, M, ds=True, Lf=186, bshift=3.0, wscale=0.7)
    stream = gapped_stream(T, 99, share=0.01, run=500)
    rng = np.random.default_rng(17)
    R = rng.integers(0, 4, size=V).astype(np.int32)
    pos = rng.integers(0, T - 3, size=V)
    A = rng.integers(0, 4, size=V)
    off = np.concatenate([[0], np.cumsum(A)]).astype(np.int64)
    codes = rng.integers(0, 4, size=int(off[-1])).astype(np.uint8)
    rc, got = _c_call(m, stream, pos, R, off, codes, K)
    assert rc == 0
    assert np.all(np.isfinite(got["dfe"])) and np.all(np.isfinite(got["per_motif"]))
    assert got["windows"].min() == 0 and got["windows"].max() == 3 + M - 1
    for sl in (slice(0, 256), slice(V - 256, V)):
        alts = [codes[off[i]:off[i + 1]] for i in range(sl.start, sl.stop)]
        check({k: got[k][sl] for k in KEYS}, allele_effects(o, stream, pos[sl], R[sl], alts), RTOL, "scale")
    rc, again = _c_call(m, stream, pos, R, off, codes, K)
    assert rc == 0
    _same(got, again, "repeat")
