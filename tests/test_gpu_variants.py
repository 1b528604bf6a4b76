"""The variant effects (CRBM.variantEffects, crbm_variant_effects_codes) on the GPU, on specialised and slabbed model
classes of test_gpu_sweeps (10 x 15 ds, 20 x 15 ds, 300 x 10 in five slabs, 257 x 1 with the moved-back last slab),
stream gapped_stream(5003, 2031), about 2000 random variants plus the forced ones of tests/variant_reference.py:
against the float64 reference by the project's mutagenesis criterion |got - want| <= RTOL |want| + RTOL max|want| (dfe
and per_motif separately, windows and the exact zeros exactly); the same bits in a second run, in one chunk, in 7
chunks over both streams, at CRBM_SLAB_BYTES=1 and under a permutation; every output alone; agreement with
mutagenesis() on gap-free rows; what an inserted gap changes; the refusals; a parameter change; and 2^20 variants on
2^24 letters for config #2's double-stranded model."""
import ctypes

import numpy as np
import pytest

from tests.test_gpu_parity import make_pair, RTOL
from tests.test_gpu_sweeps import CLASSES, ids, _model
from tests.test_gpu_scan import gapped_stream
from tests.variant_reference import variant_effects, variant_list, check

pytestmark = pytest.mark.gpu

SERVED = [CLASSES[0], CLASSES[1], CLASSES[2], CLASSES[3]]
T_A, SEED = 5003, 2031
KEYS = ("dfe", "per_motif", "windows")


def per_variant(cls):
    """bytes the driver counts per variant (crbm_sweep.h, variant_plan)"""
    name, K, M, ds, A, pool, Lf, L, env, spec = cls
    CW = 2 * M - 1
    return CW + (3 * CW + 7) // 8 + 4 * (K + 2) + 1


def _same(a, b, label=""):
    for key in KEYS:
        assert a[key].dtype == b[key].dtype and a[key].tobytes() == b[key].tobytes(), (label, key)


def _c_call(m, stream, pos, alt, K, want=KEYS, fill=77, T=None, nvar=None):
    """crbm_variant_effects_codes with the outputs in `want` (the others NULL): (rc, outputs pre-filled with `fill`)"""
    from crbm_amd import _lib
    V = len(pos)
    out = {"dfe": np.full(V, fill, np.float32), "per_motif": np.full((V, K), fill, np.float32), "windows": np.full(V, fill, np.int32)}
    pos, alt = np.ascontiguousarray(pos, np.int64), np.ascontiguousarray(alt, np.uint8)
    p = lambda key, ty: out[key].ctypes.data_as(ty) if key in want else None
    rc = m._lib.crbm_variant_effects_codes(m._h(), stream.ctypes.data_as(_lib._U8P), stream.size if T is None else T,
                                           V if nvar is None else nvar, pos.ctypes.data_as(_lib._I64P), alt.ctypes.data_as(_lib._U8P),
                                           p("dfe", _lib._F), p("per_motif", _lib._F), p("windows", _lib._I32P))
    return rc, out


@pytest.mark.parametrize("cls", SERVED, ids=ids(SERVED))
def test_variants_against_reference_and_the_same_bits_for_every_chunking(cls, monkeypatch):
    name, K, M, ds, A, pool, Lf, L, env, spec = cls
    m, o = _model(cls, monkeypatch)
    stream = gapped_stream(T_A, SEED)
    pos, alt = variant_list(stream, M, 2000, 77)
    V = pos.size
    want = variant_effects(o, stream, pos, alt)
    w = want["windows"]
    assert (w == M).any() and (w == 0).any() and (M == 1 or ((0 < w) & (w < M)).any())      # every branch is met
    monkeypatch.delenv("CRBM_SLAB_BYTES", raising=False)
    got = m.variantEffects(stream, pos, alt)                                                # one chunk
    assert got["dfe"].shape == (V,) and got["per_motif"].shape == (V, K) and got["windows"].shape == (V,)
    check(got, want, RTOL, name)
    _same(got, m.variantEffects(stream, pos, alt), "second run")
    chunk = V // 7 + 1
    assert -(-V // chunk) == 7
    monkeypatch.setenv("CRBM_SLAB_BYTES", str(per_variant(cls) * chunk))
    _same(got, m.variantEffects(stream, pos, alt), "7 chunks")
    monkeypatch.setenv("CRBM_SLAB_BYTES", "1")
    _same(got, m.variantEffects(stream, pos, alt), "one variant a chunk")
    monkeypatch.setenv("CRBM_SLAB_BYTES", str(per_variant(cls) * 301))
    perm = np.random.default_rng(5).permutation(V)
    shuffled = m.variantEffects(stream, pos[perm], alt[perm])
    _same({k: got[k][perm] for k in KEYS}, shuffled, "permuted")


@pytest.mark.parametrize("cls", [CLASSES[0], CLASSES[3]], ids=ids([CLASSES[0], CLASSES[3]]))
def test_every_output_alone_gives_the_same_bits(cls, monkeypatch):
    name, K, M, ds, A, pool, Lf, L, env, spec = cls
    m, o = _model(cls, monkeypatch)
    stream = gapped_stream(T_A, SEED)
    pos, alt = variant_list(stream, M, 500, 78)
    monkeypatch.setenv("CRBM_SLAB_BYTES", str(per_variant(cls) * 200))
    rc, full = _c_call(m, stream, pos, alt, K)
    assert rc == 0
    check(full, variant_effects(o, stream, pos, alt), RTOL, name)
    for key in KEYS:
        rc, one = _c_call(m, stream, pos, alt, K, want=(key,))
        assert rc == 0 and one[key].tobytes() == full[key].tobytes(), key
        assert all(np.all(one[other] == 77) for other in KEYS if other != key)             # the NULL outputs' stand-ins: untouched


@pytest.mark.parametrize("cls", [CLASSES[0], CLASSES[2]], ids=ids([CLASSES[0], CLASSES[2]]))
def test_gap_free_rows_agree_with_mutagenesis(cls, monkeypatch):
    """rows written as a stream with separators: dfe of (row n, position p, letter a) against mutagenesis(codes)[n, p, a]
    within the tolerance (both are within it of the oracle), and per_motif.sum(1) minus the bias term against dfe"""
    name, K, M, ds, A, pool, Lf, L, env, spec = cls
    m, o = _model(cls, monkeypatch)
    monkeypatch.delenv("CRBM_SLAB_BYTES", raising=False)
    n, L = 5, min(L, 90)
    codes = np.random.default_rng(3).integers(0, 4, size=(n, L), dtype=np.uint8)
    stream = np.concatenate([codes, np.full((n, 1), 4, np.uint8)], axis=1).ravel()[:-1].copy()
    row, p, a = np.repeat(np.arange(n), L * 4), np.tile(np.repeat(np.arange(L), 4), n), np.tile(np.arange(4), n * L).astype(np.uint8)
    got = m.variantEffects(stream, row * (L + 1) + p, a)
    mut = m.mutagenesis(codes)[row, p, a].astype(np.float64)
    for label, x, ref in (("mutagenesis", got["dfe"].astype(np.float64), mut),
                          ("sum of per_motif", got["per_motif"].astype(np.float64).sum(axis=1) - (o.c.ravel()[a] - o.c.ravel()[codes[row, p]]),
                           got["dfe"].astype(np.float64))):
        err, bound = np.abs(x - ref), RTOL * np.abs(ref) + RTOL * np.abs(ref).max()
        print("%s vs dfe: max err %.3g, max|dfe| %.4g" % (label, err.max(), np.abs(ref).max()))
        assert np.all(err <= bound), label
    assert np.all(got["dfe"][a == codes[row, p]] == 0.0)
    # seq / offsets: the same variants by record
    by_record = m.variantEffects(stream, p, a, offsets=np.arange(n + 1) * (L + 1), seq=row, ref=codes[row, p])
    _same(got, by_record)


@pytest.mark.parametrize("cls", [CLASSES[0], CLASSES[2]], ids=ids([CLASSES[0], CLASSES[2]]))
def test_an_inserted_gap_removes_the_windows_that_cover_it_and_nothing_else(cls, monkeypatch):
    name, K, M, ds, A, pool, Lf, L, env, spec = cls
    m, o = _model(cls, monkeypatch)
    monkeypatch.delenv("CRBM_SLAB_BYTES", raising=False)
    stream = np.random.default_rng(8).integers(0, 4, size=600, dtype=np.uint8)
    pos = np.arange(600, dtype=np.int64)
    alt = ((stream + 1 + pos % 3) % 4).astype(np.uint8)
    before = m.variantEffects(stream, pos, alt)
    assert np.all(before["windows"][M - 1:600 - M + 1] == M)
    p = 300
    for d in (1, M // 2 + 1, M - 1, -1, -(M - 1)):
        g = p + d
        gapped = stream.copy()
        gapped[g] = 4
        after = m.variantEffects(gapped, pos, alt)
        # a variant at distance e = |pos - g| < M loses the M - e windows that cover both; the gap itself loses all
        e = np.abs(pos - g)
        lost = np.where(e < M, M - e, 0)
        assert np.array_equal(before["windows"] - after["windows"], np.minimum(lost, before["windows"])), d
        far = e > M - 1
        _same({k: before[k][far] for k in KEYS}, {k: after[k][far] for k in KEYS}, d)
        check(after, variant_effects(o, gapped, pos, alt), RTOL, "%s gap at %+d" % (name, d))
        assert after["dfe"][g] == 0.0 and after["windows"][g] == 0


def test_refusals_leave_outputs_untouched_and_the_handle_usable(monkeypatch):
    from crbm_amd import _lib
    stream = gapped_stream(400, 3)
    pos, alt = variant_list(stream, 15, 50, 4)
    for cls in (CLASSES[4], CLASSES[7], CLASSES[6]):                # pooled, 20 letters, motifs beyond 64 letters
        name, K, M, ds, A, pool, Lf, L, env, spec = cls
        m, o = _model(cls, monkeypatch)
        rc, out = _c_call(m, stream, pos, alt, K)
        assert rc == _lib.ERR_INVALID and all(np.all(out[k] == 77) for k in KEYS), name
        with pytest.raises(Exception, match="pooling|alphabet|generic"):
            m.variantEffects(stream, pos, alt)
    name, K, M, ds, A, pool, Lf, L, env, spec = CLASSES[0]
    m, o = _model(CLASSES[0], monkeypatch)
    monkeypatch.setenv("CRBM_SLAB_BYTES", str(per_variant(CLASSES[0]) * 20))
    good = m.variantEffects(stream, pos, alt)
    check(good, variant_effects(o, stream, pos, alt), RTOL, "before the refusals")
    bad_pos, bad_alt, bad_code = pos.copy(), alt.copy(), stream.copy()
    bad_pos[-1] = stream.size
    bad_alt[-1] = 4
    bad_code[399] = 5                                               # read by no context of the first chunks
    cases = {"pos = T": (stream, bad_pos, alt, {}), "pos < 0": (stream, -bad_pos - 1, alt, {}), "alt = 4": (stream, pos, bad_alt, {}),
             "a code 5": (bad_code, pos, alt, {}), "all outputs NULL": (stream, pos, alt, {"want": ()}),
             "nvar < 0": (stream, pos, alt, {"nvar": -1}), "T < 0": (stream, pos, alt, {"T": -1}),
             "T = 2^31": (stream, pos, alt, {"T": 2 ** 31})}
    for what, (s, p, a, kw) in cases.items():
        rc, out = _c_call(m, s, p, a, K, **kw)
        assert rc == _lib.ERR_INVALID and all(np.all(out[k] == 77) for k in KEYS), what
        _same(good, m.variantEffects(stream, pos, alt), what)
    rc, out = _c_call(m, stream, pos, alt, K, nvar=0)              # nvar == 0 succeeds and writes nothing
    assert rc == 0 and all(np.all(out[k] == 77) for k in KEYS)


def test_a_parameter_change_between_two_calls_is_seen_by_the_second(monkeypatch):
    m, o = _model(CLASSES[0], monkeypatch)
    monkeypatch.delenv("CRBM_SLAB_BYTES", raising=False)
    stream = gapped_stream(1200, 6)
    pos, alt = variant_list(stream, 15, 400, 9)
    first = m.variantEffects(stream, pos, alt)
    check(first, variant_effects(o, stream, pos, alt), RTOL, "before")
    W = (o.W * 0.5).astype(np.float32)
    b = (o.b - 1.0).astype(np.float32)
    c = (o.c + np.array([[0.3, -0.2, 0.1, 0.0]])).astype(np.float32)
    m.motifs.set_value(W)
    m.bias.set_value(b)
    m.c.set_value(c)
    o.W, o.b, o.c = W.astype(np.float64), b.astype(np.float64), c.astype(np.float64)
    second = m.variantEffects(stream, pos, alt)
    check(second, variant_effects(o, stream, pos, alt), RTOL, "after")
    assert np.abs(second["dfe"] - first["dfe"]).max() > 0.1


def test_variants_scale_cfg2_two_to_the_20_on_two_to_the_24():
    """config #2's double-stranded model, 2^20 random variants on 2^24 letters with gap runs: finite outputs, the first
    and the last 256 variants against the reference, and a repeat with the same bits"""
    K, M = 10, 15
    T, V = 1 << 24, 1 << 20
    m, o = make_pair(K, M, ds=True, Lf=186, bshift=3.0, wscale=0.7)
    stream = gapped_stream(T, 99, share=0.01, run=500)
    rng = np.random.default_rng(17)
    pos, alt = rng.integers(0, T, size=V), rng.integers(0, 4, size=V).astype(np.uint8)
    got = m.variantEffects(stream, pos, alt)
    assert np.all(np.isfinite(got["dfe"])) and np.all(np.isfinite(got["per_motif"]))
    assert got["windows"].min() == 0 and got["windows"].max() == M
    for sl in (slice(0, 256), slice(V - 256, V)):
        check({k: got[k][sl] for k in KEYS}, variant_effects(o, stream, pos[sl], alt[sl]), RTOL, "scale")
    _same(got, m.variantEffects(stream, pos, alt), "repeat")
