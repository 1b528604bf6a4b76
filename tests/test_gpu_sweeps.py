"""The evaluation side at scale, against the float64 oracle: freeEnergy, motifHitProbs, motifHitSummary, _evaluateData
and crbm_eval_epoch_resident on every model class that takes a route of its own through crbm_api.hip -- streamed in
several slabs over the two streams of a host-input sweep (free_energy_any / hit_summary_any), from host one-hot arrays,
host letter codes and resident row ranges -- and past the launch caps of the evaluation and h|v kernels (row counts
where the grid-stride loops and several rows per tile begin).  Also the chain launch of crbm_time_gibbs after a
parameter change (the partitions must wait for the tables the main stream rebuilds).
"""
import ctypes

import numpy as np
import pytest

from oracle.crbm_oracle import OracleCRBM, synthetic_onehot
from tests.test_gpu_parity import make_pair, _unpack_sums, assert_chain_steps, RTOL, _cfg2_model

pytestmark = pytest.mark.gpu

# model classes and the routes they take (crbm_api.hip):
#   free energy: specialised free_energy / slab_launch_fe (+ slab_fe_combine_kernel) / big_eval_kernel
#   hit probabilities and summaries: specialised hgv and hit_summary / big_hgv and big_eval_kernel
#   _evaluateData's sample count: specialised hgv / slab_launch_hgv / big_hgv
# (name, K, M, ds, A, pool, Lf, L, env, specialised)
CLASSES = [
    ("spec_10x15_ds", 10, 15, True, 4, 1, 200, 200, {}, True),
    ("spec_20x15_ds_L1200", 20, 15, True, 4, 1, 200, 1200, {}, True),        # several position chunks (hit summary)
    ("slab_300x10_ss", 300, 10, False, 4, 1, 51, 60, {}, False),              # 5 slabs of 60 motifs
    ("slab_257x1_ss", 257, 1, False, 4, 1, 12, 40, {}, False),                # last slab moved back to end at K
    ("slab_150x6_ds_pool2", 150, 6, True, 4, 2, 24, 45, {}, False),
    ("slab_300x10_ss_nofe", 300, 10, False, 4, 1, 51, 60, {"CRBM_SLAB_FE": "0"}, False),   # big_eval_kernel
    ("big_8x100_ds", 8, 100, True, 4, 1, 200, 140, {}, False),                # motifs beyond 64 letters
    ("alpha20_12x9_ss", 12, 9, False, 20, 1, 200, 40, {}, False),             # other alphabets: encode_*_any_kernel
    ("alpha5_7x6_ds_pool2", 7, 6, True, 5, 2, 200, 47, {}, False),
]
ids = lambda cs: [c[0] for c in cs]


def _model(cls, monkeypatch, **kw):
    name, K, M, ds, A, pool, Lf, L, env, spec = cls
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    extra = {}
    if A != 4:
        extra["input_dims"] = A
    if pool > 1:
        extra["pooling"] = pool
    extra.update(kw)
    m, o = make_pair(K, M, ds=ds, Lf=Lf, bshift=3.0, wscale=0.7, **extra)
    _assert_route(m, spec)
    return m, o


def _assert_route(m, spec):
    """specialised kernels or the generic path (gibbs_grid == 0 there): no case may silently take the other one"""
    from crbm_amd import _lib
    info = _lib.CrbmLaunchInfo()
    h = m._h()
    m._check(m._lib.crbm_get_launch_info(h, ctypes.byref(info)))
    assert (info.gibbs_grid > 0) == spec


def _codes(n, L, A, seed):
    return np.random.default_rng(seed).integers(0, A, size=(n, L), dtype=np.uint8)


def _onehot(codes, A):
    return np.ascontiguousarray(np.eye(A, dtype=np.float32)[codes].transpose(0, 2, 1)[:, None])


def _budget(monkeypatch, per_row, rows):
    """CRBM_SLAB_BYTES for slabs of `rows` rows of a call whose bytes per row (input + outputs: crbm_api.hip, sweep_slab /
    slab_rows) are `per_row`; None: the default budget (read on every call)"""
    if rows is None:
        monkeypatch.delenv("CRBM_SLAB_BYTES", raising=False)
    else:
        monkeypatch.setenv("CRBM_SLAB_BYTES", str(per_row * rows))


def _in_bytes(src, A, L):
    return {"onehot": 4 * A * L, "codes": L, "resident": 0}[src]


def _fe(m, src, data, codes, lo):
    """(fe, fe_per_motif) of all rows of a source in ONE call each"""
    from crbm_amd._lib import fptr
    n, K = codes.shape[0], m.num_motifs
    if src == "resident":
        fe, fem = np.empty(n, np.float32), np.empty((n, K), np.float32)
        m._call("crbm_free_energy_resident", lo, lo + n, fptr(fe), fptr(fem))
        return fe, fem
    x = data if src == "onehot" else codes
    return m.freeEnergy(x), m.freeEnergy(x, True)


def _hits(m, src, data, codes, lo):
    """(hit probabilities, hit summary dict)"""
    from crbm_amd._lib import fptr
    n, K, Lh = codes.shape[0], m.num_motifs, codes.shape[1] - m.motif_length + 1
    if src == "resident":
        hp = np.empty((n, K, 1, Lh), np.float32)
        m._call("crbm_hit_probs_resident", lo, lo + n, fptr(hp))
        mx, mean, pos = np.empty((n, K), np.float32), np.empty((n, K), np.float32), np.empty((K, Lh), np.float32)
        m._call("crbm_hit_summary_resident", lo, lo + n, fptr(mx), fptr(mean), fptr(pos))
        return hp, {"max": mx, "mean": mean, "position_mean": pos}
    x = data if src == "onehot" else codes
    return m.motifHitProbs(x), m.motifHitSummary(x)


def _check_oracle(o, data, fe, fem, hp=None, summ=None, chunk=1000):
    """every output against the float64 oracle (RTOL, the atols of check_model_against_oracle), in row chunks"""
    n = data.shape[0]
    pos = 0.0
    for a in range(0, n, chunk):
        D = data[a:a + chunk]
        np.testing.assert_allclose(fe[a:a + chunk], o.freeEnergy(D), rtol=RTOL, atol=1e-6)
        np.testing.assert_allclose(fem[a:a + chunk], o.freeEnergy(D, True), rtol=RTOL, atol=2e-5)
        if hp is None and summ is None:
            continue
        P = o.motifHitProbs(D)
        if hp is not None:
            np.testing.assert_allclose(hp[a:a + chunk], P, rtol=RTOL, atol=1e-7)
        if summ is not None:
            np.testing.assert_allclose(summ["max"][a:a + chunk], P.max(axis=(2, 3)), rtol=RTOL, atol=1e-7)
            np.testing.assert_allclose(summ["mean"][a:a + chunk], P.mean(axis=(2, 3)), rtol=RTOL, atol=1e-7)
            pos = pos + P.sum(axis=(0, 2))
    if summ is not None:
        np.testing.assert_allclose(summ["position_mean"], pos / n, rtol=RTOL, atol=1e-7)


# ---- A. sweeps over several slabs, every source, every model class -------------------------------------------------
@pytest.mark.parametrize("cls", CLASSES, ids=ids(CLASSES))
def test_sweep_sources_and_slabs(cls, monkeypatch):
    """Host one-hot, host codes and a resident range inside a larger set, each in one slab and in >= 6 slabs with a short
    last one (slab i on stream i & 1): the row-local outputs (free energies per sequence and per motif, hit probabilities,
    hit max) are the same bits everywhere; hit means are the same bits in a repeat and agree across splits to 1e-5 (the
    mean of a row is summed per position chunk and combined); the multi-slab run matches the oracle; _evaluateData in
    slabs equals the one-slab call (rows keep their global sampler index) and the oracle's sample."""
    name, K, M, ds, A, pool, Lf, L, env, spec = cls
    n, lo = 200, 7
    m, o = _model(cls, monkeypatch)
    allc = _codes(n + 19, L, A, seed=K + M)
    codes = np.ascontiguousarray(allc[lo:lo + n])
    data = _onehot(codes, A)
    m._upload(allc, 0)
    m._call("crbm_dataset_select", 0)
    rows = -(-n // 7)                                     # 7 slabs: 6 of 29 rows, the last of 26
    Lh = L - M + 1
    res = {}
    for src in ("onehot", "codes", "resident"):
        for multi in (False, True):
            _budget(monkeypatch, _in_bytes(src, A, L) + (K + 1) * 4, rows if multi else None)
            fe, fem = _fe(m, src, data, codes, lo)
            _budget(monkeypatch, _in_bytes(src, A, L) + K * Lh * 4, rows if multi else None)
            hp = _hits(m, src, data, codes, lo)[0]
            _budget(monkeypatch, _in_bytes(src, A, L) + 2 * K * 4, rows if multi else None)
            s = _hits(m, src, data, codes, lo)[1]
            again = _hits(m, src, data, codes, lo)[1]
            for key in s:
                np.testing.assert_array_equal(s[key], again[key], err_msg=key)       # a repeat: the same bits
            res[src, multi] = (fe, fem, hp, s)
    fe0, fem0, hp0, s0 = res["onehot", False]
    for key, (fe, fem, hp, s) in res.items():
        np.testing.assert_array_equal(fe, fe0, err_msg=str(key))
        np.testing.assert_array_equal(fem, fem0, err_msg=str(key))
        np.testing.assert_array_equal(hp, hp0, err_msg=str(key))
        np.testing.assert_array_equal(s["max"], s0["max"], err_msg=str(key))
        np.testing.assert_allclose(s["mean"], s0["mean"], rtol=1e-5, atol=0, err_msg=str(key))
        np.testing.assert_allclose(s["position_mean"], s0["position_mean"], rtol=1e-5, atol=0, err_msg=str(key))
    fe, fem, hp, s = res["codes", True]
    _check_oracle(o, data, fe, fem, hp, s)
    # evaluateData (one-hot input only), one slab and several: same sampler step, rows keep their index within the call
    _budget(monkeypatch, _in_bytes("onehot", A, L) + (K + 1) * 4, None)
    m.set_rng(gibbs_step=0, eval_step=3)
    one = m._evaluateData(data)
    _budget(monkeypatch, _in_bytes("onehot", A, L) + (K + 1) * 4, rows)
    m.set_rng(gibbs_step=0, eval_step=3)
    many = m._evaluateData(data)
    assert many[1] == one[1] and many[1] > 0
    assert abs(many[0] - one[0]) <= 1e-6 * abs(one[0])
    want = o.evaluateData(data.astype(np.float64), eval_step=3)
    assert abs(many[0] - want[0]) <= RTOL * abs(want[0]) + 1e-6
    assert abs(many[1] - want[1]) <= 2.0 / (n * K * Lh)                       # a p == u tie may decide differently


@pytest.mark.parametrize("cls", CLASSES, ids=ids(CLASSES))
def test_multi_slab_free_energy_is_the_same_bits_in_every_run(cls, monkeypatch):
    """The regression test of the slab free-energy race (two streams writing one per-motif scratch, slab tables read
    by the second stream while the first builds them): slabs of 300 rows, so that the two streams' kernels overlap,
    three runs on one handle right after a parameter change -- all the same bits as the one-slab call."""
    name, K, M, ds, A, pool, Lf, L, env, spec = cls
    n = 1900
    m, o = _model(cls, monkeypatch)
    codes = _codes(n, L, A, seed=3 * K + M)
    data = _onehot(codes, A)
    m.bias.set_value((m.bias.get_value() - 0.5).astype(np.float32))            # the tables are stale when the sweep starts
    _budget(monkeypatch, _in_bytes("onehot", A, L) + (K + 1) * 4, 300)
    first = m.freeEnergy(data, True)
    for _ in range(2):
        np.testing.assert_array_equal(m.freeEnergy(data, True), first)
    _budget(monkeypatch, 0, None)
    np.testing.assert_array_equal(m.freeEnergy(data, True), first)
    o.b = m.bias.get_value().astype(np.float64)
    np.testing.assert_allclose(first[:64], o.freeEnergy(data[:64], True), rtol=RTOL, atol=2e-5)
    np.testing.assert_allclose(first[-64:], o.freeEnergy(data[-64:], True), rtol=RTOL, atol=2e-5)


@pytest.mark.parametrize("cls", CLASSES, ids=ids(CLASSES))
def test_sweep_after_parameter_change_and_resize(cls, monkeypatch):
    """A multi-slab sweep, new motifs and biases, another multi-slab sweep: the numbers of the new parameters (stale
    d_tables / d_slab_tables would show).  Then n = 600, 50, 900 on the same handle, in one slab (the buffers grow
    between calls) and in several: every result against the oracle."""
    name, K, M, ds, A, pool, Lf, L, env, spec = cls
    m, o = _model(cls, monkeypatch)
    codes = _codes(900, L, A, seed=K + 2 * M)
    data = _onehot(codes, A)
    fe_row = _in_bytes("onehot", A, L) + (K + 1) * 4
    hit_row = _in_bytes("onehot", A, L) + 2 * K * 4
    _budget(monkeypatch, fe_row, 23)
    m.freeEnergy(data[:150], True)
    rng = np.random.default_rng(K * M)
    W2 = (rng.standard_normal((K, 1, A, M)) * 0.6).astype(np.float32)
    b2 = (m.bias.get_value() + rng.uniform(-1.0, 0.5, size=(1, K))).astype(np.float32)
    m.motifs.set_value(W2)
    m.bias.set_value(b2)
    o.W, o.b = W2.astype(np.float64), b2.astype(np.float64)
    fe, fem = m.freeEnergy(data[:150]), m.freeEnergy(data[:150], True)
    _budget(monkeypatch, hit_row, 23)
    _check_oracle(o, data[:150], fe, fem, summ=m.motifHitSummary(data[:150]))
    for multi in (False, True):
        for n in (600, 50, 900):
            _budget(monkeypatch, fe_row, 97 if multi else None)
            fe, fem = m.freeEnergy(data[:n]), m.freeEnergy(codes[:n], True)
            _budget(monkeypatch, hit_row, 97 if multi else None)
            _check_oracle(o, data[:n], fe, fem, summ=m.motifHitSummary(data[:n]))


@pytest.mark.parametrize("cls", CLASSES, ids=ids(CLASSES))
def test_validity_flags_across_streams(cls, monkeypatch):
    """A row that is not one-hot, or a letter code >= A, in an odd-numbered slab (the second stream) or in the short last
    slab fails the call with 'one-hot'; the next valid call on the handle succeeds with the right numbers (d_flags was
    reset)."""
    name, K, M, ds, A, pool, Lf, L, env, spec = cls
    n, rows = 130, 20                                        # 7 slabs, the last one of 10 rows
    m, o = _model(cls, monkeypatch)
    codes = _codes(n, L, A, seed=K + 5 * M)
    data = _onehot(codes, A)
    fe_ref = m.freeEnergy(codes, True)
    s_ref = m.motifHitSummary(codes)
    for row in (rows * 3 + 5, n - 2):                        # slab 3 (odd: stream 2), the last slab
        bad_d = data.copy()
        bad_d[row, 0, 0, L // 2] = 1.0 - bad_d[row, 0, 0, L // 2]
        bad_c = codes.copy()
        bad_c[row, L - 1] = A
        for kind, bad in (("onehot", bad_d), ("codes", bad_c)):
            if kind == "codes" and A >= 255:
                continue
            _budget(monkeypatch, _in_bytes(kind, A, L) + (K + 1) * 4, rows)
            with pytest.raises(Exception, match="one-hot"):
                m.freeEnergy(bad, True)
            np.testing.assert_array_equal(m.freeEnergy(codes, True), fe_ref)
            _budget(monkeypatch, _in_bytes(kind, A, L) + 2 * K * 4, rows)
            with pytest.raises(Exception, match="one-hot"):
                m.motifHitSummary(bad)
            s = m.motifHitSummary(codes)
            np.testing.assert_array_equal(s["max"], s_ref["max"])
            np.testing.assert_allclose(s["mean"], s_ref["mean"], rtol=1e-5, atol=0)
    _check_oracle(o, data, m.freeEnergy(data), m.freeEnergy(data, True))


@pytest.mark.parametrize("cls", CLASSES, ids=ids(CLASSES))
def test_epoch_evaluation_is_the_loop_over_batches(cls, monkeypatch):
    """crbm_eval_epoch_resident with a short last batch: bit for bit the loop over crbm_eval_data_resident."""
    name, K, M, ds, A, pool, Lf, L, env, spec = cls
    m, o = _model(cls, monkeypatch)
    codes = _codes(130, L, A, seed=K + 7 * M)                  # 7 mini-batches of 20, the last one of 10 rows
    m._upload(codes, 0)
    m._call("crbm_dataset_select", 0)
    m.set_rng(gibbs_step=0, eval_step=5)
    mfe, nmh = ctypes.c_float(), ctypes.c_float()
    sfe = snmh = 0.0
    nb = 0
    for start in range(0, 130, 20):
        m._call("crbm_eval_data_resident", start, min(start + 20, 130), ctypes.byref(mfe), ctypes.byref(nmh))
        sfe, snmh, nb = sfe + mfe.value, snmh + nmh.value, nb + 1
    assert m.get_rng()[2] == 5 + nb
    m.set_rng(gibbs_step=0, eval_step=5)
    a, b = ctypes.c_double(), ctypes.c_double()
    m._call("crbm_eval_epoch_resident", 20, ctypes.byref(a), ctypes.byref(b))
    assert a.value == sfe / nb and b.value == snmh / nb
    assert b.value > 0 and m.get_rng()[2] == 5 + nb
    want = np.mean([o._meanFreeEnergy(_onehot(codes[s:s + 20], A).astype(np.float64)) for s in range(0, 130, 20)])
    assert abs(a.value - want) <= RTOL * abs(want) + 1e-6


# ---- B. past the launch caps ---------------------------------------------------------------------------------------
CAPS = [c for c in CLASSES if c[0] in ("spec_10x15_ds", "slab_300x10_ss", "big_8x100_ds")]


@pytest.mark.parametrize("cls", CAPS, ids=ids(CAPS))
def test_evaluation_past_the_launch_caps(cls, monkeypatch):
    """9000 rows in one call (host codes and a resident set): past big_eval_kernel's 8 x CUs blocks (n > 2048), the
    slab and specialised free-energy grids' ~8192 rows and the specialised hit-summary grid -- every row of the free
    energies, hit probabilities and hit summary against the oracle."""
    name, K, M, ds, A, pool, Lf, L, env, spec = cls
    L = M + 30
    n = 9000
    m, o = _model(cls, monkeypatch)
    codes = _codes(n, L, A, seed=K + 11 * M)
    data = _onehot(codes, A)
    m._upload(codes, 0)
    m._call("crbm_dataset_select", 0)
    fe, fem = _fe(m, "codes", data, codes, 0)
    rfe, rfem = _fe(m, "resident", data, codes, 0)
    np.testing.assert_array_equal(rfe, fe)
    np.testing.assert_array_equal(rfem, fem)
    hp, s = _hits(m, "resident", data, codes, 0)
    hs = m.motifHitSummary(codes)
    np.testing.assert_array_equal(hs["max"], s["max"])
    np.testing.assert_allclose(hs["mean"], s["mean"], rtol=1e-5, atol=0)
    _check_oracle(o, data, fe, fem, hp, s, chunk=500)
    # the last rows once more, one row per call (a row's numbers do not depend on where the grid put it)
    for r in (n - 1, n - 5, 8191, 2047):
        np.testing.assert_array_equal(m.freeEnergy(codes[r:r + 1], True)[0], fem[r])
        np.testing.assert_array_equal(m.motifHitSummary(codes[r:r + 1])["max"][0], s["max"][r])


@pytest.mark.parametrize("K,M,ds,B,Lf", [(300, 10, False, 512, 30), (120, 40, True, 256, 24), (8, 100, False, 1100, 31)])
def test_chains_and_statistics_with_several_rows_per_tile(K, M, ds, B, Lf):
    """Generic DNA models at batch sizes where the slabbed h|v (n x slabs > 4 x CUs) and the big h|v (TS > 1) put
    several rows in one tile: two Gibbs steps sample for sample against the oracle (ties only), then the packed raw
    sums of one crbm_train_local against OracleCRBM.local_sums (test_slabbed_statistics_of_generic_models' tolerances)."""
    from crbm_amd import CRBM
    from crbm_amd._lib import fptr
    m, o = make_pair(K, M, ds=ds, batchsize=B, Lf=Lf, cd_k=2, bshift=3.0, wscale=0.6)
    _assert_route(m, False)
    assert_chain_steps(m, o, 2)
    n, L = 10, Lf + M - 1
    W = (np.random.default_rng(K + M).standard_normal((K, 1, 4, M)) * 0.6).astype(np.float32)
    D = synthetic_onehot(n, L, seed=17)
    m = CRBM(K, M, doublestranded=ds, batchsize=B, cd_k=2, fantasy_hidden_len=Lf, seed=9, rho=0.02)
    m.motifs.set_value(W)
    m.bias.set_value((m.bias.get_value() + 3.0).astype(np.float32))
    h = m._h()
    buf = np.zeros(m._lib.crbm_sums_count(h), dtype=np.float32)
    m._call("crbm_train_local", fptr(D), n, L, fptr(buf))
    got = _unpack_sums(buf, K, M)
    assert got["n_d"] == n and got["n_m"] == B
    o = OracleCRBM(K, M, doublestranded=ds, batchsize=B, cd_k=2, fantasy_hidden_len=Lf, seed=9, rho=0.02, W=W)
    o.b = m.bias.get_value().astype(np.float64)
    P_m, P_mp, v_m = o.gibbs_steps(2)
    h1, h1p = m.get_fantasy()
    want = o.local_sums(D, P_m, P_mp, v_m)
    keys = ("vh_d", "h_d", "sw", "sb", "v_d") + (("vh_dp", "h_dp") if ds else ())          # the data half: no chain in it
    if np.array_equal(h1, o.fantasy_h) and (not ds or np.array_equal(h1p, o.fantasy_h_prime)):
        keys += ("vh_m", "h_m", "v_m") + (("vh_mp", "h_mp") if ds else ())               # (a tie on the way: the chains differ)
    for key in keys:
        atol = 1e-5 + (1.6e-6 * float(np.abs(want[key]).max()) if key.startswith(("vh", "sw")) else 0.0)
        np.testing.assert_allclose(got[key], np.ravel(want[key]), rtol=RTOL, atol=atol, err_msg=key)


# ---- crbm_time_gibbs after a parameter change ----------------------------------------------------------------------
def test_time_gibbs_waits_for_the_tables_after_set_params():
    """Config #2 at 8192 chains goes out in chain partitions on streams of their own.  After crbm_set_params the main
    stream rebuilds the tables inside the first launch of crbm_time_gibbs; the partitions must wait for them: the chain
    is the same bits as gibbsSteps(2) after the same change (and the step counter moves the same), and its first 32
    chains follow the oracle of the new parameters (ties only)."""
    from crbm_amd import _lib
    B = 8192
    W2 = (np.random.default_rng(77).standard_normal((10, 1, 4, 15)) * 1.2).astype(np.float32)
    a = _cfg2_model(B)
    info = _lib.CrbmLaunchInfo()
    a._check(a._lib.crbm_get_launch_info(a._h(), ctypes.byref(info)))
    assert info.chain_parts > 1
    a.motifs.set_value(W2)
    ms = ctypes.c_float()
    a._call("crbm_time_gibbs", 1, 2, ctypes.byref(ms))
    b = _cfg2_model(B)
    b.motifs.set_value(W2)
    b.gibbsSteps(2)
    assert a.get_rng()[1] == b.get_rng()[1] == 2
    ha = a.get_fantasy()[0]
    np.testing.assert_array_equal(ha, b.get_fantasy()[0])
    small = _cfg2_model(32)
    small.motifs.set_value(W2)
    small.gibbsSteps(2)
    np.testing.assert_array_equal(small.get_fantasy()[0], ha[:32])
    o = OracleCRBM(10, 15, doublestranded=False, batchsize=32, cd_k=1, fantasy_hidden_len=186, seed=2026, W=W2)
    twin = _cfg2_model(32)
    twin.motifs.set_value(W2)
    if assert_chain_steps(twin, o, 2) == 0:                 # no tie met: the oracle's chain is the handle's
        np.testing.assert_array_equal(ha[:32], o.fantasy_h)


# ---- crbm_create takes the plan crbm_precompile compiled for (crbm_plan.h) -----------------------------------------------
# (K, M, ds, batchsize, Lf) of models __graft_entry__.build() precompiles: plain, partitioned, slabbed generic; config #5
# at 8192 chains for the recorded plan
PLAN_SHAPES = [(10, 15, 0, 20, 200), (10, 15, 0, 8192, 186), (300, 10, 0, 20, 51)]
PLAN_IDS = ["plain", "partitioned", "slabbed_generic"]


def _create(K, M, ds, B, Lf):
    """a bare handle of the model, configured as crbm_amd.csrc.build.precompile configures it"""
    from crbm_amd import _lib
    lib = _lib.load()
    cfg = _lib.CrbmConfig(num_motifs=K, motif_length=M, input_dims=4, doublestranded=ds, batchsize=B, cd_k=1, pooling=1,
                          fantasy_hidden_len=Lf, learning_rate=0.1, momentum=0.9, rho=0.01, lambda_rate=0.1, seed=0, device=0,
                          reserved=0)
    h = ctypes.c_void_p()
    assert lib.crbm_create(ctypes.byref(cfg), ctypes.byref(h)) == 0, lib.crbm_last_error(None).decode()
    return lib, h


@pytest.mark.parametrize("shape", PLAN_SHAPES, ids=PLAN_IDS)
def test_create_takes_the_precompiled_code_objects(shape):
    """The JIT cache is keyed by what the launch plan chooses (letter groupings, occupancy hint, block bound, slab model):
    a handle of a precompiled model must find its code object in the in-tree cache -- creating it adds no file there."""
    import os
    from crbm_amd import _lib
    for knob in ("CRBM_JIT_CACHE", "CRBM_JIT_DEFINES", "CRBM_JIT_NOCACHE"):
        if os.environ.get(knob):
            pytest.skip(knob + " is set: handles do not take the in-tree cache as the build left it")
    cache = os.path.join(os.path.dirname(os.path.abspath(_lib.__file__)), "csrc", "jit_cache")
    before = sorted(os.listdir(cache))
    assert before, "the build leaves the precompiled code objects in " + cache
    lib, h = _create(*shape)
    lib.crbm_destroy(h)
    assert sorted(os.listdir(cache)) == before


@pytest.mark.parametrize("shape", PLAN_SHAPES + [(20, 15, 1, 8192, 486)], ids=PLAN_IDS + ["partitioned_cfg5"])
def test_launch_info_is_the_recorded_plan(shape):
    """crbm_get_launch_info of a handle against tests/golden/launch_plans.json (recorded before crbm_plan.h existed)"""
    import json
    import os
    import torch
    from crbm_amd import _lib
    with open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "launch_plans.json")) as f:
        golden = json.load(f)
    num_cu = torch.cuda.get_device_properties(0).multi_processor_count
    if num_cu != golden["num_cu"]:
        pytest.skip("recorded on a device of %d compute units, this one has %d" % (golden["num_cu"], num_cu))
    K, M, ds, B, Lf = shape
    rows = [r["info"] for r in golden["plans"]["default"]
            if (r["config"]["num_motifs"], r["config"]["motif_length"], r["config"]["doublestranded"],
                r["config"].get("batchsize", 20), r["config"].get("fantasy_hidden_len", 200), r["config"].get("pooling", 1)) == (K, M, ds, B, Lf, 1)]
    assert len(rows) == 1
    lib, h = _create(*shape)
    info = _lib.CrbmLaunchInfo()
    assert lib.crbm_get_launch_info(h, ctypes.byref(info)) == 0
    lib.crbm_destroy(h)
    assert {f: getattr(info, f) for f in golden["fields"]} == rows[0]
