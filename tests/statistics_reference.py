"""TEST INFRASTRUCTURE of tests/test_gpu_statistics.py, pinned on the CPU by tests/test_statistics_reference.py: the packed
raw-sum buffer of crbm_train_local for any alphabet, its float64 reference, and the cases.

The reference leaves no sampling tie to excuse a difference.  The data half is OracleCRBM.local_sums on the batch.  The
model half is a function of the chains' last visible sample alone (P = h|v of that sample, on both strands): it is
rebuilt from the sample the HANDLE drew (get_fantasy_visible), so it is compared unconditionally -- whether the chain
followed the oracle's is the business of the chain tests.

A plain module: imported as tests.statistics_reference."""
import numpy as np

from oracle.crbm_oracle import synthetic_onehot

RTOL = 1e-4
DATA_KEYS = ("vh_d", "vh_dp", "h_d", "h_dp", "sw", "sb", "v_d", "n_d")
MODEL_KEYS = ("vh_m", "vh_mp", "h_m", "h_mp", "v_m", "n_m")
# the packed buffer (include/crbm_amd.h; crbm_layout.h, sums_layout): the data row, n_d, the model row without sw / sb, n_m
_DATA_ROW = (("vh_d", "KAM"), ("vh_dp", "KAM"), ("h_d", "K"), ("h_dp", "K"), ("sw", "KAM"), ("sb", "K"), ("v_d", "A"), ("n_d", 1))
_MODEL_ROW = (("vh_m", "KAM"), ("vh_mp", "KAM"), ("h_m", "K"), ("h_mp", "K"), ("v_m", "A"), ("n_m", 1))


def sums_fields(K, M, A=4):
    """[(name, offset, length)] of the packed buffer, in buffer order"""
    size = {"KAM": K * A * M, "K": K, "A": A, 1: 1}
    out, at = [], 0
    for name, n in _DATA_ROW + _MODEL_ROW:
        out.append((name, at, size[n]))
        at += size[n]
    return out


def unpack_sums(buf, K, M, A=4):
    """the packed raw-sum buffer -> dict of arrays (n_d, n_m: arrays of one element)"""
    fields = sums_fields(K, M, A)
    assert buf.shape == (fields[-1][1] + fields[-1][2],), buf.shape
    return {name: buf[at:at + n] for name, at, n in fields}


def pack_sums(d, K, M, A=4):
    return np.concatenate([np.ravel(d[name]) for name, _, _ in sums_fields(K, M, A)])


def model_half(o, v, chunk=512):
    """the model half of OracleCRBM.local_sums from the visible sample `v` (B,1,A,Lv) alone, float64; `chunk` chains at a
    time (the sliding windows of 8192 chains at once would not fit)"""
    v = np.asarray(v, dtype=np.float64)
    B = v.shape[0]
    out = {}
    for lo in range(0, B, chunk):
        vc = v[lo:lo + chunk]
        strands = (("", False),) + ((("p", True),) if o.doublestranded else ())
        part = {"v_m": vc.sum(axis=(0, 1, 3))}
        for tag, flip in strands:
            P = o._computeHgivenV(vc, flip)[0]
            part["vh_m" + tag] = o._collectVHStatistics(P, vc)[:, 0] * (P.shape[0] * P.shape[3])
            part["h_m" + tag] = P.sum(axis=(0, 2, 3))
        for k, x in part.items():
            out[k] = out[k] + x if k in out else x
    out["n_m"] = float(B)
    return out


def reference_sums(o, D, v):
    """every block of the packed buffer in float64: the data half of batch D, the model half of the visible sample v"""
    head = np.asarray(v[:1], dtype=np.float64)
    ref = o.local_sums(D, o._computeHgivenV(head)[0], o._computeHgivenV(head, True)[0] if o.doublestranded else None, head)
    ref = {k: x for k, x in ref.items() if k in DATA_KEYS}
    ref.update(model_half(o, v))
    return ref


def compared_keys(ds):
    return [k for k in DATA_KEYS + MODEL_KEYS if ds or not k.endswith("p")]


def check_conditions(o, D, ref, Lf, full_size=False):
    """What keeps the tolerances from hiding an error, on the REFERENCE: the forward-strand mean P of the batch lies in
    [0.02, 0.5]; every compared block reaches 1; and (not at full size) no sum runs over more than 4000 hidden positions,
    so one dropped or doubled position moves it by at least 1e-3 of its size -- ten times RTOL."""
    n, Lh = D.shape[0], D.shape[3] - o.motif_length + 1
    B = int(ref["n_m"])
    meanP = float(ref["h_d"].sum()) / (o.num_motifs * n * Lh)
    assert 0.02 <= meanP <= 0.5, ("mean P of the batch", meanP)
    for key in compared_keys(o.doublestranded):
        assert float(np.abs(ref[key]).max()) >= 1.0, (key, float(np.abs(ref[key]).max()))
    if not full_size:
        assert n * Lh <= 4000 and B * Lf <= 4000, (n, Lh, B, Lf)


def assert_sums(got, ref, ds, what=""):
    """vh*, sw: RTOL and the derived-fourth-letter allowance (the fourth letter of a (K,4,M) block is H - the other three when M
    is no multiple of 16, crbm_layout.h NL: its absolute error follows H, 4e-7 of the largest); h*, sb: RTOL, 1e-5; letter
    counts and normalisers exact"""
    for key in compared_keys(ds):
        want = np.ravel(ref[key])
        if key.startswith(("v_", "n_")):
            np.testing.assert_array_equal(got[key], want, err_msg="%s %s" % (what, key))
            continue
        atol = 1e-5 + (1.6e-6 * float(np.abs(want).max()) if key.startswith(("vh", "sw")) else 0.0)
        np.testing.assert_allclose(got[key], want, rtol=RTOL, atol=atol, err_msg="%s %s" % (what, key))


# ---- the cases ---------------------------------------------------------------------------------------------------------
B, LF, CD_K, RHO = 7, 33, 2, 0.03
# (K, M, ds, pool, A, bshift): the bias shift puts the mean activity of the batch inside check_conditions' window (about 5
# for motifs of 15 letters and unit weights, as in the chain tests; less for short motifs, whose bias starts higher)
MODELS = {
    "10x15ss": (10, 15, False, 1, 4, 5.0),        # fused, NL = 3, config #2's model
    "16x16ds": (16, 16, True, 1, 4, 5.0),         # fused, both strands, NL = 4
    "16x32ss": (16, 32, False, 1, 4, 5.0),        # fused, JT = 2, NL = 4
    "32x16ss": (32, 16, False, 1, 4, 5.0),        # fused, two motif tiles
    "8x12ds": (8, 12, True, 1, 4, 4.0),           # fused, packed tiles
    "20x15ds": (20, 15, True, 1, 4, 5.0),         # packed, not fused
    "33x17ss": (33, 17, False, 1, 4, 5.0),        # NR = 3 (odd tile count), JT = 2
    "64x32ds": (64, 32, True, 1, 4, 5.0),         # four roles, NL = 4
    "20x40ds": (20, 40, True, 1, 4, 5.0),         # 128-bit windows, JT = 3
    "4x64ds": (4, 64, True, 1, 4, 7.0),           # 128-bit windows, JT = 4, NL = 4
    "100x15ss": (100, 15, False, 1, 4, 5.0),      # NR = 7
    "130x7ds": (130, 7, True, 1, 4, 3.0),         # NR = 9 (more roles than 8 waves)
    "256x4ss": (256, 4, False, 1, 4, 2.0),        # 16 tiles; data half NTW = 4, model half NTW = 8
    "6x7ds_p2": (6, 7, True, 2, 4, 5.0),          # parked pooled Q, pooled slope
    "10x15ss_p4": (10, 15, False, 4, 4, 5.0),
    "5x8ds_p3": (5, 8, True, 3, 4, 5.0),
    "300x10ss": (300, 10, False, 1, 4, 4.0),      # slabs, more than one group per row
    "150x6ds_p2": (150, 6, True, 2, 4, 5.0),
    "8x100ss": (8, 100, False, 1, 4, 5.0),        # generic DNA kernel
    "A3_6x5ds": (6, 5, True, 1, 3, 3.0),          # generic statistics of other alphabets
    "A20_12x9ss": (12, 9, False, 1, 20, 4.0),
    "A5_7x6ds_p2": (7, 6, True, 2, 5, 5.0),
}
FUSED = ("10x15ss", "16x16ds", "16x32ss", "32x16ss", "8x12ds")
BOUNDARY_MODELS = ("10x15ss", "20x40ds")
ROWS_MODELS = ("10x15ss", "33x17ss")
# data shapes (n, Lh): rows shorter than a group (units span rows); three groups with a ragged tail
SHAPES = ((5, 21), (3, 70))
# exact group boundaries, on both halves: (chain length Lf, data shape)
BOUNDARIES = ((64, (3, 64)), (33, (3, 33)), (32, (4, 32)))


def round_up(x, pool):
    return -(-x // pool) * pool


def case_lengths(name, Lf=LF, shapes=SHAPES):
    """(Lf, [(n, L)]) of a model: hidden lengths rounded up to the model's pooling"""
    K, M, ds, pool, A, bshift = MODELS[name]
    out = []
    for n, Lh in shapes:
        Lh = round_up(Lh, pool)
        out.append((n, Lh + M - 1))
    return round_up(Lf, pool), out


def make_case_pair(name, Lf, batchsize=B, cd_k=CD_K):
    """(crbm_amd.CRBM, OracleCRBM) of a case, built as tests/test_gpu_parity.py make_pair builds them (the device handle
    is created on first use: on the CPU only the oracle is used)"""
    from tests.test_gpu_parity import make_pair
    K, M, ds, pool, A, bshift = MODELS[name]
    kw = {}
    if pool > 1:
        kw["pooling"] = pool
    if A != 4:
        kw["input_dims"] = A
    return make_pair(K, M, ds=ds, batchsize=batchsize, cd_k=cd_k, Lf=Lf, seed=5, wscale=1.0, bshift=bshift, rho=RHO, **kw)


def case_data(name, n, L):
    K, M, ds, pool, A, bshift = MODELS[name]
    return synthetic_onehot(n, L, seed=100 * n + L, A=A)


class Case(object):
    """one GPU case: a handle of `model` with chains of hidden length Lf, created under `env`, then one crbm_train_local per
    data shape (n, L); `fused`: what crbm_get_launch_info must report as stats_fused"""

    def __init__(self, id, model, Lf, shapes, env=None, batchsize=B, cd_k=CD_K, full_size=False):
        self.id, self.model, self.Lf, self.shapes, self.env = id, model, Lf, shapes, dict(env or {})
        self.batchsize, self.cd_k, self.full_size = batchsize, cd_k, full_size
        self.fused = int(model in FUSED and self.env.get("CRBM_STATS") != "split")


def _cases():
    out = []
    for name in MODELS:
        Lf, shapes = case_lengths(name)
        out.append(Case(name, name, Lf, shapes))
    for name in BOUNDARY_MODELS:                      # group boundaries on both halves
        for Lf, shape in BOUNDARIES:
            out.append(Case("%s-Lf%d-%dx%d" % ((name, Lf) + shape), name, *case_lengths(name, Lf, (shape,))))
    for name in FUSED:                                # launch structures of the fused models (default: one launch)
        for structure in ("two", "split"):
            out.append(Case("%s-%s" % (name, structure), name, *case_lengths(name), env={"CRBM_STATS": structure}))
    for name in ROWS_MODELS:                          # one block does everything / blocks with an uneven share of units
        for rows in (1, 3):
            out.append(Case("%s-rows%d" % (name, rows), name, *case_lengths(name), env={"CRBM_STATS_ROWS": str(rows)}))
    # config #2's model at the plan of the benchmark: grid-level errors (a block's partial row lost, a tile of chains twice)
    out.append(Case("10x15ss-full-size", "10x15ss", 186, [(1024, 200)], batchsize=8192, cd_k=1, full_size=True))
    return out


CASES = _cases()
KNOBS = ("CRBM_STATS", "CRBM_STATS_ROWS")


def report(got, ref, ds):
    """one line per compared block: its size and the largest error in units of its tolerance (assert_sums)"""
    lines = []
    for key in compared_keys(ds):
        want = np.ravel(ref[key]).astype(np.float64)
        err = np.abs(np.asarray(got[key], dtype=np.float64) - want)
        if key.startswith(("v_", "n_")):
            lines.append("  %-6s max|ref| %-12.6g max err %g (exact)" % (key, np.abs(want).max(), err.max()))
            continue
        atol = 1e-5 + (1.6e-6 * float(np.abs(want).max()) if key.startswith(("vh", "sw")) else 0.0)
        lines.append("  %-6s max|ref| %-12.6g max err %.3g = %.3f of the tolerance" % (
            key, np.abs(want).max(), err.max(), float((err / (atol + RTOL * np.abs(want))).max())))
    return "\n".join(lines)
