"""The yardstick of tests/test_gpu_statistics.py (tests/statistics_reference.py) on the CPU, before any kernel is held to it:
the model half rebuilt from the visible sample alone is the oracle's; the unpacking of the packed buffer is
crbm_layout.h's sums_layout() for every alphabet; and every GPU case meets, on the oracle alone, the conditions that keep
its tolerances from hiding an error (the GPU test asserts them again on the sample the handle drew)."""
import os
import subprocess

import numpy as np
import pytest

from oracle.crbm_oracle import OracleCRBM, synthetic_onehot
from tests import statistics_reference as S

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize("K,M,ds,pool,A", [(6, 9, True, 1, 4), (5, 7, False, 3, 4), (4, 5, True, 2, 5)])
def test_model_half_from_the_visible_sample_alone(K, M, ds, pool, A):
    B, Lf, k = 8, 12 * pool, 2
    rng = np.random.default_rng(K + M)
    o = OracleCRBM(K, M, doublestranded=ds, batchsize=B, cd_k=k, pooling=pool, input_dims=A, fantasy_hidden_len=Lf, seed=3,
                   rho=0.03, W=rng.standard_normal((K, 1, A, M)).astype(np.float32))
    o.b = o.b + 4.0
    D = synthetic_onehot(5, 10 * pool + M - 1, seed=2, A=A)
    P_m, P_mp, v_m = o.gibbs_steps(k)
    want = o.local_sums(D, P_m, P_mp, v_m)
    assert P_m.sum() > 1.0 and set(want) == set(S.compared_keys(ds))
    for chunk in (512, 3):                         # all chains at once / 3 + 3 + 2
        got = dict(S.reference_sums(o, D, o.last_v_model))
        got.update(S.model_half(o, o.last_v_model, chunk=chunk))
        assert set(got) == set(want)
        for key in want:
            np.testing.assert_allclose(got[key], want[key], rtol=1e-12, atol=0, err_msg=key)


TRIPLES = [(10, 15, 4), (1, 1, 4), (6, 5, 3), (12, 9, 20), (7, 6, 5), (3, 4, 1), (5, 8, 64)]


def test_unpacking_is_the_layout_of_the_library(tmp_path):
    exe = str(tmp_path / "sums_layout")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g1", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                           "-I", os.path.join(ROOT, "crbm_amd", "csrc"), os.path.join(ROOT, "tests", "emu", "sums_layout_main.cpp"),
                           "-o", exe])
    out = subprocess.run([exe] + [str(x) for t in TRIPLES for x in t], capture_output=True, text=True, timeout=60)
    assert out.returncode == 0, out.stderr
    rows = [[int(x) for x in line.split()] for line in out.stdout.splitlines()]
    assert len(rows) == len(TRIPLES)
    for (K, M, A), (data_off, n_d, model_off, n_m, count, skip_begin, skip_len) in zip(TRIPLES, rows):
        buf = np.arange(count, dtype=np.float32)          # every element is its own offset (exact in float32: count < 2^24)
        d = S.unpack_sums(buf, K, M, A)
        KAM = K * A * M
        assert (d["vh_d"][0], d["n_d"][0], d["vh_m"][0], d["n_m"][0]) == (data_off, n_d, model_off, n_m)
        assert d["sw"][0] == data_off + skip_begin and d["sw"].size + d["sb"].size == skip_len
        assert d["v_d"][-1] + 1 == n_d and d["v_m"][-1] + 1 == n_m
        sizes = {k: x.size for k, x in d.items()}
        assert sizes == {"vh_d": KAM, "vh_dp": KAM, "h_d": K, "h_dp": K, "sw": KAM, "sb": K, "v_d": A, "n_d": 1,
                         "vh_m": KAM, "vh_mp": KAM, "h_m": K, "h_mp": K, "v_m": A, "n_m": 1}
        np.testing.assert_array_equal(S.pack_sums(d, K, M, A), buf)      # every element once, in order
        if A == 4:                                                       # the DNA helper of the older tests
            from tests.test_gpu_parity import _unpack_sums
            old = _unpack_sums(buf, K, M)
            for key in old:
                np.testing.assert_array_equal(np.ravel(old[key]), np.ravel(d[key]), err_msg=key)


def _distinct(cases):
    seen, out = set(), []
    for c in cases:
        key = (c.model, c.Lf, tuple(c.shapes), c.batchsize, c.cd_k)
        if key not in seen:
            seen.add(key)
            out.append(c)
    return out


@pytest.mark.parametrize("case", _distinct(S.CASES), ids=[c.id for c in _distinct(S.CASES)])
def test_conditions_of_the_gpu_cases_hold_on_the_oracle(case):
    """activity window, block sizes and sum lengths of every case, with the oracle's own chain in place of the handle's"""
    K, M, ds, pool, A, bshift = S.MODELS[case.model]
    _, o = S.make_case_pair(case.model, case.Lf, case.batchsize, case.cd_k)
    o.gibbs_steps(case.cd_k)
    assert case.Lf % pool == 0 and (case.full_size or case.batchsize == S.B)
    for n, L in case.shapes:
        Lh = L - M + 1
        assert Lh % pool == 0 and (case.full_size or Lh % 32 != 0 or (case.Lf, (n, Lh)) in S.BOUNDARIES)
        D = S.case_data(case.model, n, L)
        ref = S.reference_sums(o, D, o.last_v_model)
        S.check_conditions(o, D, ref, case.Lf, case.full_size)


def test_the_case_list_covers_what_it_is_for():
    ids = [c.id for c in S.CASES]
    assert len(set(ids)) == len(ids)
    by = {c.id: c for c in S.CASES}
    for name in S.FUSED:
        K, M, ds, pool, A, _ = S.MODELS[name]
        assert 4 * -(-M // 16) * (1 + ds) * -(-K // 16) <= 8 and pool == 1 and A == 4          # Cfg::FUSE_STATS
        assert [by[i].fused for i in (name, name + "-two", name + "-split")] == [1, 1, 0]
    for name in set(S.MODELS) - set(S.FUSED):
        K, M, ds, pool, A, _ = S.MODELS[name]
        assert not (4 * -(-M // 16) * (1 + ds) * -(-K // 16) <= 8 and pool == 1 and A == 4 and K <= 256 and M <= 64)
        assert by[name].fused == 0
    assert by["10x15ss-full-size"].batchsize == 8192 and by["10x15ss-full-size"].fused == 1
    # the build leaves the code object of every case that takes specialised kernels (DNA, motifs of up to 64 letters) in the cache
    import __graft_entry__ as entry
    built = {(c["num_motifs"], c["motif_length"], int(c.get("doublestranded", 0)), c.get("pooling", 1), c.get("batchsize", 20),
              c.get("fantasy_hidden_len", 200)) for c in entry.PRECOMPILE + entry.STATISTICS_SHAPES}
    for c in S.CASES:
        K, M, ds, pool, A, _ = S.MODELS[c.model]
        assert A != 4 or M > 64 or (K, M, int(ds), pool, c.batchsize, c.Lf) in built, c.id
