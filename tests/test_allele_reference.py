"""The float64 reference of the allele effects (tests/allele_reference.py) against what it claims to be, on the CPU: its
dfe is the brute-force F(edited stream) - F(stream) over whole streams with gaps; its (1, 1) alleles are the SNPs of
tests/variant_reference.py; a VCF anchor base in front of ref and alt changes nothing; and the lists the emulator and
GPU tests use meet full, partial and zero window counts on both haplotypes."""
import numpy as np
import pytest

from tests.emu import harness
from tests.test_emu_scan import gapped_stream as emu_stream
from tests.test_gpu_scan import gapped_stream as gpu_stream
from tests.allele_reference import allele_effects, allele_list, covers_every_count
from tests.variant_reference import variant_effects, _hidden_terms

MODELS = [(10, 15, True, 25), (10, 5, False, 15), (6, 1, True, 7)]


def free_energy(o, stream):
    """F of a stream: the valid windows' hidden terms and the letters' visible biases"""
    M = o.motif_length
    stream = np.asarray(stream, np.uint8)
    F = -np.asarray(o.c, np.float64).ravel()[stream[stream < 4]].sum()
    if stream.size >= M:
        bad = np.concatenate([[0], np.cumsum(stream > 3)])
        valid = (bad[M:] - bad[:stream.size - M + 1]) == 0
        F -= (_hidden_terms(o, stream[None, :])[0] * valid[None, :]).sum()
    return F


@pytest.mark.parametrize("K,M,ds,seed", MODELS)
def test_dfe_is_the_free_energy_change_of_the_edited_stream(K, M, ds, seed):
    o = harness.random_model(K, M, ds, seed, draw_c=True)
    stream = emu_stream(300, seed, M)
    pos, R, alts = allele_list(stream, M, 60, seed)
    want = allele_effects(o, stream, pos, R, alts)
    F0 = free_energy(o, stream)
    assert (~want["exact_zero"]).sum() > 60
    for i in np.flatnonzero(~want["exact_zero"]):
        edited = np.concatenate([stream[:pos[i]], alts[i], stream[pos[i] + R[i]:]]).astype(np.uint8)
        assert abs(want["dfe"][i] - (free_energy(o, edited) - F0)) <= 1e-9, (i, pos[i], R[i], alts[i])
    z = want["exact_zero"]
    assert z.any() and np.all(want["dfe"][z] == 0) and np.all(want["per_motif"][z] == 0) and np.all(want["windows"][z] == 0)
    assert np.allclose(want["per_motif"].sum(axis=1) - want["dfe"], [
        0.0 if z[i] else o.c.ravel()[alts[i].astype(int)].sum() - o.c.ravel()[stream[pos[i]:pos[i] + R[i]].astype(int)].sum()
        for i in range(len(pos))], atol=1e-12)


@pytest.mark.parametrize("K,M,ds,seed", MODELS)
def test_one_for_one_alleles_are_the_snps_of_the_variant_reference(K, M, ds, seed):
    o = harness.random_model(K, M, ds, seed, draw_c=True)
    stream = emu_stream(600, seed, M)
    rng = np.random.default_rng(seed)
    pos = rng.integers(0, stream.size, size=200)
    alt = rng.integers(0, 4, size=200).astype(np.uint8)
    snp = variant_effects(o, stream, pos, alt)
    got = allele_effects(o, stream, pos, np.ones(200, np.int32), [alt[i:i + 1] for i in range(200)])
    assert np.abs(got["dfe"] - snp["dfe"]).max() <= 1e-12 and np.abs(got["per_motif"] - snp["per_motif"]).max() <= 1e-12
    assert np.array_equal(got["windows"][:, 0], snp["windows"]) and np.array_equal(got["windows"][:, 1], snp["windows"])
    assert np.array_equal(got["exact_zero"], stream[pos] > 3)


def test_a_vcf_anchor_base_changes_nothing():
    o = harness.random_model(10, 15, True, 25, draw_c=True)
    stream = emu_stream(600, 3, 15)
    pos, R, alts = allele_list(stream, 15, 100, 4)
    ok = (pos >= 1) & (stream[np.maximum(pos - 1, 0)] < 4)
    pos, R, alts = pos[ok], R[ok], [a for a, k in zip(alts, ok) if k]
    plain = allele_effects(o, stream, pos, R, alts)
    anchored = allele_effects(o, stream, pos - 1, R + 1, [np.concatenate([stream[p - 1:p], a]) for p, a in zip(pos, alts)])
    live = ~plain["exact_zero"]
    assert live.sum() > 80 and not anchored["exact_zero"][live].any()
    assert np.abs(plain["dfe"][live] - anchored["dfe"][live]).max() <= 1e-9
    assert np.abs(plain["per_motif"][live] - anchored["per_motif"][live]).max() <= 1e-9


def test_every_list_of_the_emulator_tests_meets_full_partial_and_zero_window_counts():
    from tests import test_emu_alleles as emu
    for name in emu.LISTS:
        cid, o, stream, pos, R, alts = emu.case(name)
        covers_every_count(allele_effects(o, stream, pos, R, alts), R, alts, o.motif_length)


@pytest.mark.parametrize("M", [15, 10, 1])
def test_the_list_of_the_gpu_tests_meets_full_partial_and_zero_window_counts(M):
    """tests/test_gpu_alleles.py: gapped_stream(5003, 2031), 1500 random alleles, seed 77, the motif lengths of its model
    classes (the counts depend on the stream and the list alone: any model of that motif length serves)"""
    stream = gpu_stream(5003, 2031)
    pos, R, alts = allele_list(stream, M, 1500, 77)
    covers_every_count(allele_effects(harness.random_model(2, M, False, 1), stream, pos, R, alts), R, alts, M)
