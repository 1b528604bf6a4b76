"""tests/variant_reference.py pinned (CPU, float64): on gap-free rows written as a stream with separators it agrees with
the oracle's own brute force, L (freeEnergy(mutant) - freeEnergy(base)) and the per-motif free energies of the two
rows, for single- and double-stranded models; on hand-made streams it follows the gap rules of include/crbm_amd.h -- a
gap at distance d < M removes exactly the M - d windows that touch it, a variant on a code 4 gives zeros, T < M gives
the bias term alone, alt == ref gives exact zeros."""
import numpy as np
import pytest

from oracle.crbm_oracle import onehot_of
from tests.emu import harness
from tests.variant_reference import variant_effects, forced_positions, variant_list, contexts


@pytest.mark.parametrize("K,M,ds", [(10, 15, True), (10, 5, False), (6, 1, True)], ids=["ds_10x15", "ss_10x5", "ds_6x1"])
def test_gap_free_rows_against_the_oracles_brute_force(K, M, ds):
    o = harness.random_model(K, M, ds, 31 + K + M, draw_c=True)
    rng = np.random.default_rng(5)
    n, L = 3, 2 * M + 9
    rows = rng.integers(0, 4, size=(n, L), dtype=np.uint8)
    stream = np.concatenate([np.concatenate([r, [4]]) for r in rows])[:-1].astype(np.uint8)
    row_of, p_of, alt = np.repeat(np.arange(n), L * 4), np.tile(np.repeat(np.arange(L), 4), n), np.tile(np.arange(4), n * L)
    got = variant_effects(o, stream, row_of * (L + 1) + p_of, alt)
    base = onehot_of(rows)
    fe0, fem0 = L * o.freeEnergy(base), o.freeEnergy(base, True)
    c = o.c.ravel()
    for i in range(0, row_of.size, 7):                      # every seventh (row, position, letter): each a row of its own
        r, p, a = row_of[i], p_of[i], alt[i]
        mutant = rows[r:r + 1].copy()
        mutant[0, p] = a
        D = onehot_of(mutant)
        np.testing.assert_allclose(got["dfe"][i], L * o.freeEnergy(D)[0] - fe0[r], rtol=1e-9, atol=1e-9)
        # the oracle's per-motif free energy carries the visible term in every column
        want_k = o.freeEnergy(D, True)[0] - fem0[r] + (c[a] - c[rows[r, p]])
        np.testing.assert_allclose(got["per_motif"][i], want_k, rtol=1e-9, atol=1e-9)
    assert np.array_equal(got["windows"], np.minimum(p_of, L - M) - np.maximum(0, p_of - M + 1) + 1)   # the row's starts that cover p
    own = alt == rows[row_of, p_of]
    assert np.all(got["dfe"][own] == 0.0) and np.all(got["per_motif"][own] == 0.0)
    assert np.abs(got["dfe"][~own]).min() > 0


def test_gap_rules_on_hand_made_streams():
    M = 5
    o = harness.random_model(10, M, False, 15, draw_c=True)
    c = o.c.ravel()
    T, p = 40, 20
    clean = np.random.default_rng(2).integers(0, 4, size=T, dtype=np.uint8)
    alt = (clean[p] + 1) % 4
    full = variant_effects(o, clean, [p], [alt])
    assert full["windows"][0] == M
    for d in range(1, M + 2):                               # a gap d letters to the right (left): the M - d windows that reach it leave
        for side in (1, -1):
            s = clean.copy()
            s[p + side * d] = 4
            got = variant_effects(o, s, [p], [alt])
            assert got["windows"][0] == M - max(0, M - d), (d, side)
            if d >= M:
                assert got["dfe"][0] == full["dfe"][0]
    both = clean.copy()
    both[p - 1] = both[p + 1] = 4                           # gaps on both sides: no window, the bias term alone
    got = variant_effects(o, both, [p], [alt])
    assert got["windows"][0] == 0 and np.all(got["per_motif"] == 0) and got["dfe"][0] == -(c[alt] - c[clean[p]])
    on_n = clean.copy()
    on_n[p] = 4                                             # the variant sits on a code 4
    got = variant_effects(o, on_n, [p], [alt])
    assert got["windows"][0] == 0 and got["dfe"][0] == 0 and np.all(got["per_motif"] == 0)
    short = clean[:M - 1]                                   # T < M
    got = variant_effects(o, short, [0, M - 2], [(short[0] + 1) % 4, (short[M - 2] + 2) % 4])
    assert np.all(got["windows"] == 0) and np.all(got["per_motif"] == 0)
    assert got["dfe"][0] == -(c[(short[0] + 1) % 4] - c[short[0]])
    ends = variant_effects(o, clean, [0, 1, T - 2, T - 1], [3 - clean[0], 3 - clean[1], 3 - clean[T - 2], 3 - clean[T - 1]])
    assert ends["windows"].tolist() == [1, 2, 2, 1]


def test_contexts_and_the_forced_positions():
    s = np.array([0, 1, 4, 4, 2, 3, 0, 1, 2, 3], np.uint8)
    assert contexts(s, [0, 9], 3).tolist() == [[4, 4, 0, 1, 4], [1, 2, 3, 4, 4]]
    f = forced_positions(s, 3).tolist()
    assert f == [0, 1, 2, 3, 4, 7, 8, 9]                    # 0, 1, M-2, M-1, T-M, T-2, T-1; 1|2 and 3|4 straddle the gap's edges; 3 is inside
    pos, alt = variant_list(s, 3, 20, 1)
    assert pos.size == 20 + len(f) + 2 and pos[-1] == pos[-2] and alt[-1] == s[pos[-1]] and s[pos[-1]] < 4
    assert (pos[:-2] == pos[-1]).any()
