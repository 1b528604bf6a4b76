"""The chain kernels with the launch geometry compiled in (crbm_kernels.h: GeomCT; CRBM_GEOM=2: every handle) against the
same kernels reading the geometry from their arguments (CRBM_GEOM=0), on the GPU through crbm_create / crbm_gibbs_steps:
three one-step launches and one three-step launch from the same state and seeds must leave EXACTLY the same chain state
and visible sample in both forms, and the chain must be the float64 oracle's (sample for sample, p == u ties only).
crbm_geometry_launches tells which form the launches took: a shape with a ragged last tile stays in the run-time form.
One PCD-2 update of a double-stranded model on a resident data set (the fused training launch) must leave identical
parameters, velocities, chains and raw sums in both forms."""
import ctypes

import numpy as np
import pytest

from oracle.crbm_oracle import synthetic_onehot
from tests.test_gpu_parity import make_pair, assert_chain_equal_or_tied

pytestmark = pytest.mark.gpu

# (K, M, ds, Lf, chains, chains per tile, form the launches must take under CRBM_GEOM=2); __graft_entry__.GEOMETRY_SHAPES
SHAPES = [(10, 15, False, 186, 8, 4, "compiled"),      # 16-byte state loads, full tiles
          (10, 15, False, 185, 8, 4, "compiled"),      # 185 words per chain (a tile of four: 740 words, still 16-byte loads)
          (10, 15, False, 185, 6, 2, "compiled"),      # 370 words per tile: the 4-byte load path compiled in
          (10, 15, True, 50, 6, 2, "compiled"),
          (40, 6, False, 30, 4, 4, "compiled"),        # two mask words
          (10, 15, False, 186, 9, 4, "run-time")]      # ragged last tile


def _launch_counts(model):
    ct, rt = ctypes.c_int64(-1), ctypes.c_int64(-1)
    model._call("crbm_geometry_launches", ctypes.byref(ct), ctypes.byref(rt))
    return ct.value, rt.value


def _state(model):
    h, hp = model.get_fantasy()
    return h.copy(), (None if hp is None else hp.copy()), model.get_fantasy_visible().copy()


def _same(a, b):
    for x, y in zip(a, b):
        assert (x is None) == (y is None)
        if x is not None:
            np.testing.assert_array_equal(x, y)


@pytest.mark.parametrize("K,M,ds,Lf,B,S,form", SHAPES)
def test_chain_launches_are_the_same_in_both_geometry_forms(K, M, ds, Lf, B, S, form, monkeypatch):
    monkeypatch.setenv("CRBM_GIBBS_S", str(S))
    rng = np.random.default_rng(40 + Lf + B)
    h0 = rng.binomial(1, 0.05, size=(B, K, 1, Lf)).astype(np.float32)
    hp0 = rng.binomial(1, 0.05, size=(B, K, 1, Lf)).astype(np.float32) if ds else None

    def run(mode):
        monkeypatch.setenv("CRBM_GEOM", mode)
        model, o = make_pair(K, M, ds=ds, batchsize=B, Lf=Lf, wscale=1.5, bshift=5.0)
        model.set_fantasy(h0, hp0)
        model.set_rng(gibbs_step=0)
        before = _launch_counts(model)[0]
        states = []
        for k in (1, 1, 1, 3):
            model.gibbsSteps(k)
            states.append(_state(model))
        return model, o, states, _launch_counts(model)[0] - before

    model, o, compiled, n_compiled = run("2")
    _, _, runtime, n_runtime = run("0")
    assert n_runtime == 0
    assert n_compiled == (4 if form == "compiled" else 0)
    for a, b in zip(compiled, runtime):
        _same(a, b)
    # ... and that chain is the oracle's: six steps from h0
    o.fantasy_h, o.fantasy_h_prime = h0.astype(np.float64), (hp0.astype(np.float64) if ds else None)
    o.gibbs_step = 0
    o.gibbs_steps(6)
    assert_chain_equal_or_tied(model, o, (h0, hp0, 0), 6)
    assert o.fantasy_h.sum() > 0


def test_training_step_is_the_same_in_both_geometry_forms(monkeypatch):
    from crbm_amd._lib import fptr
    K, M, B, L, n = 10, 15, 8, 64, 13
    monkeypatch.setenv("CRBM_GIBBS_S", "2")
    D = synthetic_onehot(n, L, seed=77)

    def run(mode):
        monkeypatch.setenv("CRBM_GEOM", mode)
        model, _ = make_pair(K, M, ds=True, batchsize=B, Lf=L - M + 1, cd_k=2, bshift=4.0, rho=0.02)
        model._upload(D, 0)
        before = _launch_counts(model)[0]
        model._call("crbm_train_step_resident", 0, n)
        out = [model.motifs.get_value(), model.bias.get_value(), model.c.get_value(), *model.get_velocities(), *_state(model)]
        sums = np.zeros(model._lib.crbm_sums_count(model._h()), dtype=np.float32)
        model._call("crbm_train_local", fptr(D), n, L, fptr(sums))
        return out + [sums, *_state(model)], _launch_counts(model)[0] - before

    compiled, n_compiled = run("2")
    runtime, n_runtime = run("0")
    assert n_runtime == 0 and n_compiled == 2          # the update's chain launch and crbm_train_local's
    _same(compiled, runtime)
    assert np.abs(compiled[-4]).sum() > 0
