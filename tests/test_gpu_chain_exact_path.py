"""The exact path of the hidden sampler against tests/golden/chain_exact_path.npz, recorded on the GPU by
`tools/record_chain_golden.py --exact-path` on the commit BEFORE the second instruction diet of the chain kernel (the
exact path reads the coarse fields the main path kept; coarse fields converted where they sit in their word; the
wave-uniform words of Philox rounds 1-2 joined on the scalar unit).

A unit reaches the exact path when its coarse 12-bit field cannot decide it, 2^-12 of all units: the shapes of
tests/test_gpu_chain_golden.py hold too few of them to pass through every one of the ten field slots of a Philox call.
The two shapes here (tools/record_chain_golden.py, EXACT_PATH_SHAPES) run 32 chains each:
  K = 10, M = 15, one strand, Lf = 186, 4 chains per tile  -- every wave resolves its own undecided units (sample_hidden);
  K = 21, M = 8, two strands, Lf = 64, 2 chains per tile   -- the block queues them and resolves them after the pass.
The queue of the second shape resolves its units with code of its own, not with sample_hidden's exact path, so that shape
runs a second time with every wave resolving its own units (CRBM_JIT_DEFINES=-DCRBM_INLINE_EXACT_PATH, the kernel's A/B
knob: the same bits, on the commit that recorded the fixture as well): sample_hidden's exact path on both strands and in
all three groups.
tests/test_chain_exact_path_census.py shows on the CPU that the recorded run holds at least two undecided units in every
slot on every strand.  From the same parameters, state and seeds, launches of 1, 1 and 3 Gibbs steps must leave EXACTLY
the recorded hidden state and letters after every launch, with the launch geometry compiled in (CRBM_GEOM=2) and in the
run-time form (CRBM_GEOM=0)."""
import importlib.util
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_spec = importlib.util.spec_from_file_location("record_chain_golden", os.path.join(ROOT, "tools", "record_chain_golden.py"))
recorder = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(recorder)


@pytest.fixture(scope="module")
def golden():
    with np.load(os.path.join(ROOT, "tests", "golden", "chain_exact_path.npz")) as f:
        return {k: f[k] for k in f.files}


@pytest.mark.parametrize("geom", [2, 0])
@pytest.mark.parametrize("name,K,M,ds,Lf,B,S,seed", recorder.EXACT_PATH_SHAPES, ids=[s[0] for s in recorder.EXACT_PATH_SHAPES])
def test_chain_with_undecided_units_is_the_recorded_one(golden, name, K, M, ds, Lf, B, S, seed, geom):
    got = recorder.run_chain(K, M, ds, Lf, B, S, geom, seed)
    want = {k.split("/", 1)[1]: a for k, a in golden.items() if k.startswith(name + "/")}
    assert sorted(got) == sorted(want) and len(want) == (3 if ds else 2) * len(recorder.LAUNCHES)
    for k in sorted(want):
        np.testing.assert_array_equal(got[k], want[k], err_msg="%s, CRBM_GEOM=%d: %s differs from the recorded chain" % (name, geom, k))


@pytest.mark.parametrize("geom", [2, 0])
def test_second_shape_resolved_in_the_wave_is_the_recorded_one(golden, geom, monkeypatch):
    name, K, M, ds, Lf, B, S, seed = recorder.EXACT_PATH_SHAPES[1]
    monkeypatch.setenv("CRBM_JIT_DEFINES", recorder.INLINE_EXACT_PATH_DEFINES)
    got = recorder.run_chain(K, M, ds, Lf, B, S, geom, seed)
    want = {k.split("/", 1)[1]: a for k, a in golden.items() if k.startswith(name + "/")}
    assert sorted(got) == sorted(want)
    for k in sorted(want):
        np.testing.assert_array_equal(got[k], want[k], err_msg="%s resolved in the wave, CRBM_GEOM=%d: %s differs from the recorded chain" % (name, geom, k))
