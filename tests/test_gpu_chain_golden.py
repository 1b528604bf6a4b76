"""The chains of the chain kernels against tests/golden/chain_parent.npz, recorded on the GPU by
tools/record_chain_golden.py on the commit BEFORE the kernels' instruction diet (letters from the signs of t - threshold,
the mask window packed in 32-bit halves, one load round trip in the prologue): from the same parameters, state and seeds,
launches of 1, 1 and 3 Gibbs steps must leave EXACTLY the recorded hidden state of both strands and the recorded letters
after every launch, with the launch geometry compiled in (CRBM_GEOM=2) and in the run-time form (CRBM_GEOM=0).

The shapes (tools/record_chain_golden.py, SHAPES) are the six of tests/test_gpu_geometry.py -- Lv % 4 of 0 and 3, both
state-load paths, both strands, two mask words, a ragged last tile -- and three mask widths that decide how the window
word is packed: K = 7 (a mask across bit 32 at bits 28..35), K = 16 (no straddle, exactly 64 bits), K = 21 (three masks
per word)."""
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
    with np.load(os.path.join(ROOT, "tests", "golden", "chain_parent.npz")) as f:
        return {k: f[k] for k in f.files}


@pytest.mark.parametrize("geom", [2, 0])
@pytest.mark.parametrize("name,K,M,ds,Lf,B,S", recorder.SHAPES, ids=[s[0] for s in recorder.SHAPES])
def test_chain_is_the_recorded_one(golden, name, K, M, ds, Lf, B, S, geom):
    got = recorder.run_chain(K, M, ds, Lf, B, S, geom)
    want = {k.split("/", 1)[1]: a for k, a in golden.items() if k.startswith(name + "/")}
    assert sorted(got) == sorted(want) and len(want) == (3 if ds else 2) * len(recorder.LAUNCHES)
    for k in sorted(want):
        np.testing.assert_array_equal(got[k], want[k], err_msg="%s, CRBM_GEOM=%d: %s differs from the recorded chain" % (name, geom, k))
