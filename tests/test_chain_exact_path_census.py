"""Host side of tests/test_gpu_chain_exact_path.py: the run recorded in tests/golden/chain_exact_path.npz reaches every
field slot of the hidden sampler's exact path.  The float64 oracle replays the chains of EXACT_PATH_SHAPES with its own
sampler (same parameters, start state, seed and steps) and counts the units whose coarse 12-bit field equals
floor(4096 P), the ones the coarse tests leave undecided: at least two in each of the ten slots, on each strand."""
import importlib.util
import os

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_spec = importlib.util.spec_from_file_location("record_chain_golden", os.path.join(ROOT, "tools", "record_chain_golden.py"))
recorder = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(recorder)


def test_the_shapes_are_the_issue_s():
    assert [s[1:7] for s in recorder.EXACT_PATH_SHAPES] == [(10, 15, False, 186, 32, 4), (21, 8, True, 64, 32, 2)]
    assert recorder.LAUNCHES == (1, 1, 3)


@pytest.mark.parametrize("name,K,M,ds,Lf,B,S,seed", recorder.EXACT_PATH_SHAPES, ids=[s[0] for s in recorder.EXACT_PATH_SHAPES])
def test_every_field_slot_holds_two_undecided_units(name, K, M, ds, Lf, B, S, seed):
    counts = recorder.exact_path_census(K, M, ds, Lf, B, seed)
    print(name, counts.tolist())
    assert counts.shape == (2 if ds else 1, 10)
    assert counts.min() >= 2, "%s: undecided units per (strand, slot) %s" % (name, counts.tolist())
