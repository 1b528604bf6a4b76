"""The pin of tests/rng_counter_cases.py: along the float64 oracle's OWN trajectory of every case of
tests/test_gpu_rng_counters.py, the draws with |p - u| < 1e-6 -- the only draws at which the GPU comparison accepts a
difference -- number no more than the helpers' caps on ties (1e-4 of the draws + 2 for chains and evaluation samples,
4 tied runs in AIS, the caps of assert_samples and test_topdown for the stand-alone samplers, none at all where the GPU
test asks for the oracle's very chain).  The GPU cases can then not pass by excusing differences as ties."""
import pytest

from tests import rng_counter_cases as cases

CASES = cases.all_cases()


def test_the_settings_are_the_stated_ones():
    assert cases.SEED_HI == 0x9E3779B900000005 and cases.SEED_HI & 0xFFFFFFFF == 5 and cases.SEED_HI >> 63 == 1
    assert cases.STEPS == (65534, 2147483646, 4294967294) and cases.OFFSETS == (65533, 2147483645, 4294967293)
    assert cases.SETTINGS["ALL"] == (cases.SEED_HI, 2**32 - 2, 2**16 - 3)
    assert cases.SETTINGS["ALL31"] == (cases.SEED_HI, 2**31 - 2, 2**31 - 3)
    assert len({c[0] for c in CASES}) == len(CASES)


@pytest.mark.parametrize("name,run", CASES, ids=[c[0] for c in CASES])
def test_oracle_trajectory_stays_inside_the_tie_cap(name, run):
    near, cap = run()
    print("%s: %d draws within 1e-6 of their threshold, cap %g" % (name, near, cap))
    assert near <= cap
