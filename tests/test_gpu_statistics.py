"""The packed raw sums of crbm_train_local -- both halves of the gradient statistics, straight from the matrix cores --
against the float64 oracle, block by block (vh, vh', h, h', sw, sb, letter counts, normalisers), on every branch of the
statistics kernels: fused / two launches / split, NL = 3 / 4, 64- / 128-bit letter windows, packed column tiles, role
counts of 1 to 9, parked pooled sparsity columns, slabs with several groups per row, the generic kernels (long motifs,
other alphabets), one block / an uneven share of units, group boundaries, and config #2 at the benchmark's plan.

After an UPDATE the statistics are seen through lr * (difference of normalised means) with the sparsity blocks further
scaled by lambda * g / K: errors of 1e-3 in vh and of 10 % in sw pass there.  Here every raw block is held to 1e-4.

The reference (tests/statistics_reference.py) has no tie to hide behind: the model half is rebuilt in float64 from the
visible sample the handle itself drew.  Cases, tolerances and the conditions that keep a tolerance from hiding an error
are pinned on the CPU by tests/test_statistics_reference.py."""
import ctypes

import numpy as np
import pytest

from tests import statistics_reference as S

pytestmark = pytest.mark.gpu


def train_local_sums(m, D):
    """one crbm_train_local on batch D -> the packed buffer as a dict"""
    from crbm_amd._lib import fptr
    h = m._h()
    buf = np.zeros(m._lib.crbm_sums_count(h), dtype=np.float32)
    m._call("crbm_train_local", fptr(D), D.shape[0], D.shape[3], fptr(buf))
    return S.unpack_sums(buf, m.num_motifs, m.motif_length, m.input_dims)


@pytest.mark.parametrize("case", S.CASES, ids=[c.id for c in S.CASES])
def test_raw_sums_match_the_oracle(case, monkeypatch):
    from crbm_amd._lib import CrbmLaunchInfo
    for knob in S.KNOBS:
        monkeypatch.delenv(knob, raising=False)
    for knob, value in case.env.items():          # read when the handle is created
        monkeypatch.setenv(knob, value)
    m, o = S.make_case_pair(case.model, case.Lf, case.batchsize, case.cd_k)
    info = CrbmLaunchInfo()
    handle = m._h()                               # creates the device handle (and m._lib)
    m._lib.crbm_get_launch_info(handle, ctypes.byref(info))
    assert info.stats_fused == case.fused
    for n, L in case.shapes:
        D = S.case_data(case.model, n, L)
        got = train_local_sums(m, D)
        v = m.get_fantasy_visible()               # what d_vf holds in every launch structure: the model half is a function of it
        np.testing.assert_array_equal(v.sum(axis=2), 1.0)
        ref = S.reference_sums(o, D, v)
        S.check_conditions(o, D, ref, case.Lf, case.full_size)
        what = "%s n=%d L=%d" % (case.id, n, L)
        print(what + "\n" + S.report(got, ref, o.doublestranded))
        assert got["n_m"][0] == case.batchsize and got["n_d"][0] == n
        S.assert_sums(got, ref, o.doublestranded, what)
