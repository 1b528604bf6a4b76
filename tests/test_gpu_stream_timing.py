"""The timing switches of the five stream entry points (crbm_api.hip, StreamSweep::run_chunks): with CRBM_*_TIMING=1 a
call writes one line "<entry point>: kernels <ms> ms over <count> <segments|chunks>" to stderr, the count being the
segments or chunks its CRBM_SLAB_BYTES gives, and returns the same bits as without the switch; without the switch it
writes nothing; a call that launches nothing (a stream shorter than a motif, an empty variant list) writes nothing
under the switch either.  Models: the 10 x 15 double-stranded and the 300 x 10 slabbed class of test_gpu_sweeps;
stream: gapped_stream(5003, 2031)."""
import re

import numpy as np
import pytest

from tests.test_gpu_sweeps import CLASSES, ids, _model
from tests.test_gpu_scan import gapped_stream, per_start, _c_scan
from tests.test_gpu_variants import per_variant, _c_call
from tests.test_gpu_alleles import costs
from tests.variant_reference import variant_list
from tests.allele_reference import allele_list, strings

pytestmark = pytest.mark.gpu

SERVED = [CLASSES[0], CLASSES[2]]
T_A, SEED = 5003, 2031


def _bits(x):
    """what a call returned, a dict or a tuple of arrays and numbers: (dtype, shape, bytes) of every field"""
    fields = [x[k] for k in sorted(x)] if isinstance(x, dict) else list(x)
    return [(np.asarray(v).dtype.str, np.shape(v), np.ascontiguousarray(v).tobytes()) for v in fields]


@pytest.mark.parametrize("cls", SERVED, ids=ids(SERVED))
def test_one_timing_line_per_call_with_the_count_of_its_segments_or_chunks(cls, monkeypatch, capfd):
    name, K, M, ds, A, pool, Lf, L, env, spec = cls
    m, o = _model(cls, monkeypatch)
    stream = gapped_stream(T_A, SEED)
    starts = T_A - M + 1
    seven = per_start(cls) * (starts // 7 + 1)                       # the budget of the sweeps' tests for 7 segments
    vpos, valt = variant_list(stream, M, 300, 77)
    chunk = vpos.size // 7 + 1
    apos, aR, aalts = allele_list(stream, M, 300, 77)
    aref, aalt = strings(stream, apos, aR, aalts)
    one_record = np.array([0, T_A + 1], np.int64)

    def hist():
        h = m.scoreHistogram(stream, bins=64, lo=-8.0, hi=8.0)
        return h.counts, h.windows

    # (entry point, switch, budget, unit, what the count must be, the call: one call of the entry point each)
    calls = [
        ("crbm_scan_sites_codes", "CRBM_SCAN_TIMING", seven, "segments", lambda n: n == 7,
         lambda: _c_scan(m, stream, 0.5, 1 << 16)),
        ("crbm_scan_histogram_codes", "CRBM_HIST_TIMING", seven, "segments", lambda n: n == 7, hist),
        ("crbm_scan_records_codes", "CRBM_RECORDS_TIMING", seven, "segments", lambda n: n == 7,
         lambda: m._records_call(stream, one_record)),
        ("crbm_variant_effects_codes", "CRBM_VARIANT_TIMING", per_variant(cls) * chunk, "chunks",
         lambda n: n == -(-vpos.size // chunk), lambda: m.variantEffects(stream, vpos, valt)),
        ("crbm_allele_effects_codes", "CRBM_ALLELE_TIMING", int(costs(cls, aR, aalts).sum()) // 7, "chunks",
         lambda n: n >= 2, lambda: m.alleleEffects(stream, apos, aref, aalt, trim=False)),
    ]
    for api, switch, budget, unit, count_ok, call in calls:
        monkeypatch.setenv("CRBM_SLAB_BYTES", str(budget))
        monkeypatch.delenv(switch, raising=False)
        capfd.readouterr()
        plain = _bits(call())
        assert capfd.readouterr().err == "", api                     # the switch unset: nothing
        monkeypatch.setenv(switch, "1")
        timed = _bits(call())
        err = capfd.readouterr().err
        monkeypatch.delenv(switch)
        print("%s %s: %r" % (name, api, err))
        lines = err.splitlines()
        assert len(lines) == 1, (api, err)
        hit = re.match(r"^%s: kernels [0-9.]+ ms over (\d+) (segments|chunks)$" % api, lines[0])
        assert hit and hit.group(2) == unit, (api, err)
        assert count_ok(int(hit.group(1))), (api, err)
        assert timed == plain, api                                   # the same bits with the switch


def test_a_call_that_launches_nothing_prints_nothing_under_its_switch(monkeypatch, capfd):
    cls = CLASSES[0]
    name, K, M, ds, A, pool, Lf, L, env, spec = cls
    m, o = _model(cls, monkeypatch)
    stream = gapped_stream(T_A, SEED)
    vpos, valt = variant_list(stream, M, 50, 4)
    monkeypatch.setenv("CRBM_SLAB_BYTES", "1")
    monkeypatch.setenv("CRBM_HIST_TIMING", "1")
    monkeypatch.setenv("CRBM_VARIANT_TIMING", "1")
    capfd.readouterr()
    h = m.scoreHistogram(stream[1:M], bins=64, lo=-8.0, hi=8.0)      # T = M - 1: no window
    assert h.windows == 0 and not h.counts.any()
    rc, out = _c_call(m, stream, vpos, valt, K, nvar=0)              # nvar == 0 succeeds and writes nothing
    assert rc == 0 and all(np.all(v == 77) for v in out.values())
    assert capfd.readouterr().err == ""
