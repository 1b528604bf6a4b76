// run_slabs (crbm_amd/csrc/crbm_sweep.h) with recording callbacks, for tests/test_sweep_host.py: every call of enqueue,
// collect and drain is written to `ev` as five ints (kind, i, set, start, cnt; kind 0 enqueue, 1 collect, 2 drain), and
// the callback of kind `fail_kind` for slab `fail_slab` returns `fail_code` (fail_kind < 0: none fails).  Returns what
// run_slabs returned; *nev is the number of calls, of which the first `cap` are recorded.
#include "crbm_sweep.h"

extern "C" int sweep_trace(int n, int slab, int depth, int fail_kind, int fail_slab, int fail_code, int* ev, int cap, int* nev) {
  int count = 0;
  auto record = [&](int kind, int i, int set, int start, int cnt) -> int {
    if (count < cap) {
      const int rec[5] = {kind, i, set, start, cnt};
      for (int k = 0; k < 5; ++k) ev[count * 5 + k] = rec[k];
    }
    ++count;
    return (kind == fail_kind && i == fail_slab) ? fail_code : 0;
  };
  const int rc = crbm::run_slabs(n, slab, depth,
    [&](int i, int set, int start, int cnt) { return record(0, i, set, start, cnt); },
    [&](int i, int set, int start, int cnt) { return record(1, i, set, start, cnt); },
    [&] { record(2, -1, -1, -1, -1); });
  *nev = count;
  return rc;
}
