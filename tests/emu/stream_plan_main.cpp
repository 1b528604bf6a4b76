// TEST INFRASTRUCTURE: a stand-alone program around stream_plan and run_slabs (crbm_amd/csrc/crbm_sweep.h), the segment
// plan of the stream sweeps; tests/test_stream_plan_host.py builds it with ASan + UBSan and runs it directly.
// usage: stream_plan_main <T> <M> <nslab> <budget> <budget_was_set>
// prints "starts_all seg nsets valid_words letter_words tiles" (the plan, with the layout of a full segment), then one
// line "set start cnt valid_words letter_words tiles" per segment as run_slabs hands it out, with the segment's own layout.
#include "crbm_sweep.h"

#include <cstdio>
#include <cstdlib>

using namespace crbm;

int main(int argc, char** argv) {
  if (argc != 6) { fprintf(stderr, "usage: %s <T> <M> <nslab> <budget> <budget_was_set>\n", argv[0]); return 2; }
  const long T = atol(argv[1]);
  const int M = atoi(argv[2]), nslab = atoi(argv[3]);
  const size_t budget = (size_t)strtoull(argv[4], nullptr, 10);
  if (M < 1 || T < M || nslab < 1) { fprintf(stderr, "bad arguments\n"); return 2; }
  const StreamPlan p = stream_plan(T, M, nslab, budget, atoi(argv[5]) != 0);
  printf("%d %d %d %ld %ld %d\n", p.starts_all, p.seg, p.nsets, p.full.valid_words, p.full.letter_words, p.full.tiles);
  return run_slabs(p.starts_all, p.seg, 2,
    [&](int, int set, int start, int cnt) {
      const ScanLayout l = scan_layout((long)cnt + M - 1, cnt);
      printf("%d %d %d %ld %ld %d\n", set, start, cnt, l.valid_words, l.letter_words, l.tiles);
      return 0;
    },
    [](int, int, int, int) { return 0; }, [] {});
}
