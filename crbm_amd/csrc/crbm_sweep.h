// The slab pipeline of the evaluation sweeps (crbm_api.hip), host only: slabs, buffer sets and the order of calls, and
// nothing of what a slab computes.  Rows [0, n) go out in slabs of `slab` rows (the last one may be shorter):
//   enqueue(i, set, start, cnt)  stages, encodes and launches slab i = rows [start, start + cnt) on buffer set `set`;
//   collect(i, set, start, cnt)  copies that slab's outputs out and waits for them;
// both return 0 or an error code.  The order is what makes two sets enough:
//   depth 2: slab i runs on set i & 1 and is collected after slab i+1 has been enqueued (the copies of one slab overlap the
//            kernels of the other) and before slab i+2 is (which reuses its set);
//   depth 1: set 0 only, every slab collected right after it has been enqueued.
// A sweep of one slab uses set 0 only at either depth.  On the first error nothing more is enqueued or collected, drain()
// is called once (the caller lets everything already enqueued run out there) and the error is returned; a sweep that
// succeeds never calls drain().
#pragma once

#include <algorithm>

namespace crbm {

template <class Enqueue, class Collect, class Drain>
int run_slabs(int n, int slab, int depth, Enqueue enqueue, Collect collect, Drain drain) {
  slab = std::max(slab, 1);
  int rc = 0;
  int pi = -1, pset = 0, pstart = 0, pcnt = 0;     // the slab enqueued and not yet collected (depth 2)
  for (int start = 0, i = 0; start < n && !rc; ++i) {
    const int cnt = std::min(slab, n - start), set = depth == 2 ? (i & 1) : 0;
    rc = enqueue(i, set, start, cnt);
    if (!rc && pi >= 0) rc = collect(pi, pset, pstart, pcnt);
    if (depth == 2) { pi = i; pset = set; pstart = start; pcnt = cnt; }
    else if (!rc) rc = collect(i, set, start, cnt);
    start += cnt;
  }
  if (!rc && pi >= 0) rc = collect(pi, pset, pstart, pcnt);
  if (rc) drain();
  return rc;
}

}  // namespace crbm
