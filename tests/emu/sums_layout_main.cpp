// Prints sums_layout() (crbm_layout.h: the packed raw-sum buffer) for the (K, M, A) triples of its command line, one line of
// seven ints each: data_off n_d model_off n_m count model_skip_begin model_skip_len.  A stand-alone program of host code
// alone, built with ASan + UBSan by tests/test_statistics_reference.py.
#include "crbm_layout.h"

#include <cstdio>
#include <cstdlib>

int main(int argc, char** argv) {
  if (argc < 4 || (argc - 1) % 3 != 0) {
    fprintf(stderr, "usage: %s K M A [K M A ...]\n", argv[0]);
    return 2;
  }
  for (int i = 1; i + 2 < argc; i += 3) {
    const crbm::SumsLayout s = crbm::sums_layout(atoi(argv[i]), atoi(argv[i + 1]), atoi(argv[i + 2]));
    printf("%d %d %d %d %d %d %d\n", s.data_off, s.n_d, s.model_off, s.n_m, s.count, s.model_skip_begin, s.model_skip_len);
  }
  return 0;
}
