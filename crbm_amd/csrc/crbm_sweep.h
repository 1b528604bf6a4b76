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
// succeeds never calls drain().  Below it: stream_plan, the segments a stream sweep hands to run_slabs.
#pragma once

#include <math.h>
#include <stddef.h>
#include <stdint.h>
#include <string.h>

#include <algorithm>
#include <vector>

#include "crbm_layout.h"

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

// The segments of a stream sweep (crbm_api.hip, StreamSweep): the T - M + 1 window starts of a stream of T >= M letters
// go out `seg` at a time; segment [start, start + cnt) reads letters [start, start + cnt + M - 1), a halo of M - 1
// behind its own.  A window start costs its staged byte, its letter and validity bits, per slab of the model its counts
// and offsets, and a share of records: 4 + 4 nslab bytes of `budget` (CRBM_SLAB_BYTES, or 256 MB).  Unless the budget
// was set by hand, a segment stays within 32 MB, so that a long stream has something to overlap.  Two buffer sets
// exactly when there is more than one segment; `full` is the layout of a whole segment, what every set is sized for.
struct StreamPlan {
  int starts_all, seg, nsets;
  ScanLayout full;
};
inline StreamPlan stream_plan(long T, int M, int nslab, size_t budget, bool budget_was_set) {
  StreamPlan p;
  p.starts_all = (int)(T - M + 1);
  const size_t per_start = 4 + (size_t)4 * nslab;
  size_t seg = std::max<size_t>(budget / per_start, 1);
  if (!budget_was_set) seg = std::min(seg, std::max<size_t>(1, (32u << 20) / per_start));
  p.seg = (int)std::min(seg, (size_t)p.starts_all);
  p.nsets = p.seg < p.starts_all ? 2 : 1;
  p.full = scan_layout((long)p.seg + M - 1, p.seg);
  return p;
}

// The chunks of a variant sweep (crbm_api.hip, variant_effects_any): nvar >= 1 variants go out `chunk` at a time.  A
// variant costs its staged context of CW = 2M - 1 bytes, their letter and validity bits (3 bits each), the outputs
// 4 (K + 2) and its alt byte out of `budget` (CRBM_SLAB_BYTES, or 256 MB); unless the budget was set by hand a chunk
// stays within 32 MB, so that a long list has something to overlap.  A chunk's contexts are one stream for the kernels,
// whose window starts are 32 bits wide: chunk * CW stays within 2^30.  Two buffer sets exactly when there is more than
// one chunk; `full` is the layout of a whole chunk, what every set is sized for.
struct VariantPlan {
  int chunk, nsets, CW;
  size_t per_variant;
  ScanLayout full;
};
inline VariantPlan variant_plan(long nvar, int M, int K, size_t budget, bool budget_was_set) {
  VariantPlan p;
  p.CW = 2 * M - 1;
  p.per_variant = (size_t)p.CW + ((size_t)3 * p.CW + 7) / 8 + (size_t)4 * (K + 2) + 1;
  size_t chunk = std::max<size_t>(budget / p.per_variant, 1);
  if (!budget_was_set) chunk = std::min(chunk, std::max<size_t>(1, (32u << 20) / p.per_variant));
  chunk = std::min(chunk, ((size_t)1 << 30) / (size_t)p.CW);
  p.chunk = (int)std::min(chunk, (size_t)nvar);
  p.nsets = p.chunk < nvar ? 2 : 1;
  p.full = scan_layout((long)p.chunk * p.CW, p.chunk);      // (tiles: of 64 variants)
  return p;
}
// the contexts of variants pos[0 .. cnt) of a stream of T codes, CW = 2M - 1 bytes each at dst: codes
// [pos - M + 1, pos + M - 1], code 4 (no letter) for what lies outside the stream; every pos inside [0, T)
inline void gather_contexts(const uint8_t* codes, int64_t T, const int64_t* pos, int cnt, int M, uint8_t* dst) {
  const int CW = 2 * M - 1;
  for (int i = 0; i < cnt; ++i, dst += CW) {
    const int64_t lo = pos[i] - (M - 1);
    if (lo >= 0 && lo + CW <= T) memcpy(dst, codes + lo, (size_t)CW);
    else
      for (int j = 0; j < CW; ++j) dst[j] = lo + j >= 0 && lo + j < T ? codes[lo + j] : (uint8_t)4;
  }
}

// The chunks of an allele sweep (crbm_api.hip, allele_effects_any): variant i replaces ref_len[i] codes by the
// alt_off[i + 1] - alt_off[i] letters of its alt.  It costs its staged haplotypes, n_i = R + A + 4M - 4 codes (no
// separators: the kernel bounds the window starts of a haplotype), their letter and validity bits (3 bits each, rounded
// up per variant), its table entry and the outputs 4 (K + 3) out of `budget` (CRBM_SLAB_BYTES, or 256 MB); unless the
// budget was set by hand a chunk stays within 32 MB.  Chunk j is variants [cuts[j], cuts[j + 1]): the longest prefix of
// what is left that stays within the budget and within 2^30 staged codes (the kernels' window starts are 32 bits wide),
// and at least one variant.  Two buffer sets exactly when there is more than one chunk; every set is sized for the
// longest chunk (max_cnt variants) and for the most staged codes (max_codes), `full` being the layout of the latter.
struct AllelePlan {
  std::vector<int64_t> cuts;
  int nsets, max_cnt;
  long max_codes;
  ScanLayout full;
};
inline size_t allele_cost(long R, long A, int M, int K) {
  const size_t n = (size_t)allele_codes(R, A, M);
  return n + (3 * n + 7) / 8 + sizeof(AlleleEntry) + (size_t)4 * (K + 3);
}
inline AllelePlan allele_plan(long nvar, const int32_t* ref_len, const int64_t* alt_off, int M, int K, size_t budget, bool budget_was_set) {
  AllelePlan p;
  if (!budget_was_set) budget = std::min(budget, (size_t)32 << 20);
  p.cuts.push_back(0);
  p.max_cnt = 0; p.max_codes = 0;
  size_t bytes = 0;
  long codes = 0;
  for (long i = 0; i < nvar; ++i) {
    const long R = ref_len[i], A = (long)(alt_off[i + 1] - alt_off[i]), n = allele_codes(R, A, M);
    const size_t cost = allele_cost(R, A, M, K);
    if (i > p.cuts.back() && (bytes + cost > budget || codes + n > (1L << 30))) {
      p.cuts.push_back(i);
      bytes = 0; codes = 0;
    }
    bytes += cost; codes += n;
    p.max_cnt = std::max(p.max_cnt, (int)(i + 1 - p.cuts.back()));
    p.max_codes = std::max(p.max_codes, codes);
  }
  p.cuts.push_back(nvar);
  p.nsets = p.cuts.size() > 2 ? 2 : 1;
  p.full = scan_layout(p.max_codes, p.max_codes);
  return p;
}
// the haplotypes of variants [0, cnt) of a stream of T codes, back to back at dst, and their table entries: per variant
// left = codes [pos - M + 1, pos), the R replaced codes, right = codes [pos + R, pos + R + M - 1), then left, the A alt
// letters and right again; code 4 (no letter) for what lies outside the stream.  0 <= pos, pos + R <= T.  Returns the
// number of codes written.
inline long gather_haplotypes(const uint8_t* codes, int64_t T, const int64_t* pos, const int32_t* ref_len, const int64_t* alt_off,
                              const uint8_t* alt_codes, int cnt, int M, uint8_t* dst, AlleleEntry* table) {
  auto span = [&](uint8_t* d, int64_t lo, int64_t n) {       // codes [lo, lo + n), 4 outside the stream
    if (lo >= 0 && lo + n <= T) { if (n) memcpy(d, codes + lo, (size_t)n); }
    else
      for (int64_t j = 0; j < n; ++j) d[j] = lo + j >= 0 && lo + j < T ? codes[lo + j] : (uint8_t)4;
  };
  long at = 0;
  for (int i = 0; i < cnt; ++i) {
    const int64_t p = pos[i];
    const int R = ref_len[i], A = (int)(alt_off[i + 1] - alt_off[i]);
    AlleleEntry e{(int32_t)at, R, A, R == 0 && A == 0 ? 1 : 0};
    uint8_t* d = dst + at;
    span(d, p - (M - 1), (int64_t)R + 2 * (M - 1));          // left . ref . right is one run of the stream
    for (int j = 0; j < R; ++j) e.zero |= d[M - 1 + j] > 3 ? 1 : 0;
    d += R + 2 * (M - 1);
    memcpy(d, dst + at, (size_t)(M - 1));
    if (A) memcpy(d + M - 1, alt_codes + alt_off[i], (size_t)A);
    memcpy(d + M - 1 + A, dst + at + M - 1 + R, (size_t)(M - 1));
    at += allele_codes(R, A, M);
    table[i] = e;
  }
  return at;
}

// Record summaries (crbm_api.hip, scan_records_any), the host's part.  records_check: what is wrong with the record
// starts of a stream of T codes (sequences.seqsToStream: nrec + 1 entries from 0 on, every record followed by one
// code 4, T + 1 last), or null.  nrec >= 1.
inline const char* records_check(const uint8_t* codes, int64_t T, const int64_t* rec_start, int64_t nrec) {
  if (rec_start[0] != 0) return "rec_start must start at 0";
  for (int64_t r = 0; r < nrec; ++r)
    if (rec_start[r + 1] <= rec_start[r]) return "rec_start must ascend (every record is followed by one separator)";
  if (rec_start[nrec] != T + 1) return "the last entry of rec_start must be T + 1";
  for (int64_t r = 1; r < nrec; ++r)
    if (codes[rec_start[r] - 1] != 4) return "records must be separated by a code 4";
  return nullptr;
}
// x_max of records_unit_exp from the model's parameters W [K][4][M], b [K]
inline double records_x_max(const float* W, const float* b, int K, int M) {
  double best = 0.0;
  for (int k = 0; k < K; ++k) {
    double x = b[k];
    for (int j = 0; j < M; ++j) {
      float m = W[((size_t)k * 4) * M + j];
      for (int a = 1; a < 4; ++a) m = std::max(m, W[((size_t)k * 4 + a) * M + j]);
      x += m;
    }
    best = k == 0 ? x : std::max(best, x);
  }
  return best;
}
// records_finish: the outputs of crbm_scan_records_codes from the call's accumulators -- sums [nrec][K] in units of
// 2^-e, keys [nrec][K] (crbm_kernels.h, site_key; 0: no valid window), counts [nrec][5] (valid windows, A, C, G, T).  A
// sum becomes a float32 with one rounding; fe is formed in double, ascending k, then ascending letter, and rounded
// once.  Any output, and with it its accumulator, may be null.
inline void records_finish(int64_t nrec, int K, int ds, int e, const float* c, const unsigned long long* sums,
                           const unsigned long long* keys, const unsigned long long* counts, int64_t* windows, int64_t* letters,
                           float* fe, float* fe_per_motif, int32_t* best_start, int32_t* best_strand, float* best_prob) {
  const double unit = records_unit(e);
  for (int64_t r = 0; r < nrec; ++r) {
    if (windows) windows[r] = (int64_t)counts[5 * r];
    if (letters)
      for (int a = 0; a < 4; ++a) letters[4 * r + a] = (int64_t)counts[5 * r + 1 + a];
    if (fe_per_motif)
      for (int k = 0; k < K; ++k) {
        const unsigned long long s = sums[r * K + k];
        fe_per_motif[r * K + k] = s ? -ldexpf((float)s, -e) : 0.f;
      }
    if (fe) {
      double acc = 0.0;
      for (int k = 0; k < K; ++k) acc -= (double)sums[r * K + k] * unit;
      for (int a = 0; a < 4; ++a) acc -= (double)counts[5 * r + 1 + a] * (double)c[a];
      fe[r] = (float)acc;
    }
    for (int k = 0; k < K && keys; ++k) {
      const unsigned long long key = keys[r * K + k];
      const uint32_t low = 0xFFFFFFFFu - (uint32_t)key, bits = (uint32_t)(key >> 32);
      float p;
      memcpy(&p, &bits, 4);
      if (best_start) best_start[r * K + k] = key ? (int32_t)(low >> 1) : -1;
      if (best_strand) best_strand[r * K + k] = key && ds ? ((low & 1u) ? -1 : 1) : 0;
      if (best_prob) best_prob[r * K + k] = key ? p : 0.f;
    }
  }
}

}  // namespace crbm
