// TEST INFRASTRUCTURE: a stand-alone program that runs the kernels of crbm_amd/csrc/crbm_compare.h on CPU threads, block
// after block; tests/test_emu_compare.py builds it with ASan + UBSan and runs it directly.
// usage: compare_main <in> <out>
//   <in>   int32 op, K, N, bins, both, min_overlap, threads, tile, null_mask, nqstart, ntstart, 0; int64 budget
//          (CRBM_COMPARE_BYTES), nqcols, ntcols, 0; double invC; then int32 qstart[nqstart], tstart[ntstart]; uint16
//          qcols[nqcols][4], tcols[ntcols][4].  The arrays are as long as the header says, whatever K and N claim; bit
//          0..4 of null_mask pass a null pointer for qcols, qstart, tcols, tstart, the outputs.
//   <out>  every output between GUARD words of its own:
//          op 0 (crbm_motif_compare)       double p_min[K][N]; int32 offset; int8 strand; int32 overlap; int32 n_off
//          op 1 (crbm_motif_compare_null)  uint32 counts[m][bins]; double tail[table_elems]      (K = 1)
// The plan and the launch geometry are the header's (plan_or_refusal, count_blocks, conv_tiles, place_lds), driven as
// crbm_api.hip drives them; `threads` replaces the block size (a lane is an OS thread here).  What the entry point would
// refuse ends the program with status 3 and the reason on stderr, before the output file is opened.  Every buffer a
// kernel sees is a heap block of exactly the size the driver gives it, filled with garbage unless the driver clears it,
// the LDS exactly the bytes a launch asks for.
#include <hip/hip_runtime.h>

// what the shim does not have
static inline unsigned long long atomicMin(unsigned long long* p, unsigned long long v) {
  unsigned long long old = __atomic_load_n(p, __ATOMIC_RELAXED);
  while (old > v && !__atomic_compare_exchange_n(p, &old, v, false, __ATOMIC_RELAXED, __ATOMIC_RELAXED)) {}
  return old;
}
static inline uint32_t atomicMin(uint32_t* p, uint32_t v) {
  uint32_t old = __atomic_load_n(p, __ATOMIC_RELAXED);
  while (old > v && !__atomic_compare_exchange_n(p, &old, v, false, __ATOMIC_RELAXED, __ATOMIC_RELAXED)) {}
  return old;
}
static inline long long __double_as_longlong(double d) { long long r; __builtin_memcpy(&r, &d, 8); return r; }
static inline double __longlong_as_double(long long v) { double r; __builtin_memcpy(&r, &v, 8); return r; }

#include "crbm_compare.h"
#include "emu_launch.h"

#include <cstdio>
#include <cstdlib>
#include <cstring>

const bool emu::concurrent_blocks = false;

using namespace crbm;

static const uint32_t GUARD_WORD = 0xA5A5BEEFu;
static const int GUARD = 8;

template <typename T>
static std::vector<T> take(FILE* f, size_t n) {
  std::vector<T> v(n);
  if (n && fread(v.data(), sizeof(T), n, f) != n) { fprintf(stderr, "short input\n"); exit(2); }
  return v;
}

static int refuse(const char* why) {
  fprintf(stderr, "refused: %s\n", why);
  return 3;
}

// `bytes` of payload between guard words; the payload starts as garbage
struct Guarded {
  std::vector<unsigned char> block;
  size_t bytes;
  explicit Guarded(size_t n) : block(8 * GUARD + n, 0xCD), bytes(n) {
    for (int i = 0; i < GUARD; ++i) {
      memcpy(block.data() + 4 * i, &GUARD_WORD, 4);
      memcpy(block.data() + 4 * GUARD + n + 4 * i, &GUARD_WORD, 4);
    }
  }
  template <typename T>
  T* data() { return reinterpret_cast<T*>(block.data() + 4 * GUARD); }
  void write(FILE* g) const {
    for (int i = 0; i < GUARD; ++i) {
      uint32_t lo, hi;
      memcpy(&lo, block.data() + 4 * i, 4);
      memcpy(&hi, block.data() + 4 * GUARD + bytes + 4 * i, 4);
      if (lo != GUARD_WORD || hi != GUARD_WORD) { fprintf(stderr, "a guard word was written\n"); exit(4); }
    }
    if (fwrite(block.data(), 1, block.size(), g) != block.size()) { perror("write"); exit(2); }
  }
};

// a device buffer: exactly `count` elements on the heap, garbage
template <typename T>
static std::vector<T> device(size_t count) {
  std::vector<T> v(count);
  memset(static_cast<void*>(v.data()), 0xCD, count * sizeof(T));
  return v;
}

int main(int argc, char** argv) {
  if (argc != 3) { fprintf(stderr, "usage: %s <in> <out>\n", argv[0]); return 2; }
  FILE* f = fopen(argv[1], "rb");
  if (!f) { perror(argv[1]); return 2; }
  const std::vector<int32_t> hd = take<int32_t>(f, 12);
  const int op = hd[0], K = hd[1], N = hd[2], bins = hd[3], both = hd[4], min_overlap = hd[5], threads = hd[6], tile = hd[7], null_mask = hd[8];
  const std::vector<int64_t> wide = take<int64_t>(f, 4);
  const int64_t budget = wide[0];
  const double invC = take<double>(f, 1)[0];
  if (threads < 1 || threads > 256 || hd[9] < 1 || hd[10] < 1 || wide[1] < 0 || wide[2] < 0 || (op != 0 && op != 1)) { fprintf(stderr, "bad header\n"); return 2; }
  const std::vector<int32_t> qstart = take<int32_t>(f, (size_t)hd[9]), tstart = take<int32_t>(f, (size_t)hd[10]);
  const std::vector<uint16_t> qcols = take<uint16_t>(f, (size_t)wide[1] * 4), tcols = take<uint16_t>(f, (size_t)wide[2] * 4);
  fclose(f);
  if (op == 1 && K != 1) { fprintf(stderr, "op 1 takes one query\n"); return 2; }
  compare::Plan plan;
  if (const char* why = compare::plan_or_refusal((null_mask & 1) ? nullptr : qcols.data(), (null_mask & 2) ? nullptr : qstart.data(), K,
                                                 (null_mask & 4) ? nullptr : tcols.data(), (null_mask & 8) ? nullptr : tstart.data(), N, bins, both,
                                                 min_overlap, invC, !(null_mask & 16), budget, tile, &plan))
    return refuse(why);
  if ((size_t)K + 1 != qstart.size() || (size_t)N + 1 != tstart.size() || (size_t)qstart[(size_t)K] * 4 != qcols.size() ||
      (size_t)tstart[(size_t)N] * 4 != tcols.size()) { fprintf(stderr, "the arrays do not match K and N\n"); return 2; }

  const size_t pairs = (size_t)K * (size_t)N;
  const bool place = op == 0;
  Guarded p_min(place ? pairs * 8 : 0), offset(place ? pairs * 4 : 0), strand(place ? pairs : 0), overlap(place ? pairs * 4 : 0), n_off(place ? pairs * 4 : 0);
  Guarded counts_out(place ? 0 : (size_t)qstart[1] * bins * 4), tail_out(place ? 0 : (size_t)compare::table_elems(bins, qstart[1]) * 8);

  // (uint2 columns: the uint16 arrays copied into aligned blocks of exactly their size)
  std::vector<uint2> dq = device<uint2>((size_t)qstart[(size_t)K]), dt = device<uint2>((size_t)plan.tcols);
  memcpy(static_cast<void*>(dq.data()), qcols.data(), qcols.size() * 2);
  memcpy(static_cast<void*>(dt.data()), tcols.data(), tcols.size() * 2);
  const compare::Motifs motifs{dq.data(), qstart.data(), dt.data(), tstart.data()};
  const unsigned T = (unsigned)threads;
  for (int g = 0; g < plan.groups(); ++g) {
    const int q0 = plan.group_start[(size_t)g], rows = plan.group_start[(size_t)g + 1] - q0;
    const int wq = compare::widest(qstart.data(), q0, q0 + rows);
    // the buffers of this group, as large as the driver of crbm_api.hip makes them
    std::vector<uint32_t> dcounts = device<uint32_t>((size_t)plan.count_elems_max);
    std::vector<double> dtables = device<double>((size_t)plan.table_elems_max);
    const size_t rows_out = place ? (size_t)plan.rows_max * (size_t)N : 1;
    std::vector<double> dp = device<double>(rows_out);
    std::vector<int32_t> doff = device<int32_t>(rows_out), dovl = device<int32_t>(rows_out), dnoff = device<int32_t>(rows_out);
    std::vector<int8_t> dstrand = device<int8_t>(rows_out);
    const size_t ncounts = (size_t)(qstart[(size_t)(q0 + rows)] - qstart[(size_t)q0]) * (size_t)bins;
    memset(dcounts.data(), 0, ncounts * 4);
    compare::CountArgs c;
    c.m = motifs; c.counts = dcounts.data(); c.tcols = plan.tcols; c.q0 = q0; c.bins = bins; c.both = both;
    emu::launch([&] { compare::counts_kernel(c); }, dim3(compare::count_blocks(plan.tcols), (unsigned)rows), dim3(T), compare::counts_lds(wq, bins));
    compare::NullArgs n;
    n.qstart = qstart.data(); n.counts = dcounts.data(); n.tables = dtables.data(); n.table_base = plan.table_base.data();
    n.invC = invC; n.q0 = q0; n.bins = bins; n.l = 0; n.tiles = 0;
    for (int l = 1; l <= wq; ++l) {
      n.l = l;
      n.tiles = (int32_t)compare::conv_tiles(bins, l);
      emu::launch([&] { compare::conv_kernel(n); }, dim3((unsigned)(n.tiles * (wq - l + 1)), (unsigned)rows), dim3(T), compare::conv_lds(bins));
    }
    emu::launch([&] { compare::tail_kernel(n); }, dim3((unsigned)((wq * (wq + 1) / 2 + threads - 1) / threads), (unsigned)rows), dim3(T), 0);
    if (place) {
      compare::PlaceArgs a;
      a.m = motifs; a.tables = dtables.data(); a.table_base = plan.table_base.data();
      a.p_min = dp.data(); a.offset = doff.data(); a.strand = dstrand.data(); a.overlap = dovl.data(); a.n_off = dnoff.data();
      a.q0 = q0; a.N = N; a.bins = bins; a.both = both; a.min_overlap = min_overlap; a.tile = plan.tile;
      a.diagonals = wq + plan.width_max_targets - 1;
      emu::launch([&] { compare::place_kernel(a); }, dim3((unsigned)((N + plan.tile - 1) / plan.tile), (unsigned)rows), dim3(T),
                  compare::place_lds(plan.tile, a.diagonals));
      const size_t at = (size_t)q0 * (size_t)N, cnt = (size_t)rows * (size_t)N;
      memcpy(p_min.data<double>() + at, dp.data(), cnt * 8);
      memcpy(offset.data<int32_t>() + at, doff.data(), cnt * 4);
      memcpy(strand.data<int8_t>() + at, dstrand.data(), cnt);
      memcpy(overlap.data<int32_t>() + at, dovl.data(), cnt * 4);
      memcpy(n_off.data<int32_t>() + at, dnoff.data(), cnt * 4);
    } else {
      memcpy(counts_out.data<uint32_t>(), dcounts.data(), ncounts * 4);
      memcpy(tail_out.data<double>(), dtables.data(), tail_out.bytes);
    }
  }
  FILE* out = fopen(argv[2], "wb");
  if (!out) { perror(argv[2]); return 2; }
  if (place) { p_min.write(out); offset.write(out); strand.write(out); overlap.write(out); n_off.write(out); }
  else { counts_out.write(out); tail_out.write(out); }
  fclose(out);
  return 0;
}
