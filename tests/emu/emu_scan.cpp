// TEST INFRASTRUCTURE: runs the stream-scan kernels of crbm_amd/csrc/crbm_kernels.h (scan_encode_kernel, scan_sites_body
// in both passes, scan_offsets_kernel) on CPU threads under ASan/UBSan, like emu_sites.cpp does for the motif-site
// kernels.  Every buffer has exactly the size of scan_layout (crbm_layout.h), so that ASan sees any overrun.  Plain C
// entry points for tests/test_emu_scan.py (ctypes).
#define CRBM_DEFINE_MISC_KERNELS
#include "crbm_kernels.h"
#include "emu_launch.h"

#include <cstring>

// all blocks of the grid at once, as concurrent OS threads
const bool emu::concurrent_blocks = true;

using namespace crbm;

// the model configurations of the scan cases (K, M, DS, G)
#define SCAN_DISPATCH(id, ...)                                           \
  switch (id) {                                                          \
    case 0: { using C = Cfg<10, 15, 1, 3>; __VA_ARGS__; break; }         \
    case 1: { using C = Cfg<10, 5, 0, 2>; __VA_ARGS__; break; }          \
    case 2: { using C = Cfg<6, 1, 1, 1>; __VA_ARGS__; break; }           \
    case 3: { using C = Cfg<20, 15, 1, 2>; __VA_ARGS__; break; }         /* two groups of quads */ \
    case 4: { using C = Cfg<36, 6, 0, 2>; __VA_ARGS__; break; }          /* three */ \
    case 5: { using C = Cfg<5, 40, 1, 2>; __VA_ARGS__; break; }          /* a window of two 64-bit words */ \
    default: return -1;                                                  \
  }

extern "C" {

int emu_scan_info(int id, int* out) {   // K, M, DS, TABLES
  SCAN_DISPATCH(id, (out[0] = C::K, out[1] = C::M, out[2] = C::DS, out[3] = C::TABLES_ALL));
  return 0;
}

int emu_scan_tables(int id, const float* W, const float* b, const float* c, float* out) {
  SCAN_DISPATCH(id, emu::build_tables<C>(W, b, c, out));
  return 0;
}

// The whole scan of a stream of T codes as one segment: encode, count, offsets, write.  recs holds `capacity` records
// (plus whatever guard the caller keeps behind them); *count gets the exact total, *flags the encode kernel's flag.
// valid_out / letters_out (optional) receive the planes of scan_layout.  Returns the number of tiles, -2 for T < M.
int emu_scan_run(int id, const float* tables, const unsigned char* codes, long T, float threshold, SiteRec* recs,
                 unsigned long long capacity, unsigned long long* count, uint32_t* flags, int grid, int threads,
                 unsigned long long* valid_out, uint32_t* letters_out) {
  int M = 0, tab = 0, K = 0;
  SCAN_DISPATCH(id, (M = C::M, tab = C::TAB, K = C::K));
  if (T < M) return -2;
  const long starts = T - M + 1;
  const ScanLayout l = scan_layout(T, starts);
  std::vector<uint32_t> staged((size_t)(T + 3) / 4);                    // 4-byte aligned, as the driver's staging buffer
  std::memcpy(staged.data(), codes, (size_t)T);
  std::vector<uint32_t> letters((size_t)l.letter_words, 0xDEADBEEFu);
  std::vector<unsigned long long> valid((size_t)l.valid_words, ~0ull);
  std::vector<unsigned short> lanes((size_t)64 * l.tiles, 0xFFFFu);
  std::vector<uint32_t> tiles((size_t)l.tiles, 0xFFFFFFFFu);
  std::vector<unsigned long long> off((size_t)l.tiles + 1, ~0ull);
  ScanEncodeArgs e{reinterpret_cast<const unsigned char*>(staged.data()), letters.data(), valid.data(), flags, T, l.valid_words};
  // the encode kernel reads whole 32-bit words only where four codes exist: hand it the exact byte count
  emu::launch([&] { scan_encode_kernel(e); }, dim3(2), dim3(64), 0);
  if (valid_out) std::memcpy(valid_out, valid.data(), valid.size() * 8);
  if (letters_out) std::memcpy(letters_out, letters.data(), letters.size() * 4);
  ScanArgs a{ScanInput{tables, letters.data(), valid.data(), (int)starts, l.tiles, 0, SlabPlan{K, K, 0}}};
  a.lane_cnt = lanes.data(); a.tile_cnt = tiles.data(); a.tile_off = off.data();
  a.recs = recs; a.capacity = capacity;
  a.pos0 = 0; a.pass = 0; a.threshold = threshold; a.pad_ = 0;
  SCAN_DISPATCH(id, emu::launch([&] { scan_sites_body<C>(a); }, dim3(grid), dim3(threads), (size_t)tab * 4));
  ScanOffsetsArgs o{tiles.data(), off.data(), off.data() + l.tiles, l.tiles};
  emu::launch([&] { scan_offsets_kernel(o); }, dim3(1), dim3(128), 128 * 8);
  *count = off[(size_t)l.tiles];
  if (recs) {
    a.pass = 1;
    SCAN_DISPATCH(id, emu::launch([&] { scan_sites_body<C>(a); }, dim3(grid), dim3(threads), (size_t)tab * 4));
  }
  return l.tiles;
}

}  // extern "C"
