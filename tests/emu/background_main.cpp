// TEST INFRASTRUCTURE: a stand-alone program that runs the kernels of crbm_amd/csrc/crbm_background.h on CPU threads,
// block after block; tests/test_emu_background.py builds it with ASan + UBSan and runs it directly.
// usage: background_main <in> <out>
//   <in>   int32 op, order, grid, threads, chunk, has_template, segment, 0; int64 T, pos0; uint64 seed; then
//          op 0 (j-mer counts):  uint8 codes[T]
//          op 1 (sampling):      uint32 thr[contexts][3]; uint8 template[T] if has_template
//   <out>  GUARD words, the output, GUARD words: op 0 uint64 counts[kmer_slots], op 1 uint8 codes[T] (no padding).
// segment: positions per segment (0: one segment), as the driver of crbm_api.hip cuts a long stream: a halo of `order`
// codes for the counts, the carried context for the sampler.
// What the entry point would refuse (crbm_background.h, *_refusal) ends the program with status 3 and the reason on
// stderr, before the output file is opened.  Every buffer a kernel sees is a heap block of exactly the size the driver
// gives it, the LDS exactly the bytes it asks for.
#include "crbm_background.h"
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

static void write_guarded(const char* path, const void* data, size_t bytes) {
  FILE* g = fopen(path, "wb");
  if (!g) { perror(path); exit(2); }
  uint32_t guard[GUARD];
  for (int i = 0; i < GUARD; ++i) guard[i] = GUARD_WORD;
  if (fwrite(guard, 4, GUARD, g) != (size_t)GUARD || (bytes && fwrite(data, 1, bytes, g) != bytes) || fwrite(guard, 4, GUARD, g) != (size_t)GUARD) {
    perror("write");
    exit(2);
  }
  fclose(g);
}

// an output between guard words in memory: the kernels' results land here, and the guards are checked before it is written
struct Guarded {
  std::vector<uint32_t> words;
  size_t bytes;
  explicit Guarded(size_t n) : words(2 * GUARD + (n + 3) / 4, 0xCDCDCDCDu), bytes(n) {
    for (int i = 0; i < GUARD; ++i) words[i] = words[words.size() - 1 - i] = GUARD_WORD;
  }
  uint8_t* data() { return reinterpret_cast<uint8_t*>(words.data() + GUARD); }
  void check() const {
    for (int i = 0; i < GUARD; ++i)
      if (words[i] != GUARD_WORD || words[words.size() - 1 - i] != GUARD_WORD) { fprintf(stderr, "a guard word was written\n"); exit(4); }
    const uint8_t* p = reinterpret_cast<const uint8_t*>(words.data() + GUARD);
    for (size_t i = bytes; i < (bytes + 3) / 4 * 4; ++i)
      if (p[i] != 0xCD) { fprintf(stderr, "a byte behind the output was written\n"); exit(4); }
  }
};

template <int ORDER>
static void sample_segment(const bg::SampleArgs& a, int grid, int threads) {
  constexpr int NS = bg::contexts(ORDER);
  emu::launch([&] { bg::sample_maps_kernel<ORDER>(a); }, dim3(grid), dim3(threads), NS * 16);
  emu::launch([&] { bg::sample_groups_kernel<ORDER>(a); }, dim3(grid), dim3(threads), 0);
  emu::launch([&] { bg::sample_walk_kernel<ORDER>(a); }, dim3(1), dim3(threads), bg::WALK_TILE * NS);
  emu::launch([&] { bg::sample_entries_kernel<ORDER>(a); }, dim3(grid), dim3(threads), 0);
  emu::launch([&] { bg::sample_letters_kernel<ORDER>(a); }, dim3(grid), dim3(threads), NS * 16);
}

int main(int argc, char** argv) {
  if (argc != 3) { fprintf(stderr, "usage: %s <in> <out>\n", argv[0]); return 2; }
  FILE* f = fopen(argv[1], "rb");
  if (!f) { perror(argv[1]); return 2; }
  const std::vector<int32_t> hd = take<int32_t>(f, 8);
  const int op = hd[0], order = hd[1], grid = hd[2], threads = hd[3], has_template = hd[5];
  const std::vector<int64_t> wide = take<int64_t>(f, 2);
  const int64_t T = wide[0], pos0 = wide[1];
  const uint64_t seed = take<uint64_t>(f, 1)[0];
  if (grid < 1 || grid > 64 || threads < 64 || threads > 256 || threads % 64 != 0 || T > (1 << 24)) { fprintf(stderr, "bad header\n"); return 2; }
  const int64_t seg = hd[6] > 0 ? hd[6] : (T > 0 ? T : 1);
  if (op == 0) {
    if (order < 0 || order > bg::MAX_ORDER || T < 0) return refuse(bg::counts_refusal(nullptr, T, order, &op));
    const std::vector<uint8_t> codes = take<uint8_t>(f, (size_t)T);
    Guarded counts((size_t)bg::kmer_slots(order) * 8);
    if (const char* why = bg::counts_refusal(codes.data(), T, order, counts.data())) return refuse(why);
    std::vector<unsigned long long> acc((size_t)bg::kmer_slots(order), 0ull);
    for (int64_t start = 0; start < T; start += seg) {
      const int64_t cnt = std::min(seg, T - start), n = std::min(cnt + order, T - start);
      const std::vector<uint8_t> staged(codes.begin() + start, codes.begin() + start + n);
      const bg::KmerArgs a{staged.data(), acc.data(), n, cnt, order};
      emu::launch([&] { bg::kmer_count_kernel(a); }, dim3(grid), dim3(threads), (size_t)bg::kmer_slots(order) * 4);
    }
    memcpy(counts.data(), acc.data(), acc.size() * 8);
    counts.check();
    write_guarded(argv[2], counts.data(), counts.bytes);
  } else if (op == 1) {
    if (order < 0 || order > bg::MAX_ORDER || T < 0) return refuse(bg::sample_refusal(nullptr, order, T, pos0, nullptr, &op));
    const int NS = bg::contexts(order), chunk = bg::chunk_length(hd[4]);
    const std::vector<uint32_t> thr = take<uint32_t>(f, (size_t)NS * 3);
    const std::vector<uint8_t> tmpl = take<uint8_t>(f, has_template ? (size_t)T : 0);
    Guarded out((size_t)T);
    if (const char* why = bg::sample_refusal(thr.data(), order, T, pos0, has_template ? tmpl.data() : nullptr, out.data())) return refuse(why);
    std::vector<uint32_t> rows((size_t)NS * 4);
    bg::build_rows(thr.data(), order, rows.data());
    std::vector<uint4> drows((size_t)NS);
    memcpy(drows.data(), rows.data(), rows.size() * 4);
    std::vector<uint32_t> carry(1, 0u);                      // the empty context (a word: the allocation is 4-byte aligned)
    for (int64_t start = 0; start < T; start += seg) {
      const int64_t cnt = std::min(seg, T - start), chunks = (cnt + chunk - 1) / chunk, groups = (chunks + bg::GROUP - 1) / bg::GROUP;
      std::vector<uint8_t> cmap((size_t)chunks * NS), gmap((size_t)groups * NS), centry((size_t)chunks), gentry((size_t)groups);
      // the codes of the segment in blocks of their own, cnt bytes each (operator new aligns them to 16 bytes: the
      // accesses of whole words of four codes are aligned, and ASan's red zone starts right behind byte cnt)
      std::vector<uint8_t> tmpl_exact, out_exact;
      tmpl_exact.assign(tmpl.begin() + (has_template ? start : 0), tmpl.begin() + (has_template ? start + cnt : 0));
      out_exact.assign((size_t)cnt, 0xCD);
      bg::SampleArgs a;
      a.rows = drows.data(); a.tmpl = has_template ? tmpl_exact.data() : nullptr; a.out = out_exact.data();
      a.cmap = cmap.data(); a.gmap = gmap.data(); a.centry = centry.data(); a.gentry = gentry.data();
      a.carry = reinterpret_cast<uint8_t*>(carry.data());
      a.n = cnt; a.pos0 = pos0 + start; a.chunks = chunks; a.groups = groups; a.chunk = chunk;
      a.seed_lo = (uint32_t)(seed & 0xffffffffu); a.seed_hi = (uint32_t)(seed >> 32);
      switch (order) {
        case 0: sample_segment<0>(a, grid, threads); break;
        case 1: sample_segment<1>(a, grid, threads); break;
        case 2: sample_segment<2>(a, grid, threads); break;
        default: sample_segment<3>(a, grid, threads); break;
      }
      memcpy(out.data() + start, out_exact.data(), (size_t)cnt);
    }
    out.check();
    write_guarded(argv[2], out.data(), out.bytes);
  } else {
    fprintf(stderr, "unknown op %d\n", op);
    return 2;
  }
  fclose(f);
  return 0;
}
