// TEST INFRASTRUCTURE: a stand-alone program that runs the t-SNE kernels of crbm_amd/csrc/crbm_tsne.h on CPU threads,
// block after block; tests/test_emu_tsne.py builds it with ASan + UBSan and runs it directly.
// usage: tsne_main <in> <out>
//   <in>   int32 op, n, a, k, grid, threads, flags, 0, then
//          op 0 (neighbours, a = D):      float32 X[n][D]
//          op 1 (affinities):             float32 perplexity, d2[n][k]
//          op 2 (descent, a = iterations; flags 1: gradient, 2: KL and Z):  float32 exaggeration, learning rate, momentum;
//                                         int64 indptr[n + 1]; int32 indices[nnz]; float32 values[nnz], y[n][2],
//                                         velocity[n][2], gains[n][2]
//   <out>  32-bit words: per output array GUARD words, the array, GUARD words.  op 0: idx, d2.  op 1: p, beta.
//          op 2: y, the other position buffer, velocity, gains, gradient, then Z and KL as two float64 (the last three
//          as they were allocated when not asked for).
// What the entry point would refuse (crbm_tsne.h, *_refusal) ends the program with status 3 and the reason on stderr.
// Every buffer has exactly the size the driver gives it (crbm_api.hip), the LDS exactly the bytes it asks for; the
// launches are the driver's, with the grid and the block size of the header.
#include "crbm_tsne.h"
#include "emu_launch.h"

#include <cstdio>
#include <cstdlib>
#include <cstring>

const bool emu::concurrent_blocks = false;

using namespace crbm;

static const uint32_t GUARD_WORD = 0xA5A5BEEFu;
static const int GUARD = 8;

// an output array between guard words
template <typename T>
struct Guarded {
  std::vector<uint32_t> words;
  size_t count;
  explicit Guarded(size_t n) : words(2 * GUARD + n * sizeof(T) / 4, 0xCDCDCDCDu), count(n) {
    for (int i = 0; i < GUARD; ++i) words[i] = words[words.size() - 1 - i] = GUARD_WORD;
  }
  T* data() { return reinterpret_cast<T*>(words.data() + GUARD); }
  void write(FILE* f) {
    if (fwrite(words.data(), 4, words.size(), f) != words.size()) { perror("write"); exit(2); }
  }
};

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

int main(int argc, char** argv) {
  if (argc != 3) { fprintf(stderr, "usage: %s <in> <out>\n", argv[0]); return 2; }
  FILE* f = fopen(argv[1], "rb");
  if (!f) { perror(argv[1]); return 2; }
  const std::vector<int32_t> hd = take<int32_t>(f, 8);
  const int op = hd[0], arg = hd[2], k = hd[3], grid = hd[4], threads = hd[5], flags = hd[6];
  const int64_t n = hd[1];
  if (grid < 1 || grid > 64 || threads < 64 || threads > 512 || threads % 64 != 0) { fprintf(stderr, "bad header\n"); return 2; }
  FILE* g = fopen(argv[2], "wb");
  if (!g) { perror(argv[2]); return 2; }
  if (op == 0) {
    const int D = arg;
    if (const char* why = tsne::neighbors_refusal(n, D, k)) return refuse(why);
    const std::vector<float> X = take<float>(f, (size_t)n * D);
    Guarded<int32_t> idx((size_t)n * k);
    Guarded<float> d2((size_t)n * k);
    const tsne::KnnArgs a{X.data(), idx.data(), d2.data(), (int)n, D, k};
    emu::launch([&] { tsne::tsne_knn_kernel(a); }, dim3(grid), dim3(threads), tsne::knn_lds_bytes(D, k, threads / 64));
    idx.write(g);
    d2.write(g);
  } else if (op == 1) {
    const float perplexity = take<float>(f, 1)[0];
    if (const char* why = tsne::affinities_refusal(n, k, perplexity)) return refuse(why);
    const std::vector<float> d2 = take<float>(f, (size_t)n * k);
    Guarded<float> p((size_t)n * k), beta((size_t)n);
    const tsne::AffinityArgs a{d2.data(), p.data(), beta.data(), (int)n, k, log((double)perplexity)};
    emu::launch([&] { tsne::tsne_affinity_kernel(a); }, dim3(grid), dim3(threads), 0);
    p.write(g);
    beta.write(g);
  } else if (op == 2) {
    const int iterations = arg;
    const std::vector<float> hyper = take<float>(f, 3);
    if (n < 2 || n > tsne::MAX_N) return refuse("t-SNE needs at least two rows");
    const std::vector<int64_t> indptr = take<int64_t>(f, (size_t)n + 1);
    if (indptr[0] != 0 || indptr[n] < 0 || indptr[n] > (1 << 26)) return refuse("indptr must start at 0 and ascend");
    const size_t nnz = (size_t)indptr[n];
    const std::vector<int32_t> indices = take<int32_t>(f, nnz);
    const std::vector<float> values = take<float>(f, nnz);
    if (const char* why = tsne::descend_refusal(n, indptr.data(), indices.data(), iterations)) return refuse(why);
    Guarded<float2> y0((size_t)n), y1((size_t)n), vel((size_t)n), gains((size_t)n), grad((size_t)n);
    Guarded<double> scalars(2);
    const std::vector<float> yin = take<float>(f, (size_t)n * 2), vin = take<float>(f, (size_t)n * 2), gin = take<float>(f, (size_t)n * 2);
    memcpy(y0.data(), yin.data(), (size_t)n * 8);
    memcpy(vel.data(), vin.data(), (size_t)n * 8);
    memcpy(gains.data(), gin.data(), (size_t)n * 8);
    const int S = tsne::slices(n);
    const int64_t chunks = tsne::sum_chunks(n);
    std::vector<float4> part((size_t)n * S), rs((size_t)n);
    std::vector<double> chunk((size_t)chunks), klrow((size_t)n);
    scalars.data()[0] = scalars.data()[1] = 0.0;
    Guarded<float2>* yb[2] = {&y0, &y1};
    int cur = 0;
    const int passes = iterations > 0 ? iterations : 1;
    for (int it = 0; it < passes; ++it) {
      const bool last = it == passes - 1;
      const tsne::RepulsionArgs ra{yb[cur]->data(), part.data(), (int)n, S, tsne::slice_tiles(n)};
      emu::launch([&] { tsne::tsne_repulsion_kernel(ra); }, dim3(grid, S), dim3(std::min(threads, 256)), tsne::TJ * 8);
      const tsne::CombineArgs ca{part.data(), rs.data(), chunk.data(), (int)n, S};
      emu::launch([&] { tsne::tsne_combine_kernel(ca); }, dim3(grid), dim3(threads), tsne::SUM_CHUNK * 8);
      const tsne::SumArgs za{chunk.data(), scalars.data(), chunks};
      emu::launch([&] { tsne::tsne_final_sum_kernel(za); }, dim3(1), dim3(threads), tsne::SUM_CHUNK * 8);
      const bool want_kl = last && (flags & 2);
      const tsne::StepArgs sa{indptr.data(), indices.data(), values.data(), yb[cur]->data(), yb[cur ^ 1]->data(), vel.data(),
                              gains.data(), rs.data(), scalars.data(), (last && (flags & 1)) ? grad.data() : nullptr,
                              want_kl ? klrow.data() : nullptr, (int)n, iterations > 0 ? 1 : 0, hyper[0], hyper[1], hyper[2]};
      emu::launch([&] { tsne::tsne_step_kernel(sa); }, dim3(grid), dim3(threads), 0);
      if (want_kl) {
        const tsne::SumArgs ka{klrow.data(), chunk.data(), n};
        emu::launch([&] { tsne::tsne_chunk_sum_kernel(ka); }, dim3(grid), dim3(threads), tsne::SUM_CHUNK * 8);
        const tsne::SumArgs kf{chunk.data(), scalars.data() + 1, chunks};
        emu::launch([&] { tsne::tsne_final_sum_kernel(kf); }, dim3(1), dim3(threads), tsne::SUM_CHUNK * 8);
      }
      if (iterations > 0) cur ^= 1;
    }
    yb[cur]->write(g);
    yb[cur ^ 1]->write(g);                            // the other buffer: its guard words count too
    vel.write(g);
    gains.write(g);
    grad.write(g);
    scalars.write(g);
  } else {
    fprintf(stderr, "unknown op %d\n", op);
    return 2;
  }
  fclose(f);
  fclose(g);
  return 0;
}
