// TEST INFRASTRUCTURE: a stand-alone program that runs the kernels of crbm_amd/csrc/crbm_null.h on CPU threads, block
// after block; tests/test_emu_null.py builds it with ASan + UBSan and runs it directly.
// usage: null_main <in> <out>
//   <in>   int32 op, R, M, order, variant, threads, 0, 0; int64 G, budget (CRBM_NULL_BYTES), tile (CRBM_NULL_TILE), 0; then
//          int32 q[R][M][4]; double trans[contexts][4]; double init[contexts]
//   <out>  GUARD words, the output, GUARD words:
//          op 0 (the distribution)        double pmf[R][G]
//          op 1 (the predecessor table)   per context and slot three doubles: source, letter, probability
// The plan, the table and the launches of every position are the header's (plan_or_refusal, build_table, step_launches),
// as crbm_api.hip drives them; `threads` replaces the block size (a lane is an OS thread here).  What the entry point
// would refuse ends the program with status 3 and the reason on stderr, before the output file is opened.  Every buffer
// a kernel sees is a heap block of exactly the size the driver gives it, the LDS exactly the bytes a launch asks for.
#include "crbm_null.h"
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

// doubles between guard words: the results land here, the guards are checked, and the whole block is the file
struct Guarded {
  std::vector<uint64_t> words;
  size_t count;
  explicit Guarded(size_t n) : words(GUARD + n, 0xCDCDCDCDCDCDCDCDull), count(n) {
    uint32_t* w = reinterpret_cast<uint32_t*>(words.data());
    for (int i = 0; i < GUARD; ++i) w[i] = w[2 * words.size() - 1 - i] = GUARD_WORD;
  }
  double* data() { return reinterpret_cast<double*>(words.data() + GUARD / 2); }
  void write(const char* path) const {
    const uint32_t* w = reinterpret_cast<const uint32_t*>(words.data());
    for (int i = 0; i < GUARD; ++i)
      if (w[i] != GUARD_WORD || w[2 * words.size() - 1 - i] != GUARD_WORD) { fprintf(stderr, "a guard word was written\n"); exit(4); }
    FILE* g = fopen(path, "wb");
    if (!g) { perror(path); exit(2); }
    if (fwrite(words.data(), 8, words.size(), g) != words.size()) { perror("write"); exit(2); }
    fclose(g);
  }
};

int main(int argc, char** argv) {
  if (argc != 3) { fprintf(stderr, "usage: %s <in> <out>\n", argv[0]); return 2; }
  FILE* f = fopen(argv[1], "rb");
  if (!f) { perror(argv[1]); return 2; }
  const std::vector<int32_t> hd = take<int32_t>(f, 8);
  const int op = hd[0], R = hd[1], M = hd[2], order = hd[3], variant = hd[4], threads = hd[5];
  const std::vector<int64_t> wide = take<int64_t>(f, 4);
  const int64_t G = wide[0], budget = wide[1], tile = wide[2];
  if (threads < 1 || threads > 256 || G > (1 << 20)) { fprintf(stderr, "bad header\n"); return 2; }
  int dummy = 0;
  if (R < 1 || M < 1 || M > null::MAX_M || order < 0 || order > null::MAX_ORDER)    // before anything is read by these sizes
    return refuse(null::plan_or_refusal(&dummy, R, M, order, reinterpret_cast<const double*>(&dummy), reinterpret_cast<const double*>(&dummy),
                                        G, &dummy, budget, tile, nullptr));
  const int NS = null::contexts(order);
  const std::vector<int32_t> q = take<int32_t>(f, (size_t)R * M * 4);
  const std::vector<double> trans = take<double>(f, (size_t)NS * 4), init = take<double>(f, (size_t)NS);
  fclose(f);
  if (op == 1) {
    std::vector<null::Pred> table((size_t)NS * null::PREDS);
    null::build_table(order, trans.data(), table.data());
    Guarded out((size_t)NS * null::PREDS * 3);
    for (size_t e = 0; e < table.size(); ++e) {
      out.data()[3 * e] = table[e].src; out.data()[3 * e + 1] = table[e].letter; out.data()[3 * e + 2] = table[e].prob;
    }
    out.write(argv[2]);
    return 0;
  }
  if (op != 0) { fprintf(stderr, "unknown op %d\n", op); return 2; }
  null::Plan plan;
  if (const char* why = null::plan_or_refusal(q.data(), R, M, order, trans.data(), init.data(), G, &dummy, budget, tile, &plan)) return refuse(why);
  Guarded pmf((size_t)R * (size_t)G);
  std::vector<null::Pred> table((size_t)NS * null::PREDS);
  null::build_table(order, trans.data(), table.data());
  const int rpg = plan.rows_per_group;
  for (int row0 = 0; row0 < R; row0 += rpg) {
    const int rows = std::min(rpg, R - row0);
    // the buffers of this group, exactly as large as the driver of crbm_api.hip makes them; never cleared
    std::vector<double> state[2] = {std::vector<double>((size_t)plan.state_elems, 7.0), std::vector<double>((size_t)plan.state_elems, 7.0)};
    std::vector<double> gpmf((size_t)rows * (size_t)G, 7.0);
    const std::vector<int32_t> gq(q.begin() + (size_t)row0 * M * 4, q.begin() + (size_t)(row0 + rows) * M * 4);
    const std::vector<int32_t> greach(plan.reach.begin() + (size_t)row0 * (M + 1), plan.reach.begin() + (size_t)(row0 + rows) * (M + 1));
    null::EdgeArgs e;
    e.state = state[0].data(); e.init = init.data(); e.pmf = gpmf.data(); e.reach = greach.data();
    e.gmax = plan.gmax; e.G = G; e.M = M; e.tile = plan.tile; e.contexts = NS; e.rows = rows;
    emu::launch([&] { null::start_kernel(e); }, dim3((unsigned)((rows * NS + threads - 1) / threads)), dim3((unsigned)threads), 0);
    for (int j = 0; j < M; ++j) {
      null::Launch launches[2];
      const int n = null::step_launches(plan, q.data(), M, order, variant, row0, rows, j, launches);
      for (int i = 0; i < n; ++i) {
        const null::Launch& l = launches[i];
        if (l.gy == 0) continue;
        null::StepArgs a;
        a.src = state[j & 1].data(); a.dst = state[(j & 1) ^ 1].data();
        a.q = gq.data(); a.reach = greach.data(); a.table = table.data();
        a.gmax = plan.gmax; a.M = M; a.j = j; a.tile = plan.tile; a.contexts = NS;
        a.ctx0 = l.ctx0; a.nctx = l.nctx; a.lds_width = l.lds_width;
        if (l.siblings) emu::launch([&] { null::step_siblings_kernel(a); }, dim3(l.gx, l.gy), dim3((unsigned)threads), l.lds);
        else emu::launch([&] { null::step_plain_kernel(a); }, dim3(l.gx, l.gy), dim3((unsigned)threads), 0);
      }
    }
    e.state = state[M & 1].data();
    emu::launch([&] { null::marginal_kernel(e); }, dim3((unsigned)((G + plan.tile - 1) / plan.tile), (unsigned)rows), dim3((unsigned)threads), 0);
    memcpy(pmf.data() + (size_t)row0 * (size_t)G, gpmf.data(), gpmf.size() * 8);
  }
  pmf.write(argv[2]);
  return 0;
}
