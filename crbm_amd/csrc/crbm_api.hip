// Host side of the C-ABI declared in include/crbm_amd.h: owns device memory,
// the HIP stream and (optionally) the RCCL communicator of one GPU, and turns
// each entry point into kernel launches.  No torch, no Python types.
#define CRBM_DEFINE_MISC_KERNELS
#include "crbm_kernels.h"
#include "crbm_own.h"
#include "crbm_jit.h"
#include "crbm_plan.h"
#include "crbm_sweep.h"
#include "crbm_tsne.h"
#include "crbm_background.h"
#include "crbm_null.h"
#include "crbm_compare.h"
#include "../../include/crbm_amd.h"

#include <dlfcn.h>
#include <rccl/rccl.h>

#include <algorithm>
#include <chrono>
#include <condition_variable>
#include <deque>
#include <memory>
#include <mutex>
#include <thread>
#include <climits>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

using namespace crbm;

namespace {

std::string g_create_error;

// ---- RCCL, loaded on demand so that the library itself has no link-time
// dependency on it (single-GPU users never touch it) --------------------------
struct RcclApi {
  void* lib = nullptr;
  ncclResult_t (*GetUniqueId)(ncclUniqueId*) = nullptr;
  ncclResult_t (*CommInitRank)(ncclComm_t*, int, ncclUniqueId, int) = nullptr;
  ncclResult_t (*CommDestroy)(ncclComm_t) = nullptr;
  ncclResult_t (*AllReduce)(const void*, void*, size_t, ncclDataType_t, ncclRedOp_t, ncclComm_t, hipStream_t) = nullptr;
  ncclResult_t (*Broadcast)(const void*, void*, size_t, ncclDataType_t, int, ncclComm_t, hipStream_t) = nullptr;
  const char* (*GetErrorString)(ncclResult_t) = nullptr;
  std::string error;
};
RcclApi g_rccl;

bool load_rccl() {
  if (g_rccl.lib) return true;
  const char* names[] = {"librccl.so.1", "librccl.so", "/opt/rocm/lib/librccl.so"};
  for (const char* n : names) {
    g_rccl.lib = dlopen(n, RTLD_NOW | RTLD_GLOBAL);
    if (g_rccl.lib) break;
  }
  if (!g_rccl.lib) {
    g_rccl.error = std::string("cannot dlopen librccl: ") + dlerror();
    return false;
  }
#define CRBM_SYM(field, name)                                                    \
  g_rccl.field = reinterpret_cast<decltype(g_rccl.field)>(dlsym(g_rccl.lib, name)); \
  if (!g_rccl.field) {                                                           \
    g_rccl.error = std::string("librccl lacks ") + name;                         \
    dlclose(g_rccl.lib);                                                         \
    g_rccl.lib = nullptr;                                                        \
    return false;                                                                \
  }
  CRBM_SYM(GetUniqueId, "ncclGetUniqueId")
  CRBM_SYM(CommInitRank, "ncclCommInitRank")
  CRBM_SYM(CommDestroy, "ncclCommDestroy")
  CRBM_SYM(AllReduce, "ncclAllReduce")
  CRBM_SYM(Broadcast, "ncclBroadcast")
  CRBM_SYM(GetErrorString, "ncclGetErrorString")
#undef CRBM_SYM
  return true;
}

}  // namespace

// The slab model of a generic DNA model (LaunchPlan::slab_K): its shape, its specialised kernels, the partial rows of its
// statistics and, per set of a two-stream sweep, the per-motif scratch of its free energies.
struct SlabModel {
  int K = 0;
  crbm::ModelShape ms = {};
  crbm::JitKernels jk;
  DevBuf<float> partials, partials2, fe_scratch[2];
};

// One host thread per extra partition of the plain chain launches (LaunchPlan::chain_parts): it enqueues that
// partition's launches on the partition's stream while the caller's thread enqueues partition 0's.  Alternating two
// streams from ONE thread costs ~6 us of host time per launch (2.6 us when a thread stays on one stream), which at two
// launches per 17.6-us step leaves the GPU waiting for the host in short bursts.
struct PartJob {
  hipFunction_t fn;
  crbm::GibbsArgs args;
  unsigned grid, threads, lds;
  unsigned long long delay_ticks;   // > 0: a delay kernel in front (the partition starts this much later)
};
struct PartWorker {
  std::thread th;
  std::mutex mu;
  std::condition_variable cv, idle_cv;
  std::deque<PartJob> jobs;
  bool stop = false, busy = false;
  hipError_t error = hipSuccess;
  int device = 0;
  hipStream_t stream = nullptr;
  ~PartWorker() {                      // the thread enqueues the jobs it still holds, then ends
    { std::lock_guard<std::mutex> lock(mu); stop = true; }
    cv.notify_one();
    if (th.joinable()) th.join();
  }
};
// One partition beyond the first (partition 0 is the caller's thread on the handle's main stream and owns nothing here).
// Members go in reverse: the thread is joined first -- nothing enqueues any more -- then the stream (synchronised), then the event.
struct Partition {
  Event done;
  Stream stream;
  std::unique_ptr<PartWorker> worker;
};

// Ownership: every GPU resource is a member that releases itself (crbm_own.h); crbm_destroy deletes the handle and names
// none of them.  Members go in reverse order of declaration, so the order is part of the design: code objects and buffers
// first, then events, streams and, last, the partitions.  Deleting a handle thus joins the partitions' threads, synchronises
// and destroys their streams, then stream2 and stream, then the events, closes the mapped peer buffers and only then frees
// buffers and unloads code objects: nothing goes while a stream may still run work that uses it.  New buffers: above `err`.
struct crbm_handle {
  crbm_config cfg;
  int K = 0, M = 0, ds = 0, NW = 0, KAM = 0;
  int A = 4;                // letters of the alphabet (input_dims); anything but 4 runs on the generic kernels, rows of bytes
  int Lf = 0, Lv = 0, B = 0;
  int device = 0, num_cu = 256;
  bool overlap = false;
  // which kernels the model takes, the geometry of its chain launches, what its kernels are compiled with (crbm_plan.h:
  // the plan crbm_precompile compiled for); launches name the ChainGeom they mean, nothing here changes after crbm_create
  LaunchPlan plan;
  bool big() const { return plan.big; }              // the generic "big" kernels (crbm_kernels.h) serve every entry point
  const ModelShape& ms() const { return plan.ms; }
  JitKernels jk;            // kernels specialised for this model (hiprtc)
  DevBuf<float> d_tables;      // precomputed LDS images (gather / top-down tables, c)
  DevBuf<float> d_tf_solo;     // gather table in the solo grouping (plan.GS != plan.G only), rebuilt lazily before a plain chain launch
  bool tables_dirty = true;
  uint64_t params_version = 1, tf_solo_version = 0;   // bumped with every change of W, b, c / version d_tf_solo was built from
  // parameters and optimiser state
  DevBuf<float> dW, db, dc, dvW, dvb, dvc;
  // the update writes into a second set of buffers; the two sets swap after every step (launch_update)
  DevBuf<float> dW2, db2, dc2, dvW2, dvb2, dvc2;
  // persistent chains: K-bit masks per hidden position, letters of the last visible sample
  DevBuf<uint32_t> d_hm, d_hmp, d_vf, d_flags;
  DevBuf<unsigned long long> d_ones;
  DevBuf<float> stage, stage2, out_a, out_b, out_c;
  DevBuf<uint32_t> letters, letters2, masks_tmp;   // (…2: second set of the double-buffered host-input sweeps)
  DevBuf<float> out_a2, out_b2;
  DevBuf<uint32_t> dataset[CRBM_DATASET_SLOTS];   // resident data sets (slot 0: training, slot 1: test by convention)
  DevBuf<float> partials, partials2;
  DevBuf<unsigned long long> eval_ones;            // sampled ones per mini-batch (crbm_eval_epoch_resident)
  // What the features keep per set of a two-stream sweep (reached through sweep_set, never indexed beside it).  Motif
  // sites: records, the slab's record counter, the best-site keys of the slab's (seq, motif).  Mutagenesis: dF and pll of a
  // slab, and the expanded rows (base rows and their single-substitution copies) of the general path.
  struct SetBufs {
    DevBuf<SiteRec> site_recs;
    DevBuf<unsigned long long> site_count, site_keys;
    DevBuf<float> mut_df, mut_pll;
    DevBuf<uint32_t> mut_rows;
    // stream scan: validity plane of the segment, per-lane and per-tile hit counts, tile offsets and (behind them) the totals
    DevBuf<unsigned long long> scan_valid, scan_off;
    DevBuf<unsigned short> scan_lanes;
    DevBuf<uint32_t> scan_tiles;
    DevBuf<int32_t> var_windows;                     // variant effects: the valid windows of a chunk's variants
  } set_bufs[2];
  int mut_route = 0;                               // route of the last crbm_mutagenesis* call: 1 fused kernel, 2 general path
  // annealed importance sampling (crbm_ais): the ladder, cA, the runs' log weights and letter codes between launches
  DevBuf<float> ais_betas, ais_base, ais_logw;
  DevBuf<uint8_t> ais_state;
  DevBuf<unsigned long long> hist;                 // score histogram (crbm_scan_histogram_codes): [K][S][nbins], then the valid windows; both streams add into it
  // record summaries (crbm_scan_records_codes): the call's accumulators -- sums [nrec][K], keys [nrec][K], counts [nrec][5] --
  // and the device copy of rec_start; both streams add into the accumulators
  DevBuf<unsigned long long> rec_acc;
  DevBuf<long long> rec_start;
  DevBuf<float> d_sums;
  int dataset_n[CRBM_DATASET_SLOTS] = {0, 0}, dataset_L[CRBM_DATASET_SLOTS] = {0, 0};
  int slot = 0;
  // sampler
  uint64_t seed = 0;
  uint32_t gibbs_step = 0, eval_step = 0, chain_offset = 0;
  int LWs = 0;                         // words per row of the last visible sample (d_vf)
  // the partitions of plain chain launches (plan.chain_parts > 1): `part`, at the end
  bool forked = false;                 // the partition streams hold work the main stream has not waited for yet
  bool main_idle_hint = false;         // the main stream was idle when the caller last looked (only its own event record is pending)
  // Partitions that start together stay in lockstep for hundreds of launches -- their gaps coincide and nothing is
  // gained (config #2: 20.8 us per step over the first 20 steps, 19.3 over 200, 17.7 once they have drifted apart).
  // So partition p starts p/P of a launch late: a one-wave delay kernel in front of its first launch after a fork.
  // The length of a launch is measured on the way (events around partition 0's first launch of the previous fork).
  double part_launch_us = 0.0;         // 0: not known yet (cost model below)
  bool cal_pending = false;
  int wall_khz = 100000;               // ticks of the GPU's wall clock per millisecond
  int variant = 1;                     // top-down variant of the Gibbs kernel in use (plan.chain[variant]; fixed per handle)
  int topdown_mode = 0;                // CRBM_TOPDOWN: 1 dense, anything else the set-bit walk (fixed per handle)
  DevBuf<uint32_t> d_nset;             // per wave of the last Gibbs launch: set bits of the final state
  int nset_slots = 0;
  uint32_t launches_since_read = 0;
  double activity = -1.0;              // fraction of hidden units on after the last launch that was read back
  int stats_rows = 0;
  bool fuse_stats = false;             // model half of the statistics inside the Gibbs kernel (Cfg::FUSE_STATS; CRBM_STATS=split: off)
  bool one_launch = true;              // ... and the data half in the same launch (CRBM_STATS=two: separate launch)
  SumsLayout sl;
  // data parallel
  ncclComm_t comm = nullptr;
  int nranks = 1, rank = 0;
  // ... without a collective launch: every rank's sums buffer mapped into every rank (crbm_ipc_*)
  DevBuf<float> ipc_buf;               // own: [2 parities][ipc_stride floats], then 2 flag words and a status word
  int ipc_stride = 0;                  // floats per parity (sums count rounded up to a 128-byte line)
  bool ipc_on = false;
  uint32_t ipc_step = 0;               // steps published so far (the flag value of the next one is ipc_step + 1)
  bool ipc_published = false;          // the column reduction of the running step has written and flagged the published buffer itself
  DevBuf<uint32_t> d_ticket;           // arrival counter of that launch (zero between launches)
  DevBuf<unsigned long long> d_probe;      // {wall ticks, shader cycles, scratch, scratch} summed over the launches of all crbm_time_gibbs calls
  unsigned long long probe_base[2] = {0, 0}, probe_last[2] = {0, 0};   // the sums before / after the last call
  bool probe_on = false;
  JitGeoKernels jg;             // the chain kernels compiled for the plan's launch shapes (LaunchPlan::geo_plain / geo_fused)
  long long geo_launches[2] = {0, 0};   // chain kernel launches in the run-time form, with the geometry compiled in (crbm_geometry_launches)
  DevBuf<unsigned long long> d_timeline;      // CRBM_GIBBS_TIMELINE: first / last tick of block 0 of every launch of a crbm_time_gibbs call
  int timeline_next = 0;
  int timeline_cap() const { return (int)(d_timeline.cap / 2); }      // launches the buffer has slots for
  unsigned long long ipc_timeout_ticks = 0;   // bound of an update launch's wait for its peers, in ticks of the GPU's wall clock
  // Statistics, h|v, free energies and site scans of a generic DNA model on the specialised kernels, a slab of motifs
  // at a time: the slab model (slab.K motifs; 0: none, slab_note says why) and one table image per slab, rebuilt when
  // the parameters have changed
  SlabModel slab;
  DevBuf<float> d_slab_tables;
  int slab_n = 0;
  bool slab_hgv = false;               // the chain's h|v takes the slabs too (slab a multiple of ten motifs, or one slab: sampler groups)
  uint64_t slab_tables_version = 0;
  float tsne_ms = 0.f;                 // device time of the iterations of the last crbm_tsne_descend call (HIP events)
  float null_ms = 0.f;                 // device time of the kernels of the last crbm_score_distribution call
  float compare_ms[4] = {0.f, 0.f, 0.f, 0.f};   // ... of the last crbm_motif_compare / _null call: all kernels; counts, null, placements
  float bg_ms = 0.f;                   // device time of the kernels of the last crbm_stream_kmer_counts / crbm_background_sample call
  std::string slab_note;               // why the slabs are off, if they are (crbm_launch_info prints nothing of it; a debugging aid)
  std::string err;
  PeerMaps<IPC_MAX_RANKS> ipc_peer;    // all ranks' buffers as this process sees them (own included: ipc_buf)
  Event ev0, ev1, ev_fork, ev_join, ev_parts_fork;
  Event ev_cal0, ev_cal1;              // around partition 0's first launch of a fork (part_launch_us)
  Stream stream;
  Stream stream2;                      // model phase of a training step runs beside the data phase
  Partition part[4];                   // the streams, threads and events of the partitions of plain chain launches
};

namespace {

int fail(crbm_handle* h, int code, const std::string& msg) {
  if (h) h->err = msg; else g_create_error = msg;
  return code;
}

#define HIPCHK(expr)                                                                         \
  do {                                                                                       \
    hipError_t e__ = (expr);                                                                 \
    if (e__ != hipSuccess)                                                                   \
      return fail(h, CRBM_ERR_HIP, std::string(#expr) + ": " + hipGetErrorString(e__));      \
  } while (0)

#define ARGCHK(cond, msg)                                 \
  do {                                                    \
    if (!(cond)) return fail(h, CRBM_ERR_INVALID, msg);   \
  } while (0)

RngView rng_view(const crbm_handle* h, uint32_t step, uint32_t seq_offset) {
  RngView r;
  r.seed_lo = (uint32_t)(h->seed & 0xffffffffu);
  r.seed_hi = (uint32_t)(h->seed >> 32);
  r.step = step;
  r.seq_offset = seq_offset;
  return r;
}

int tab_bytes(const ModelShape& ms) { return ms.TAB * 4; }

// words per packed row of L letters (2-bit letters for DNA, bytes for any other alphabet)
int lw(const crbm_handle* h, int L) { return letter_words_any(h->A, L); }

// (re)build the LDS table images after a parameter change
int ensure_tables(crbm_handle* h) {
  if (!h->tables_dirty || h->big()) return CRBM_OK;
  TablesArgs t;
  t.W = h->dW.p; t.b = h->db.p; t.c = h->dc.p; t.out = h->d_tables.p;
  const unsigned grid = (unsigned)std::max(1, std::min((h->ms().TABLES_ALL + 255) / 256, h->num_cu * 4));
  HIPCHK(jit_launch(h->jk.build_tables, t, grid, 1, 256, 0, h->stream));
  h->tables_dirty = false;
  h->main_idle_hint = false;           // the main stream holds work now: partitions that fork next must wait for it
  return CRBM_OK;
}

// the gather table of the solo grouping follows the parameters lazily: built when a plain chain launch finds it stale
int ensure_solo_table(crbm_handle* h) {
  if (h->plan.GS == h->plan.G || h->tf_solo_version == h->params_version) return CRBM_OK;
  TablesArgs t;
  t.W = h->dW.p; t.b = h->db.p; t.c = h->dc.p; t.out = h->d_tf_solo.p;
  const unsigned grid = (unsigned)std::max(1, std::min((h->plan.ms_solo.TAB + 255) / 256, h->num_cu * 4));
  HIPCHK(jit_launch(h->jk.build_gather_solo, t, grid, 1, 256, 0, h->stream));
  h->tf_solo_version = h->params_version;
  h->main_idle_hint = false;
  return CRBM_OK;
}

// ---- the "big" path (crbm_kernels.h: models beyond the LDS-resident kernels) --------------------------------------
BigModel big_model(const crbm_handle* h) {
  BigModel m;
  m.W = h->dW.p; m.b = h->db.p; m.c = h->dc.p;
  m.K = h->K; m.M = h->M; m.ds = h->ds; m.NW = h->NW; m.A = h->A;
  return m;
}

constexpr int SLAB_FALLBACK = -1000;     // slab_launch_stats / slab_launch_hgv: nothing launched, take the generic kernel
// free energies of a generic DNA model slab by slab (slab_launch_fe), unless CRBM_SLAB_FE=0 or the slab's tables exceed the LDS
bool slab_fe_on(const crbm_handle* h) { return h->slab.K && tab_bytes(h->slab.ms) <= 160 * 1024 && env_int("CRBM_SLAB_FE", 1) != 0; }
int slab_launch_hgv(crbm_handle* h, const uint32_t* d_letters, int n, int L, int mode, unsigned long long* ones, uint32_t* masks,
                    uint32_t kind, uint32_t step, uint32_t seq_offset, hipStream_t st);
int slab_launch_stats(crbm_handle* h, const uint32_t* d_letters, int n, int L, bool data_half, hipStream_t st, ReduceArgs* reduce);
int slab_launch_fe(crbm_handle* h, const uint32_t* rows, int n, int L, float* fe, float* fem, DevBuf<float>* scratch, hipStream_t st);

// h | v on packed rows: dense outputs (API), a count of sampled ones (evaluateData) or the masks of one strand (chain)
int big_launch_hgv(crbm_handle* h, const uint32_t* d_letters, int n, int L, int mode, float* act, float* prob, float* sample,
                   unsigned long long* ones, uint32_t* masks, uint32_t kind, uint32_t step, uint32_t seq_offset, hipStream_t st) {
  if (h->slab.K && h->slab_hgv && (masks || ones) && !act && !prob && !sample) {
    // the chain's h|v, or the count of a sample (evaluateData, the per-epoch evaluation: into scratch masks): the
    // specialised kernel, slab by slab
    uint32_t* out = masks;
    if (!out) {
      HIPCHK(h->masks_tmp.ensure((size_t)n * (L - h->M + 1) * h->NW));
      out = h->masks_tmp.p;
    }
    const int rc = slab_launch_hgv(h, d_letters, n, L, mode, ones, out, kind, step, seq_offset, st);
    if (rc != SLAB_FALLBACK) return rc;      // (a fallback comes before anything is launched)
  }
  BigHgvArgs a;
  a.m = big_model(h);
  a.letters = d_letters;
  a.n = n; a.L = L; a.Lh = L - h->M + 1; a.LW = lw(h, L);
  const int pool = h->ms().POOL;
  const BigHgvGeom g = big_hgv_geom(h->A, h->M, pool, n, L, a.LW, h->NW, h->num_cu);     // (crbm_plan.h)
  a.KS = g.KS;
  a.pool = pool;
  a.TS = g.TS;
  a.mode = mode;
  a.act = act; a.prob = prob; a.sample = sample; a.ones = ones; a.masks = masks;
  a.rng = rng_view(h, step, seq_offset);
  a.kind = kind;
  const size_t lds = g.lds;
  // (the filters of a slab take at most 96 KB: what exceeds the LDS is a row of letters beside them)
  ARGCHK(lds <= BIG_LDS_MAX, "sequence too long for the h|v kernel of a model of this size");
  const int ntiles = (n + a.TS - 1) / a.TS;
  a.split = g.split;
  const dim3 grid(std::max(1, std::min(ntiles, h->num_cu * 8)), a.split ? h->NW : 1);
  if (pool > 1) hipLaunchKernelGGL(big_hgv_pooled_kernel, grid, dim3(256), lds, st, a);
  else hipLaunchKernelGGL(big_hgv_kernel, grid, dim3(256), lds, st, a);
  HIPCHK(hipGetLastError());
  return CRBM_OK;
}

// `steps` Gibbs steps of the persistent chains: v | h from the masks, then h | v per strand into the masks
int big_launch_gibbs(crbm_handle* h, int steps, hipStream_t st) {
  BigVghArgs v;
  v.m = big_model(h);
  v.hm = h->d_hm.p; v.hmp = h->ds ? h->d_hmp.p : nullptr; v.vout = h->d_vf.p;
  v.nchains = h->B; v.Lf = h->Lf; v.Lv = h->Lv; v.LWs = h->LWs;
  const BigVghGeom g = big_vgh_geom(h->A, h->M, h->Lv);      // (crbm_plan.h)
  v.JS = g.JS;
  const size_t lds = g.lds;
  HIPCHK(hipMemsetAsync(h->d_ones.p, 0, sizeof(unsigned long long), st));
  for (int t = 0; t < steps; ++t) {
    v.rng = rng_view(h, h->gibbs_step + (uint32_t)t, h->chain_offset);
    if (h->A == 4) hipLaunchKernelGGL(big_vgh_kernel, dim3(std::max(1, std::min(h->B, h->num_cu * 8))), dim3(256), lds, st, v);
    else hipLaunchKernelGGL(big_vgh_any_kernel, dim3(std::max(1, std::min(h->B, h->num_cu * 8))), dim3(256), lds, st, v);
    HIPCHK(hipGetLastError());
    const bool last = t == steps - 1;      // the last step also counts the units that are on (activity monitor)
    for (int strand = 0; strand <= h->ds; ++strand) {
      const int rc = big_launch_hgv(h, h->d_vf.p, h->B, h->Lv, strand, nullptr, nullptr, nullptr, last ? h->d_ones.p : nullptr,
                                    strand ? h->d_hmp.p : h->d_hm.p, KIND_CHAIN_H, h->gibbs_step + (uint32_t)t, h->chain_offset, st);
      if (rc) return rc;
    }
  }
  h->gibbs_step += (uint32_t)steps;
  h->launches_since_read += 1;
  return CRBM_OK;
}

// the column reduction of `nrows` partial rows of `row` floats -- the statistic sums of n sequences -- into the data
// or the model half of d_sums
ReduceArgs reduce_args(const crbm_handle* h, bool data_half, float* partials, int nrows, int row, int n) {
  ReduceArgs r;
  r.partials = partials;
  r.nrows = nrows; r.row = row;
  r.K = h->K; r.KAM = h->KAM; r.ds = h->ds; r.want_sparsity = data_half ? 1 : 0;
  r.sums = h->d_sums.p + (data_half ? h->sl.data_off : h->sl.model_off);
  r.skip_begin = data_half ? row : h->sl.model_skip_begin;      // (sw, sb are not carried for the model half)
  r.skip_len = data_half ? 0 : h->sl.model_skip_len;
  r.n_value = (float)n;
  return r;
}

// raw statistic sums of (letters, n, L) into partial rows; the column reduction is handed back like launch_stats does
// (reduce->row == 0: nothing left to reduce -- the slabbed form below has written the sums itself)
int big_launch_stats(crbm_handle* h, const uint32_t* d_letters, int n, int L, bool data_half, hipStream_t st, ReduceArgs* reduce) {
  if (h->slab.K) {
    const int rc = slab_launch_stats(h, d_letters, n, L, data_half, st, reduce);
    if (rc != SLAB_FALLBACK) return rc;
  }
  DevBuf<float>& pbuf = data_half ? h->partials : h->partials2;
  const int K = h->K, M = h->M, KAM = h->KAM;
  BigStatsArgs a;
  a.m = big_model(h);
  a.letters = d_letters;
  a.n = n; a.L = L; a.Lh = L - M + 1; a.LW = lw(h, L);
  a.want_sparsity = data_half ? 1 : 0;
  a.pool = h->ms().POOL;
  const BigStatsGeom g = big_stats_geom(h->A, M, K, n, a.Lh, a.pool, h->num_cu);      // (crbm_plan.h)
  a.R = g.R;
  a.CH = g.CH;
  a.row = 3 * KAM + 3 * K + h->A;
  a.off_vh0 = 0; a.off_vh1 = KAM; a.off_h0 = 2 * KAM; a.off_h1 = 2 * KAM + K;
  a.off_sw = 2 * KAM + 2 * K; a.off_sb = 3 * KAM + 2 * K; a.off_v = 3 * KAM + 3 * K;
  HIPCHK(pbuf.ensure((size_t)a.R * a.row));
  a.partials = pbuf.p;
  ARGCHK(h->A * M <= BIG_ST * 256, "motif_length too large for the statistics kernel");
  const size_t lds = g.lds;
  ARGCHK(lds <= BIG_LDS_MAX, "motif_length too large for the statistics kernel");
  hipLaunchKernelGGL(big_stats_kernel, dim3(K, a.R), dim3(256), lds, st, a);
  HIPCHK(hipGetLastError());
  *reduce = reduce_args(h, data_half, pbuf.p, a.R, a.row, n);
  return CRBM_OK;
}

// free energies (hits = 0) or motif-hit summaries (hits = 1) of n packed rows
// (`fe_scratch`: the slab path's per-motif scratch, one per stream that may run this concurrently -- SweepSet::fe_scratch)
int big_launch_eval(crbm_handle* h, const uint32_t* rows, int n, int L, int hits, float* fe, float* fem, float* hmax, float* hmean,
                    unsigned long long* pos_fx, DevBuf<float>* fe_scratch, hipStream_t st) {
  if (!hits && slab_fe_on(h)) {       // free energies: the specialised kernel, slab by slab
    const int rc = slab_launch_fe(h, rows, n, L, fe, fem, fe_scratch, st);
    if (rc != SLAB_FALLBACK) return rc;
  }
  BigEvalArgs a;
  a.m = big_model(h);
  a.letters = rows;
  a.n = n; a.L = L; a.Lh = L - h->M + 1; a.LW = lw(h, L);
  a.fe = fe; a.fem = fem; a.hmax = hmax; a.hmean = hmean; a.pos_fx = pos_fx; a.hits = hits; a.pool = h->ms().POOL;
  const size_t lds = big_eval_lds(h->A, h->M, L);             // (crbm_plan.h)
  ARGCHK(lds <= BIG_LDS_MAX, "sequence too long for the evaluation kernel of a model of this size");
  hipLaunchKernelGGL(big_eval_kernel, dim3(std::max(1, std::min(n, h->num_cu * 8))), dim3(256), lds, st, a);
  HIPCHK(hipGetLastError());
  return CRBM_OK;
}

int grid_for(long items, int threads, int cap) {
  long g = (items + threads - 1) / threads;
  return (int)std::max<long>(1, std::min<long>(g, cap));
}

// sequences per tile so that a tile has ~target items and ts*len*mult < 2^20
int tile_seqs(int len, int target) { return std::max(1, std::min(target / std::max(1, len), (1 << 20) / std::max(1, len))); }

int check_flags(crbm_handle* h) {
  uint32_t flags = 0;
  HIPCHK(hipMemcpyAsync(&flags, h->d_flags.p, sizeof(flags), hipMemcpyDeviceToHost, h->stream));
  HIPCHK(hipStreamSynchronize(h->stream));
  if (flags) {
    HIPCHK(hipMemsetAsync(h->d_flags.p, 0, sizeof(uint32_t), h->stream));
    if (flags & 1u) return fail(h, CRBM_ERR_NOT_ONEHOT, "visible data is not exactly one-hot");
    return fail(h, CRBM_ERR_NOT_BINARY, "hidden state is not exactly 0/1");
  }
  return CRBM_OK;
}

int launch_hgv(crbm_handle* h, const uint32_t* d_letters, int n, int L, int mode, float* act, float* prob,
               float* sample, unsigned long long* ones, uint32_t kind, uint32_t step, uint32_t seq_offset) {
  if (h->big()) return big_launch_hgv(h, d_letters, n, L, mode, act, prob, sample, ones, nullptr, kind, step, seq_offset, h->stream);
  int rc = ensure_tables(h);
  if (rc) return rc;
  HgvArgs a;
  a.tables = h->d_tables.p;
  a.letters = d_letters;
  a.n = n; a.L = L; a.Lh = L - h->M + 1; a.LW = lw(h, L);
  a.TS = tile_seqs(a.Lh, 4096);
  a.divLh = make_fastdiv((uint32_t)a.Lh);
  a.mode = mode;
  a.act = act; a.prob = prob; a.sample = sample; a.ones = ones;
  a.rng = rng_view(h, step, seq_offset);
  a.kind = kind;
  const int ntiles = (n + a.TS - 1) / a.TS;
  const unsigned gx = (unsigned)std::max(1, std::min(ntiles, h->num_cu * 8));
  HIPCHK(jit_launch(h->jk.hgv, a, gx, 1, 256, (unsigned)tab_bytes(h->ms()), h->stream));
  return CRBM_OK;
}

StatsGeom stats_geom(const StatsMfmaLayout& st, float* partials, long ngroups, int lds_bytes);

// Arguments of a Gibbs launch of `steps` steps in geometry `g`.  model_reduce != null selects the STATS variant: the
// launch also leaves the model half of the gradient statistics as one partial row per block in
// h->partials2 (sized here: all this writes to the handle) and the column reduction is handed back
// through `model_reduce`.  The caller that launches sets h->nset_slots.
JitGeo jit_geo(const GeoSpec& s, int Lf) {
  JitGeo j;
  if (!s.on()) return j;
  j.S = s.gl.S; j.Lf = Lf; j.Lv = s.gl.Lv; j.Lrow = s.gl.Lrow; j.LWs = s.gl.LWs; j.nvb = s.gl.nvb; j.nhb = s.gl.nhb;
  j.threads = s.threads; j.nchains = s.nchains; j.grid = s.grid; j.aligned = s.aligned ? 1 : 0; j.group = s.group;
  return j;
}

// The kernel compiled for exactly this launch (GeoSpec), or null: then the launch takes the run-time form.  Launches
// without steps and launches with profiling aids (debug, timeline) are the run-time form's.
hipFunction_t geo_kernel(const GeoSpec& spec, hipFunction_t fn, const ChainGeom& g, const GibbsArgs& a) {
  if (!fn || a.steps < 1 || a.debug || a.timeline) return nullptr;
  return spec.serves(g.gl, g.threads, a.nblocks, a.nchains) && a.Lf == spec.gl.nhb ? fn : nullptr;
}

int prepare_gibbs(crbm_handle* h, const ChainGeom& g, int steps, ReduceArgs* model_reduce, GibbsArgs* out, unsigned* lds_out) {
  const GibbsLayout& gl = g.gl;
  GibbsArgs& a = *out;
  a.tables = h->d_tables.p;
  a.tables_tf = nullptr; a.off_ws = 0;
  a.hm = h->d_hm.p; a.hmp = h->ds ? h->d_hmp.p : nullptr; a.vout = h->d_vf.p;
  a.nchains = h->B; a.Lf = h->Lf; a.Lv = gl.Lv; a.S = gl.S;
  a.nvb = gl.nvb; a.nhb = gl.nhb; a.Lrow = gl.Lrow; a.LWs = gl.LWs;
  a.divVB = make_fastdiv((uint32_t)a.nvb);
  a.divHB = make_fastdiv((uint32_t)a.nhb);
  a.divRow = make_fastdiv((uint32_t)(a.Lrow * h->NW));
  a.divLfw = make_fastdiv((uint32_t)(a.Lf * h->NW));
  a.steps = steps;
  a.rng = rng_view(h, h->gibbs_step, h->chain_offset);
  a.ones = h->d_nset.p;
  a.clock = h->probe_on ? h->d_probe.p : nullptr;
  a.timeline = nullptr;
  a.debug = env_int("CRBM_GIBBS_DEBUG", 0);
  a.nblocks = g.grid;
  a.stats_off = 0;
  a.sg = StatsGeom();
  unsigned lds = (unsigned)gl.lds_bytes;
  if (model_reduce) {
    const StatsMfmaLayout st = stats_mfma_layout(h->ms(), 0, h->Lf, g.threads, 0, false);
    HIPCHK(h->partials2.ensure((size_t)g.grid * st.row));
    a.stats_off = (gl.lds_bytes / 4 + 3) & ~3;
    lds = (unsigned)std::max((a.stats_off + st.region_floats) * 4, st.combine_bytes);
    a.sg = stats_geom(st, h->partials2.p, (long)gl.S * st.GPC, (int)lds);
    *model_reduce = reduce_args(h, false, h->partials2.p, g.grid, st.row, h->B);
  }
  *lds_out = lds;
  return CRBM_OK;
}

void part_worker_main(PartWorker* w) {
  (void)hipSetDevice(w->device);
  std::unique_lock<std::mutex> lock(w->mu);
  for (;;) {
    // launches come in bursts: poll for a couple of milliseconds before going to sleep (a sleeping thread picks its
    // first job up 20-35 us late, and that is how late the partition's first launch of a burst then starts)
    const auto spin_until_t = std::chrono::steady_clock::now() + std::chrono::milliseconds(2);
    while (!w->stop && w->jobs.empty() && std::chrono::steady_clock::now() < spin_until_t) {
      lock.unlock();
      for (int i = 0; i < 64; ++i) __builtin_ia32_pause();
      lock.lock();
    }
    w->cv.wait(lock, [&] { return w->stop || !w->jobs.empty(); });
    if (w->jobs.empty()) return;       // stop, nothing left
    PartJob job = w->jobs.front();
    w->jobs.pop_front();
    w->busy = true;
    lock.unlock();
    hipError_t e = hipSuccess;
    if (job.delay_ticks > 0) {
      hipLaunchKernelGGL(delay_kernel, dim3(1), dim3(64), 0, w->stream, job.delay_ticks);
      e = hipGetLastError();
    }
    if (e == hipSuccess) e = jit_launch(job.fn, job.args, job.grid, 1, job.threads, job.lds, w->stream);
    lock.lock();
    if (e != hipSuccess && w->error == hipSuccess) w->error = e;
    w->busy = false;
    if (w->jobs.empty()) w->idle_cv.notify_all();
  }
}

// every launch handed to the partitions' threads has been enqueued on its stream
int drain_part_workers(crbm_handle* h) {
  for (int p = 1; p < h->plan.chain_parts; ++p) {
    PartWorker* w = h->part[p].worker.get();
    if (!w) continue;
    std::unique_lock<std::mutex> lock(w->mu);
    w->idle_cv.wait(lock, [&] { return w->jobs.empty() && !w->busy; });
    if (w->error != hipSuccess) {
      const hipError_t e = w->error;
      w->error = hipSuccess;
      return fail(h, CRBM_ERR_HIP, std::string("chain launch of partition ") + std::to_string(p) + ": " + hipGetErrorString(e));
    }
  }
  return CRBM_OK;
}

// every partition stream has finished what it was given as far as the main stream is concerned
int join_parts(crbm_handle* h) {
  if (!h->forked) return CRBM_OK;
  {
    const int rc = drain_part_workers(h);
    if (rc) return rc;
  }
  for (int p = 1; p < h->plan.chain_parts; ++p) {          // (partition 0 is the main stream itself)
    HIPCHK(hipEventRecord(h->part[p].done, h->part[p].stream));
    HIPCHK(hipStreamWaitEvent(h->stream, h->part[p].done, 0));
  }
  h->forked = false;
  return CRBM_OK;
}

// `steps` Gibbs steps of all chains as chain_parts launches on the partition streams (see LaunchPlan::chain_parts)
int launch_gibbs_parts(crbm_handle* h, int steps) {
  bool first_of_fork = false;
  double stagger_ticks = 0.0;      // first launch after a fork: partition p starts p times this late
  if (!h->forked) {     // the partitions start after whatever the main stream holds (parameter updates, state uploads)
    if (!h->main_idle_hint && hipStreamQuery(h->stream) != hipSuccess) {     // ... unless it is idle: nothing to wait for, no cross-stream dependency to resolve
      (void)hipGetLastError();
      HIPCHK(hipEventRecord(h->ev_parts_fork, h->stream));
      for (int p = 1; p < h->plan.chain_parts; ++p) HIPCHK(hipStreamWaitEvent(h->part[p].stream, h->ev_parts_fork, 0));
    }
    h->main_idle_hint = false;
    h->forked = true;
    first_of_fork = true;
    if (h->cal_pending && hipEventQuery(h->ev_cal1) == hipSuccess) {
      float ms = 0.f;
      if (hipEventElapsedTime(&ms, h->ev_cal0, h->ev_cal1) == hipSuccess && ms > 0.f) h->part_launch_us = 1e3 * ms;
      h->cal_pending = false;
    }
    (void)hipGetLastError();
    if (env_int("CRBM_PART_STAGGER", 1)) {
      // (before the first measurement: ~1 ns per hidden unit and Gibbs step, what configs #2 and #5 run at)
      const double est = h->part_launch_us > 0.0 ? h->part_launch_us
                                                 : 1e-3 * (double)h->B * h->Lf * h->K * (1 + h->ds) * steps;
      stagger_ticks = 0.9 * est / h->plan.chain_parts * (h->wall_khz / 1000.0);
    }
  }
  const LaunchPlan& plan = h->plan;
  GibbsArgs a;
  unsigned lds = 0;
  const int rc = prepare_gibbs(h, plan.part, steps, nullptr, &a, &lds);
  if (rc) return rc;
  const unsigned grid = (unsigned)plan.part.grid, threads = (unsigned)plan.part.threads;
  const size_t per = (size_t)h->Lf * h->NW;
  const int waves = (int)threads / 64;
  h->nset_slots = plan.chain_parts * (int)grid * waves;
  for (int p = 0; p < plan.chain_parts; ++p) {
    const int c0 = p * plan.part_chains, n = std::min(plan.part_chains, h->B - c0);
    if (n <= 0) break;
    GibbsArgs ap = a;
    ap.hm = a.hm + (size_t)c0 * per;
    if (ap.hmp) ap.hmp = a.hmp + (size_t)c0 * per;
    ap.vout = a.vout + (size_t)c0 * a.LWs;
    ap.nchains = n;
    ap.rng.seq_offset = a.rng.seq_offset + (uint32_t)c0;
    ap.ones = a.ones + (size_t)p * grid * waves;
    if (p > 0) ap.clock = nullptr;
    if (h->d_timeline.p && h->timeline_next < h->timeline_cap()) ap.timeline = h->d_timeline.p + 2 * (size_t)(h->timeline_next++);
    ap.nblocks = (int)grid;
    hipFunction_t fn = geo_kernel(plan.geo_plain, h->jg.gibbs_sparse, plan.part, ap);
    h->geo_launches[fn ? 1 : 0] += 1;
    if (!fn) fn = h->jk.gibbs_sparse;
    if (p > 0) {          // the partition's own thread enqueues it
      PartWorker* w = h->part[p].worker.get();
      {
        std::lock_guard<std::mutex> lock(w->mu);
        w->jobs.push_back(PartJob{fn, ap, grid, threads, lds, (unsigned long long)(stagger_ticks * p)});
      }
      w->cv.notify_one();
      continue;
    }
    const bool calibrate = first_of_fork && !h->cal_pending;
    if (calibrate) HIPCHK(hipEventRecord(h->ev_cal0, h->stream));
    HIPCHK(jit_launch(fn, ap, grid, 1, threads, lds, h->stream));
    if (calibrate) {
      HIPCHK(hipEventRecord(h->ev_cal1, h->stream));
      h->cal_pending = true;
    }
  }
  h->gibbs_step += (uint32_t)steps;
  h->launches_since_read += 1;
  return CRBM_OK;
}

// plain: a launch that only advances the chains, from the API (crbm_gibbs_steps*, crbm_time_gibbs) -- those may go out in
// partitions; the chain launch inside a training step is followed at once by kernels that wait for all of it and stays whole
int launch_gibbs(crbm_handle* h, int steps, hipStream_t s = nullptr, ReduceArgs* model_reduce = nullptr, bool plain = false) {
  if (!s) s = h->stream;
  if (h->big()) return big_launch_gibbs(h, steps, s);
  int rc = ensure_tables(h);
  if (rc) return rc;
  if (plain && !model_reduce && h->variant == 1 && h->plan.chain_parts > 1 && s == h->stream) return launch_gibbs_parts(h, steps);
  // (a launch with statistics is the fused variant's, in the model's own geometry)
  const ChainGeom& g = model_reduce ? h->plan.chain[h->variant] : plain_geom(h->plan, h->variant, false);
  GibbsArgs a;
  unsigned lds = 0;
  rc = prepare_gibbs(h, g, steps, model_reduce, &a, &lds);
  if (!model_reduce && h->variant == 1 && h->plan.GS != h->plan.G) {     // crbm_gibbs_sparse is compiled for the solo grouping
    a.tables_tf = h->d_tf_solo.p; a.off_ws = h->ms().OFF_WS;
    if (rc == CRBM_OK) rc = ensure_solo_table(h);
  }
  if (rc) return rc;
  h->nset_slots = g.grid * (g.threads / 64);
  if (plain && h->d_timeline.p && h->timeline_next < h->timeline_cap()) a.timeline = h->d_timeline.p + 2 * (size_t)(h->timeline_next++);
  hipFunction_t fn = model_reduce ? h->jk.gibbs_sparse_stats : (h->variant ? h->jk.gibbs_sparse : h->jk.gibbs);
  if (h->variant == 1) {
    hipFunction_t geo = model_reduce ? geo_kernel(h->plan.geo_fused, h->jg.gibbs_sparse_stats, g, a)
                                     : geo_kernel(h->plan.geo_plain, h->jg.gibbs_sparse, g, a);
    if (geo) fn = geo;
    h->geo_launches[geo ? 1 : 0] += 1;
  }
  HIPCHK(jit_launch(fn, a, (unsigned)g.grid, 1, (unsigned)g.threads, lds, s));
  h->gibbs_step += (uint32_t)steps;
  h->launches_since_read += 1;
  return CRBM_OK;
}

// Reads the activity monitor of the last Gibbs launch back (crbm_sync /
// crbm_gibbs_steps only: a blocking copy, kept out of every timed or training
// path).  It is a monitor, nothing else: the top-down variant is fixed per
// handle, so every rank of a data-parallel job -- and a 1-GPU run of the same
// chains -- rounds identically and draws identical samples.
int refresh_activity(crbm_handle* h) {
  if (h->launches_since_read == 0) return CRBM_OK;
  if (h->big()) {          // the last step's h|v launches counted into d_ones
    unsigned long long on = 0;
    HIPCHK(hipMemcpy(&on, h->d_ones.p, sizeof(on), hipMemcpyDeviceToHost));
    h->launches_since_read = 0;
    h->activity = (double)on / ((double)h->B * h->Lf * h->K * (1 + h->ds));
    return CRBM_OK;
  }
  std::vector<uint32_t> slots((size_t)h->nset_slots);
  HIPCHK(hipMemcpy(slots.data(), h->d_nset.p, slots.size() * sizeof(uint32_t), hipMemcpyDeviceToHost));
  unsigned long long last = 0;
  for (uint32_t v : slots) last += v;
  h->launches_since_read = 0;
  h->activity = (double)last / ((double)h->B * h->Lf * h->K * (1 + h->ds));
  return CRBM_OK;
}

StatsGeom stats_geom(const StatsMfmaLayout& st, float* partials, long ngroups, int lds_bytes) {
  StatsGeom g;
  g.GPC = st.GPC;
  g.lds_floats = lds_bytes / 4;
  g.off_slices = st.off_slices; g.slice = st.slice;
  g.off_win = st.off_win; g.off_gw = st.off_gw; g.off_pt = st.off_pt;
  g.divGPC = make_fastdiv((uint32_t)st.GPC, (uint64_t)std::max<long>(ngroups, 1));
  g.row = st.row; g.off_vh0 = st.off_vh[0]; g.off_vh1 = st.off_vh[1]; g.off_h0 = st.off_h[0]; g.off_h1 = st.off_h[1];
  g.off_sw = st.off_sw; g.off_sb = st.off_sb; g.off_v = st.off_v;
  g.partials = partials;
  return g;
}

// Arguments and launch geometry of the MFMA statistics kernel (stats_mfma_body) of model `ms` with table image `tables`
// for (letters, n, L): raw statistic sums -> partial rows of the data or the model half in `pbuf`, sized here.  `threads`
// 0: the kernel's own block size and the byte LUT; otherwise the geometry of a host kernel it rides in (nibble LUT).
// The column reduction of the rows is the caller's (reduce_args).
struct StatsLaunch { int lds = 0, grid = 0, block = 0, row = 0; };   // (row: floats per partial row, `grid` rows)
int prepare_stats(crbm_handle* h, const ModelShape& ms, const float* tables, DevBuf<float>& pbuf, const uint32_t* d_letters, int n, int L,
                  bool data_half, int threads, StatsMfmaArgs* out, StatsLaunch* launch) {
  const int want_sp = data_half ? 1 : 0;
  const int Lh = L - ms.M + 1;
  const int tabs = tab_bytes(ms);
  const bool own = threads <= 0;
  // CRBM_STATS_MAX_TILES is an experiment knob: it must come with CRBM_JIT_DEFINES=-DCRBM_STATS_MAX_TILES=<same>
  const StatsMfmaLayout st = stats_mfma_layout(ms, want_sp, Lh, own ? env_int("CRBM_STATS_THREADS", 0) : threads, tabs, own,
                                               env_int("CRBM_STATS_MAX_TILES", CRBM_STATS_MAX_TILES));
  StatsMfmaArgs& a = *out;
  a.tables = tables;
  a.letters = d_letters;
  a.n = n; a.L = L; a.Lh = Lh; a.LW = lw(h, L);
  const long ngroups = (long)n * st.GPC;
  const long nunits = (ngroups + 1) / 2;
  a.off_tab = st.region_floats;
  a.debug = env_int("CRBM_STATS_DEBUG", 0);
  ARGCHK(ngroups < (1L << 31), "batch too large for the statistics kernel");
  const int lds = std::max(st.region_floats * 4 + tabs, st.combine_bytes);
  ARGCHK(lds <= 160 * 1024, "model too large for the statistics kernel");
  const int wpr = (st.threads / 64) / st.NR;                  // waves per role = units a block works on at a time
  // Grid: a persistent set of blocks, every wave with the same number of units (a ragged last round costs
  // a whole unit time: at config #2 768 blocks of 8 units per wave take 73 us per training step, 832 blocks
  // 78).  Stand-alone: as many blocks as are resident at once; riding in the training launch: three per CU
  // beside the four chain blocks (measured optimum, fewer partial rows to combine and reduce).
  const int per_cu = own ? std::max(1, std::min(2048 / st.threads, (160 * 1024) / std::max(1, lds))) : 3;
  // (riding beside the chain blocks: three 256-thread blocks per CU, the same number of waves with larger blocks)
  const long cap = h->stats_rows > 0 ? h->stats_rows : own ? (long)h->num_cu * per_cu : std::max<long>(1, (long)h->num_cu * 3 * 256 / st.threads);
  const long upw = std::max<long>(1, (nunits + cap * wpr - 1) / (cap * wpr));        // units per wave
  const int gx = (int)std::max<long>(1, (nunits + upw * wpr - 1) / (upw * wpr));
  HIPCHK(pbuf.ensure((size_t)gx * st.row));
  a.nblocks = gx;
  a.sg = stats_geom(st, pbuf.p, ngroups, lds);
  launch->lds = lds; launch->grid = gx; launch->block = st.threads; launch->row = st.row;
  return CRBM_OK;
}

// The statistics of a generic DNA model (motif_length <= 64) on the matrix cores.  VH[k], H[k] and the sparsity sums of motif
// k depend on that motif's filter alone, so the model is a row of independent sub-models of `slab.K` motifs: the
// specialised statistics kernel of that sub-model (stats_mfma_body: gather table in LDS, P split into f16 halves,
// v_mfma_f32_16x16x32_f16) runs once per slab on the slab's own table image -- W and b of a slab are contiguous pieces of
// the model's (K,4,M) and (K) arrays -- and slab_reduce_kernel adds the slab's partial rows into its columns of d_sums.
// The last slab of a model whose K is not a multiple of the slab is moved back to end at K: the motifs it shares with its
// neighbour get the same sums twice (an accumulator's value does not depend on the column it sits in).
// first motif of slab i: slabs of Ks motifs side by side; the last one of a model whose K is no multiple of Ks starts on the
// first multiple of ten at or behind K - Ks (sampler groups are ten units wide: every unit keeps its group and field), so it
// overlaps its neighbour and may reach up to nine motifs past K -- into the zero padding of W and b (crbm_create)
int slab_origin(const crbm_handle* h, int i) {
  const int Ks = h->slab.K;
  if ((i + 1) * Ks <= h->K) return i * Ks;
  return h->slab_hgv ? ((h->K - Ks + 9) / 10) * 10 : h->K - Ks;
}

SlabPlan slab_plan(const crbm_handle* h) {
  SlabPlan p;
  p.Ks = h->slab.K; p.K = h->K; p.last_k0 = slab_origin(h, h->slab_n - 1);
  return p;
}

// one launch builds the table images of all slabs (blockIdx.y = slab: slab_tables_body)
int slab_ensure_tables(crbm_handle* h, hipStream_t st) {
  const SlabModel* s = &h->slab;
  if (h->slab_tables_version == h->params_version) return CRBM_OK;
  SlabTablesArgs a;
  a.t.W = h->dW.p; a.t.b = h->db.p; a.t.c = h->dc.p; a.t.out = h->d_slab_tables.p;
  a.plan = slab_plan(h);
  a.stride = s->ms.TABLES_ALL;
  const unsigned grid = (unsigned)std::max(1, std::min((s->ms.TABLES_ALL + 255) / 256, h->num_cu * 4));
  HIPCHK(jit_launch(s->jk.slab_tables, a, grid, (unsigned)h->slab_n, 256, 0, st));
  h->slab_tables_version = h->params_version;
  return CRBM_OK;
}

// h | v of a chain of a generic DNA model: the specialised h|v pass of the slab model (hgv_masks_body: gather table in LDS,
// all of the slab's units of a position in one lane, sign-word sampling), all slabs in one launch (blockIdx.y = slab); every
// unit draws from the counter it has in the whole model (HgvMasksArgs::group0) and lands in its bit of the model's mask rows
// (HgvMasksArgs::masks, atomicOr: neighbouring slabs share words).
int slab_launch_hgv(crbm_handle* h, const uint32_t* d_letters, int n, int L, int mode, unsigned long long* ones, uint32_t* masks,
                    uint32_t kind, uint32_t step, uint32_t seq_offset, hipStream_t st) {
  const SlabModel* s = &h->slab;
  const int Lh = L - h->M + 1;
  if (tab_bytes(s->ms) > 160 * 1024) return SLAB_FALLBACK;
  int rc = slab_ensure_tables(h, st);
  if (rc) return rc;
  HIPCHK(hipMemsetAsync(masks, 0, (size_t)n * Lh * h->NW * sizeof(uint32_t), st));
  SlabHgvArgs sa;
  HgvArgs& a = sa.m.g;
  a.tables = h->d_slab_tables.p;
  a.letters = d_letters;
  a.n = n; a.L = L; a.Lh = Lh; a.LW = lw(h, L);
  // rows per tile: ~4096 positions, fewer for small batches (enough blocks, with the slabs, to cover the chip a few times over)
  a.TS = std::max(1, std::min(tile_seqs(a.Lh, 4096), (n * h->slab_n + 4 * h->num_cu - 1) / (4 * h->num_cu)));
  a.divLh = make_fastdiv((uint32_t)a.Lh);
  a.mode = mode;
  a.act = nullptr; a.prob = nullptr; a.sample = nullptr; a.ones = ones;
  a.rng = rng_view(h, step, seq_offset);
  a.kind = kind;
  sa.m.masks = masks; sa.m.NWfull = h->NW; sa.m.Kfull = h->K;
  sa.m.k0 = 0; sa.m.kskip = 0; sa.m.group0 = 0;          // per slab: slab_hgv_body
  sa.plan = slab_plan(h);
  sa.table_stride = s->ms.TABLES_ALL;
  const int ntiles = (n + a.TS - 1) / a.TS;
  const unsigned gx = (unsigned)std::max(1, std::min(ntiles, h->num_cu * 8));
  HIPCHK(jit_launch(s->jk.slab_hgv, sa, gx, (unsigned)h->slab_n, 256, (unsigned)tab_bytes(s->ms), st));
  return CRBM_OK;
}

// The statistics of a generic DNA model: the specialised statistics kernel of the slab model, all slabs in one launch
// (blockIdx.y = slab: its table image, its partial rows), then slab_reduce_kernel -- one launch too -- reduces every slab's
// partial rows into the slab's columns of the model's sums.
int slab_launch_stats(crbm_handle* h, const uint32_t* d_letters, int n, int L, bool data_half, hipStream_t st, ReduceArgs* reduce) {
  SlabModel* s = &h->slab;
  const int Ks = s->K, M = h->M;
  int rc = slab_ensure_tables(h, st);
  if (rc) return rc;
  DevBuf<float>& pbuf = data_half ? s->partials : s->partials2;
  SlabStatsArgs sa;
  StatsLaunch l;
  rc = prepare_stats(h, s->ms, h->d_slab_tables.p, pbuf, d_letters, n, L, data_half, 0, &sa.a, &l);
  if (rc == CRBM_ERR_INVALID) {      // (a data set whose rows the slab kernel's LDS does not take)
    h->err.clear();
    return SLAB_FALLBACK;
  }
  if (rc) return fail(h, rc, "slabbed statistics: " + h->err);
  const size_t per_slab = (size_t)l.grid * l.row;
  HIPCHK(pbuf.ensure(per_slab * h->slab_n));
  sa.a.sg.partials = pbuf.p;
  sa.table_stride = s->ms.TABLES_ALL; sa.pad_ = 0;
  sa.partial_stride = (long long)per_slab;
  if (jit_launch(data_half ? s->jk.slab_stats_data : s->jk.slab_stats_model, sa, (unsigned)l.grid, (unsigned)h->slab_n, (unsigned)l.block, (unsigned)l.lds, st) != hipSuccess)
    return fail(h, CRBM_ERR_HIP, "launch of the slab statistics kernel failed");
  SlabReduceArgs ra;
  ra.partials = pbuf.p;
  ra.sums = h->d_sums.p + (data_half ? h->sl.data_off : h->sl.model_off);
  ra.nrows = l.grid; ra.row = l.row;
  ra.Ks = Ks; ra.k0 = slab_origin(h, h->slab_n - 1); ra.K = h->K; ra.M4 = 4 * M;
  ra.partial_stride = (long long)per_slab;
  ra.ds = h->ds; ra.want_sparsity = data_half ? 1 : 0;
  const int full_row = 3 * h->KAM + 3 * h->K + 4;
  ra.skip_begin = data_half ? full_row : h->sl.model_skip_begin;
  ra.skip_len = data_half ? 0 : h->sl.model_skip_len;
  ra.n_value = (float)n;
  hipLaunchKernelGGL(slab_reduce_kernel, dim3((ra.row + 31) / 32, h->slab_n), dim3(1024), 0, st, ra);
  HIPCHK(hipGetLastError());
  *reduce = ReduceArgs();
  reduce->nrows = 0; reduce->row = 0;     // nothing left for the caller's column reduction
  return CRBM_OK;
}

// Free energies of a generic DNA model (freeEnergy, evaluateData, the per-epoch evaluation of fit(): convRBM.py:657-697, :517-522):
// the slab model's free-energy kernel leaves every slab's per-motif terms in a scratch (one launch, blockIdx.y = slab),
// slab_fe_combine_kernel adds them up per sequence.  The scratch belongs to the caller's stream (SlabModel::fe_scratch: [0]
// for the main stream, [1] for the second stream of a host-input sweep): the two streams' slabs run at the same time.
int slab_launch_fe(crbm_handle* h, const uint32_t* rows, int n, int L, float* fe, float* fem, DevBuf<float>* scratch, hipStream_t st) {
  const SlabModel* s = &h->slab;
  if (tab_bytes(s->ms) > 160 * 1024) return SLAB_FALLBACK;
  int rc = slab_ensure_tables(h, st);
  if (rc) return rc;
  const size_t per_slab = (size_t)n * s->K;
  HIPCHK(scratch->ensure(per_slab * h->slab_n));
  SlabFeArgs sa;
  sa.a.tables = h->d_slab_tables.p;
  sa.a.letters = rows;
  sa.a.n = n; sa.a.L = L; sa.a.Lh = L - h->M + 1; sa.a.LW = lw(h, L);
  sa.a.fe = nullptr; sa.a.fem = scratch->p;
  sa.table_stride = s->ms.TABLES_ALL; sa.pad_ = 0;
  sa.fem_stride = (long long)per_slab;
  const unsigned gx = (unsigned)std::max(1, std::min((n + 3) / 4, h->num_cu * 8));
  HIPCHK(jit_launch(s->jk.slab_fe, sa, gx, (unsigned)h->slab_n, 256, (unsigned)tab_bytes(s->ms), st));
  SlabFeCombineArgs ca;
  ca.scratch = scratch->p;
  ca.c_log2e = h->d_slab_tables.p + s->ms.OFF_C;
  ca.letters = rows;
  ca.n = n; ca.L = L; ca.LW = lw(h, L);
  ca.Ks = s->K; ca.K = h->K; ca.last_k0 = slab_origin(h, h->slab_n - 1); ca.nslab = h->slab_n;
  ca.fe = fe; ca.fem = fem;
  hipLaunchKernelGGL(slab_fe_combine_kernel, dim3(gx), dim3(256), 0, st, ca);
  HIPCHK(hipGetLastError());
  return CRBM_OK;
}

// The slab model of a generic handle (crbm_create), as the plan chose it; leaves h->slab.K zero, with the reason in
// h->slab_note, when the model is not one for slabs or the slab's kernels or tables are not to be had.
void slab_setup(crbm_handle* h) {
  const LaunchPlan& plan = h->plan;
  if (!plan.big) return;
  if (!plan.slab_K) { h->slab_note = plan.slab_note; return; }
  const int n = (h->K + plan.slab_K - 1) / plan.slab_K;
  std::string err;
  if (jit_load(plan.slab_K, h->M, h->ds, plan.slab_G, plan.slab_G, plan.slab_ms.POOL, 0, 256, &h->slab.jk, &err, true) != 0) {
    h->slab_note = "kernel specialisation of the slab failed: " + err;
    return;
  }
  if (h->d_slab_tables.alloc((size_t)n * plan.slab_ms.TABLES_ALL) != hipSuccess) {
    (void)hipGetLastError();
    h->slab = SlabModel();
    h->slab_note = "no memory for the slab tables";
    return;
  }
  h->slab.K = plan.slab_K; h->slab.ms = plan.slab_ms;
  h->slab_n = n;
  h->slab_hgv = (n == 1 || plan.slab_K % 10 == 0) && env_int("CRBM_SLAB_HGV", 1) != 0;
}

// stand-alone launch; the column reduction is handed back to the caller (`defer`, to pair it with the
// other half) or launched here
int launch_stats(crbm_handle* h, const uint32_t* d_letters, int n, int L, bool data_half, hipStream_t s = nullptr,
                 ReduceArgs* defer = nullptr) {
  if (!s) s = h->stream;
  int rc = ensure_tables(h);
  if (rc) return rc;
  ReduceArgs r;
  if (h->big()) rc = big_launch_stats(h, d_letters, n, L, data_half, s, &r);
  else {
    StatsMfmaArgs a;
    StatsLaunch l;
    DevBuf<float>& pbuf = data_half ? h->partials : h->partials2;
    rc = prepare_stats(h, h->ms(), h->d_tables.p, pbuf, d_letters, n, L, data_half, 0, &a, &l);
    if (rc) return rc;
    r = reduce_args(h, data_half, pbuf.p, l.grid, l.row, n);
    rc = jit_launch(data_half ? h->jk.stats_mfma_data : h->jk.stats_mfma_model, a, (unsigned)l.grid, 1, (unsigned)l.block, (unsigned)l.lds, s) == hipSuccess
             ? CRBM_OK : fail(h, CRBM_ERR_HIP, "launch of the statistics kernel failed");
  }
  if (rc) return rc;
  if (defer) { *defer = r; return CRBM_OK; }
  if (r.row == 0) return CRBM_OK;        // slabbed statistics: the sums are written
  hipLaunchKernelGGL(reduce_partials_kernel, dim3((r.row + 31) / 32), dim3(1024), 0, s, r);
  HIPCHK(hipGetLastError());
  return CRBM_OK;
}

void fill_update_args(crbm_handle* h, int L_data, UpdateTablesArgs& a) {
  UpdateArgs& u = a.u;
  u.sums = h->d_sums.p;
  u.W = h->dW.p; u.b = h->db.p; u.c = h->dc.p; u.vW = h->dvW.p; u.vb = h->dvb.p; u.vc = h->dvc.p;
  u.oW = h->dW2.p; u.ob = h->db2.p; u.oc = h->dc2.p; u.ovW = h->dvW2.p; u.ovb = h->dvb2.p; u.ovc = h->dvc2.p;
  u.K = h->K; u.M = h->M; u.ds = h->ds;
  u.L_data = L_data; u.Lf = h->Lf;
  u.data_off = h->sl.data_off; u.n_d = h->sl.n_d; u.model_off = h->sl.model_off; u.n_m = h->sl.n_m;
  u.lr = h->cfg.learning_rate; u.momentum = h->cfg.momentum; u.rho = h->cfg.rho; u.lambda_rate = h->cfg.lambda_rate;
  u.A = h->A;
  a.tables = h->d_tables.p;
}

// the update wrote the other set of buffers: it is the current one from now on
void swap_param_sets(crbm_handle* h) {
  h->dW.swap(h->dW2); h->db.swap(h->db2); h->dc.swap(h->dc2);
  h->dvW.swap(h->dvW2); h->dvb.swap(h->dvb2); h->dvc.swap(h->dvc2);
  h->tables_dirty = false;
  h->params_version += 1;
}

// update + rebuild of the table images in one launch (update_tables_body)
int launch_update(crbm_handle* h, int L_data) {
  UpdateTablesArgs a;
  fill_update_args(h, L_data, a);
  if (h->big()) {        // element-wise and in place: no table images to rebuild, no second buffer set
    UpdateArgs& u = a.u;
    u.oW = h->dW.p; u.ob = h->db.p; u.oc = h->dc.p; u.ovW = h->dvW.p; u.ovb = h->dvb.p; u.ovc = h->dvc.p;
    hipLaunchKernelGGL(big_update_kernel, dim3(grid_for((long)h->KAM + h->K + h->A, 256, h->num_cu * 4)), dim3(256), 0, h->stream, u);
    HIPCHK(hipGetLastError());
    h->params_version += 1;
    return CRBM_OK;
  }
  const unsigned grid = (unsigned)std::max(1, std::min((h->ms().TABLES_ALL + 4095) / 4096, 32));
  HIPCHK(jit_launch(h->jk.update_tables, a, grid, 1, UPDATE_THREADS, (unsigned)((h->KAM + h->K + 4) * 4), h->stream));
  swap_param_sets(h);
  return CRBM_OK;
}

size_t ipc_bytes(const crbm_handle* h);
float* ipc_slot_of(void* base, const crbm_handle* h, int parity, int source);
uint32_t* ipc_flag_of(void* base, const crbm_handle* h, int parity, int source);

// the column reductions of both halves in one launch; with the mapped-buffer all-reduce on, straight into this
// rank's published buffer, flag included (reduce_publish_pair_kernel)
int launch_reduce_pair(crbm_handle* h, ReducePair pair, bool publish) {
  if (pair.half[0].row == 0 || pair.half[1].row == 0) {      // slabbed statistics have written their sums themselves (slab_launch_stats)
    for (auto& half : pair.half)
      if (half.row > 0) {
        hipLaunchKernelGGL(reduce_partials_kernel, dim3((half.row + 31) / 32), dim3(1024), 0, h->stream, half);
        HIPCHK(hipGetLastError());
      }
    return CRBM_OK;
  }
  const dim3 grid((pair.half[0].row + 31) / 32, 2);
  if (publish && h->ipc_on) {
    // this rank's slot of the step's parity in every rank's buffer, the own one as the base the others are offsets of
    const int parity = (int)(h->ipc_step & 1u);
    float* base = ipc_slot_of(h->ipc_buf.p, h, parity, h->rank);
    for (auto& half : pair.half) half.sums = base + (half.sums - h->d_sums.p);
    PublishTail t;
    t.ticket = h->d_ticket.p; t.value = h->ipc_step + 1u;
    t.push.n = h->nranks;
    for (int r = 0; r < IPC_MAX_RANKS; ++r) {
      void* peer = r < h->nranks ? h->ipc_peer[r] : h->ipc_buf.p;
      t.push.delta[r] = (long long)(reinterpret_cast<char*>(ipc_slot_of(peer, h, parity, h->rank)) - reinterpret_cast<char*>(base));
      t.flag[r] = ipc_flag_of(peer, h, parity, h->rank);
    }
    hipLaunchKernelGGL(reduce_publish_pair_kernel, grid, dim3(1024), 0, h->stream, pair, t);
    h->ipc_published = true;
  } else {
    hipLaunchKernelGGL(reduce_partials_pair_kernel, grid, dim3(1024), 0, h->stream, pair);
  }
  HIPCHK(hipGetLastError());
  return CRBM_OK;
}

// data statistics + k Gibbs steps + model statistics -> d_sums (local)
// publish: the caller runs the mapped-buffer all-reduce next (train_core), so the sums may go straight to the
// published buffer; crbm_train_local wants them in d_sums
int train_local_dev(crbm_handle* h, const uint32_t* d_letters, int n, int L, bool publish = false) {
  int rc = ensure_tables(h);
  if (rc) return rc;
  if (h->slab.K) {      // the slab tables too, on the main stream: both halves read them (CRBM_OVERLAP: from two streams)
    rc = slab_ensure_tables(h, h->stream);
    if (rc) return rc;
  }
  hipStream_t sm = h->overlap ? h->stream2 : h->stream;
  if (h->overlap) {
    HIPCHK(hipEventRecord(h->ev_fork, h->stream));          // tables ready, earlier work on the chains done
    HIPCHK(hipStreamWaitEvent(h->stream2, h->ev_fork, 0));
  }
  // single stream: the two column reductions share one launch
  ReducePair pair;
  const bool paired = !h->overlap && n > 0;
  if (h->fuse_stats && paired && h->one_launch) {
    // the whole local phase in one launch (train_local_body): chain + model half in the first
    // g.grid blocks, data half in the blocks behind them
    const ChainGeom& g = h->plan.chain[h->variant];
    TrainLocalArgs t;
    unsigned glds = 0;
    rc = prepare_gibbs(h, g, h->cfg.cd_k, &pair.half[1], &t.g, &glds);
    if (rc) return rc;
    StatsLaunch d;
    rc = prepare_stats(h, h->ms(), h->d_tables.p, h->partials, d_letters, n, L, true, g.threads, &t.d, &d);
    if (rc) return rc;
    pair.half[0] = reduce_args(h, true, h->partials.p, d.grid, d.row, n);
    const unsigned lds = std::max(glds, (unsigned)d.lds);
    t.g.sg.lds_floats = (int)(lds / 4);
    t.d.sg.lds_floats = (int)(lds / 4);
    h->nset_slots = g.grid * (g.threads / 64);
    hipFunction_t fn = h->variant == 1 ? geo_kernel(h->plan.geo_fused, h->jg.train_local, g, t.g) : nullptr;
    h->geo_launches[fn ? 1 : 0] += 1;
    HIPCHK(jit_launch(fn ? fn : h->jk.train_local, t, (unsigned)(g.grid + d.grid), 1, (unsigned)g.threads, lds, h->stream));
    h->gibbs_step += (uint32_t)h->cfg.cd_k;
    h->launches_since_read += 1;
    return launch_reduce_pair(h, pair, publish);
  }
  if (h->fuse_stats) {
    // the Gibbs launch itself leaves the model half of the statistics (last-step probabilities
    // and visible sample never leave the chip)
    ReduceArgs mr;
    rc = launch_gibbs(h, h->cfg.cd_k, sm, &mr);
    if (rc) return rc;
    if (paired) pair.half[1] = mr;
    else {
      hipLaunchKernelGGL(reduce_partials_kernel, dim3((mr.row + 31) / 32), dim3(1024), 0, sm, mr);
      HIPCHK(hipGetLastError());
    }
  } else {
    rc = launch_gibbs(h, h->cfg.cd_k, sm);
    if (rc) return rc;
    rc = join_parts(h);      // (a partitioned chain launch: the statistics read what all partitions leave)
    if (rc) return rc;
    rc = launch_stats(h, h->d_vf.p, h->B, h->Lv, false, sm, paired ? &pair.half[1] : nullptr);
    if (rc) return rc;
  }
  if (h->overlap) HIPCHK(hipEventRecord(h->ev_join, h->stream2));
  if (n > 0) {
    rc = launch_stats(h, d_letters, n, L, true, nullptr, paired ? &pair.half[0] : nullptr);
    if (rc) return rc;
    if (paired) {
      rc = launch_reduce_pair(h, pair, publish);
      if (rc) return rc;
    }
  } else {   // a rank may own no rows of a short last mini-batch: contribute zeros
    HIPCHK(hipMemsetAsync(h->d_sums.p + h->sl.data_off, 0, (size_t)(h->sl.n_d + 1 - h->sl.data_off) * sizeof(float), h->stream));
  }
  if (h->overlap) HIPCHK(hipStreamWaitEvent(h->stream, h->ev_join, 0));
  return CRBM_OK;
}

// ---- IPC all-reduce (update_tables_ipc_body) -------------------------------------------------
// A rank's buffer: [2 parities][8 source ranks][ipc_stride floats] of sums, then [2][8] flag words on 64-byte lines
// of their own, then the status word
size_t ipc_bytes(const crbm_handle* h) { return ((size_t)2 * IPC_MAX_RANKS * h->ipc_stride + (2 * IPC_MAX_RANKS + 1) * 16) * sizeof(float); }
float* ipc_slot_of(void* base, const crbm_handle* h, int parity, int source) {
  return static_cast<float*>(base) + ((size_t)parity * IPC_MAX_RANKS + source) * h->ipc_stride;
}
uint32_t* ipc_flag_of(void* base, const crbm_handle* h, int parity, int source) {
  return reinterpret_cast<uint32_t*>(static_cast<float*>(base) + (size_t)2 * IPC_MAX_RANKS * h->ipc_stride) + 16 * (parity * IPC_MAX_RANKS + source);
}
uint32_t* ipc_status_of(void* base, const crbm_handle* h) {
  return reinterpret_cast<uint32_t*>(static_cast<float*>(base) + (size_t)2 * IPC_MAX_RANKS * h->ipc_stride) + 16 * 2 * IPC_MAX_RANKS;
}

int ipc_allocate(crbm_handle* h) {
  if (h->ipc_buf.p) return CRBM_OK;
  h->ipc_stride = (h->sl.count + 31) & ~31;
  // fine-grained device memory: coherent between agents, so a peer's system-scope stores are what this GPU's
  // system-scope loads see.  Plain (coarse-grained) device memory may keep stale lines of the rank's own buffer in
  // L2 after a peer's write over xGMI: refused unless CRBM_IPC_COARSE_OK=1 asks for it (one-GPU experiments).
  DevBuf<float> buf;                   // the handle's once it is zeroed
  const size_t floats = ipc_bytes(h) / sizeof(float);
  const hipError_t fe = buf.alloc(floats, true);
  if (fe != hipSuccess) {
    (void)hipGetLastError();
    if (env_int("CRBM_IPC_COARSE_OK", 0) == 0)
      return fail(h, CRBM_ERR_HIP, std::string("hipExtMallocWithFlags(hipDeviceMallocFinegrained) for the mapped sums buffer: ") + hipGetErrorString(fe));
    HIPCHK(buf.alloc(floats));
  }
  HIPCHK(hipMemset(buf.p, 0, ipc_bytes(h)));
  h->ipc_buf = std::move(buf);
  return CRBM_OK;
}

// this rank's sums of the step -> its slot in every rank's buffer + flags; then the update that sums the slots of its own buffer
int launch_ipc_allreduce_update(crbm_handle* h, int L_data) {
  const int parity = (int)(h->ipc_step & 1u);
  const uint32_t value = h->ipc_step + 1u;
  if (!h->ipc_published) {
    // the sums of this step were formed in d_sums (separate reductions of the two halves, or a rank without data
    // rows): push them and raise the flags in a launch of its own
    PublishArgs pa;
    pa.src = h->d_sums.p; pa.value = value; pa.count = h->sl.count; pa.n = h->nranks;
    for (int r = 0; r < IPC_MAX_RANKS; ++r) {
      void* peer = r < h->nranks ? h->ipc_peer[r] : h->ipc_buf.p;
      pa.dst[r] = ipc_slot_of(peer, h, parity, h->rank);
      pa.flag[r] = ipc_flag_of(peer, h, parity, h->rank);
    }
    hipLaunchKernelGGL(publish_sums_kernel, dim3(1), dim3(1024), 0, h->stream, pa);
    HIPCHK(hipGetLastError());
  }
  h->ipc_published = false;
  UpdateIpcArgs a;
  fill_update_args(h, L_data, a.ut);
  for (int r = 0; r < IPC_MAX_RANKS; ++r) {            // everything the update reads is in this rank's own buffer
    const int src = r < h->nranks ? r : 0;
    a.ipc.sums[r] = ipc_slot_of(h->ipc_buf.p, h, parity, src);
    a.ipc.flags[r] = ipc_flag_of(h->ipc_buf.p, h, parity, src);
  }
  a.ipc.status = ipc_status_of(h->ipc_buf.p, h);
  a.ipc.expect = value; a.ipc.nranks = h->nranks; a.ipc.count = h->sl.count;
  a.ipc.timeout_ticks = h->ipc_timeout_ticks;
  const unsigned grid = (unsigned)std::max(1, std::min((h->ms().TABLES_ALL + 4095) / 4096, 32));
  // the new parameters and one word (update_tables_ipc_body): the published sums are read where they lie, not staged
  const unsigned lds = (unsigned)((h->KAM + h->K + 4 + 4) * 4);
  HIPCHK(jit_launch(h->jk.update_tables_ipc, a, grid, 1, UPDATE_THREADS, lds, h->stream));
  swap_param_sets(h);
  h->ipc_step += 1;
  return CRBM_OK;
}

int train_core(crbm_handle* h, const uint32_t* d_letters, int n, int L) {
  int rc = train_local_dev(h, d_letters, n, L, true);
  if (rc) return rc;
  if (h->ipc_on) return launch_ipc_allreduce_update(h, L);
  if (h->comm) {
    ncclResult_t r = g_rccl.AllReduce(h->d_sums.p, h->d_sums.p, (size_t)h->sl.count, ncclFloat, ncclSum, h->comm, h->stream);
    if (r != ncclSuccess) return fail(h, CRBM_ERR_RCCL, std::string("ncclAllReduce: ") + g_rccl.GetErrorString(r));
  }
  return launch_update(h, L);
}

// The status word of the mapped-buffer all-reduce, read at a point where the stream is idle anyway: a wait for a
// peer that ran out (update_tables_ipc_body) is an error of every training entry point and of crbm_sync from then on.
int ipc_check(crbm_handle* h) {
  if (!h->ipc_on || !h->ipc_buf.p) return CRBM_OK;
  uint32_t st = 0;
  HIPCHK(hipMemcpy(&st, ipc_status_of(h->ipc_buf.p, h), sizeof(st), hipMemcpyDeviceToHost));
  if (st != 0)
    return fail(h, CRBM_ERR_IPC_TIMEOUT, "mapped-buffer all-reduce: waited " + std::to_string(env_int("CRBM_IPC_TIMEOUT_MS", 30000)) +
                " ms in vain for a peer's statistic sums (a rank died or fell out of step); no update has been applied since, "
                "the parameters are those of the last complete step");
  return CRBM_OK;
}

int check_data_shape(crbm_handle* h, int n, int L) {
  ARGCHK(n >= 1, "n must be positive");
  ARGCHK(L >= h->M, "sequence length must be >= motif_length");
  ARGCHK((long)L * 4 < (1 << 20), "sequence too long");
  // the reference reshapes the hidden layer into (…, Lh / pooling, pooling) (convRBM.py:250-252); fit() truncates for it
  ARGCHK((L - h->M + 1) % h->ms().POOL == 0, "hidden length L - motif_length + 1 must be a multiple of pooling");
  return CRBM_OK;
}

int copy_out(crbm_handle* h, float* host, const float* dev, size_t count) {
  HIPCHK(hipMemcpyAsync(host, dev, count * sizeof(float), hipMemcpyDeviceToHost, h->stream));
  return CRBM_OK;
}

// where the letters of a call come from
struct RowSource {
  const float* onehot = nullptr;      // host (n,1,A,L) fp32
  const uint8_t* codes = nullptr;     // host (n,L) bytes 0..A-1
  const uint32_t* resident = nullptr; // device packed rows
  int n = 0, L = 0, A = 4;
  size_t in_bytes_per_row() const { return onehot ? (size_t)4 * A * L : (codes ? (size_t)L : 0); }
};
static RowSource host_onehot_(const float* v, int n, int L, int A) { RowSource s; s.onehot = v; s.n = n; s.L = L; s.A = A; return s; }
static RowSource host_codes_(const uint8_t* c, int n, int L, int A) { RowSource s; s.codes = c; s.n = n; s.L = L; s.A = A; return s; }
#define host_onehot(v, n, L) host_onehot_(v, n, L, h->A)
#define host_codes(c, n, L) host_codes_(c, n, L, h->A)

// ---- the two buffer sets of the evaluation sweeps -------------------------------------------------
// An evaluation sweep walks its rows slab by slab through run_slabs (crbm_sweep.h; sweep_run below binds it to a
// handle).  Slab i is staged, encoded and processed on the stream of set (i & 1) and in that set's buffers; its outputs
// are collected only after slab i+1 has been enqueued, so the host->device copy of one slab overlaps the kernels of the
// other.  Resident sources alternate too: slab i's outputs are still to be copied out when slab i+1 runs.  Three
// invariants make this correct; the first is run_slabs' order of calls, the other two are the features' to keep:
//   1. a set is reused only after its previous slab has been collected;
//   2. nothing is (re)allocated while the other stream runs: whatever both sets write is sized for a whole slab before
//      the sweep starts (an ensure() inside the loop then finds its buffer large enough);
//   3. a slab's outputs are copied from the set that produced them, on that set's stream.
// Everything a slab writes belongs to its set and is reached through sweep_set: staging and letters, the outputs oa / ob,
// the per-motif scratch of the slabbed free energies (SlabModel::fe_scratch), the features' own buffers.
// Set 0 is the handle's main stream and buffers, which the calls outside the sweeps use as well.  What the two streams
// share is read-only during a sweep (parameters, d_tables and d_slab_tables: sweep_begin builds them first) or combined
// in any order (d_flags: atomicOr; the hit summary's position sums: 64-bit integer atomics).
struct SweepSet {
  hipStream_t st;
  DevBuf<float>* stage;
  DevBuf<uint32_t>* letters;
  DevBuf<float>* oa;
  DevBuf<float>* ob;
  DevBuf<float>* fe_scratch;    // of the slab model: never null, but only to be used behind slab_fe_on(h) -- a handle without a slab model has nothing that fills it
  crbm_handle::SetBufs* own;
};
SweepSet sweep_set(crbm_handle* h, int i) {
  if (i & 1) return SweepSet{h->stream2, &h->stage2, &h->letters2, &h->out_a2, &h->out_b2, &h->slab.fe_scratch[1], &h->set_bufs[1]};
  return SweepSet{h->stream, &h->stage, &h->letters, &h->out_a, &h->out_b, &h->slab.fe_scratch[0], &h->set_bufs[0]};
}

// enqueue on the set's stream: rows [start, start+cnt) of a host source, through the set's staging buffer, as packed
// letters at `dst` (no flag check)
int encode_rows(crbm_handle* h, const RowSource& src, int start, int cnt, const SweepSet& set, uint32_t* dst) {
  const int L = src.L, LW = lw(h, L);
  const dim3 grid(grid_for((long)cnt * LW, 256, h->num_cu * 8));
  if (src.onehot) {
    const size_t count = (size_t)cnt * h->A * L;
    HIPCHK(set.stage->ensure(count));
    HIPCHK(hipMemcpyAsync(set.stage->p, src.onehot + (size_t)start * h->A * L, count * sizeof(float), hipMemcpyHostToDevice, set.st));
    EncodeArgs a;
    a.v = set.stage->p; a.letters = dst; a.flags = h->d_flags.p;
    a.n = cnt; a.L = L; a.LW = LW; a.A = h->A;
    if (h->A == 4) hipLaunchKernelGGL(encode_onehot_kernel, grid, dim3(256), 0, set.st, a);
    else hipLaunchKernelGGL(encode_onehot_any_kernel, grid, dim3(256), 0, set.st, a);
  } else {
    const size_t bytes = (size_t)cnt * L;
    HIPCHK(set.stage->ensure((bytes + 3) / 4));
    HIPCHK(hipMemcpyAsync(set.stage->p, src.codes + (size_t)start * L, bytes, hipMemcpyHostToDevice, set.st));
    EncodeCodesArgs a;
    a.codes = reinterpret_cast<const unsigned char*>(set.stage->p);
    a.letters = dst; a.flags = h->d_flags.p;
    a.n = cnt; a.L = L; a.LW = LW; a.A = h->A;
    if (h->A == 4) hipLaunchKernelGGL(encode_codes_kernel, grid, dim3(256), 0, set.st, a);
    else hipLaunchKernelGGL(encode_codes_any_kernel, grid, dim3(256), 0, set.st, a);
  }
  HIPCHK(hipGetLastError());
  return CRBM_OK;
}

// ... on the main stream, the validity flags checked at once; without a destination: into h->letters
int encode_now(crbm_handle* h, const RowSource& src, int start, int cnt, uint32_t* dst = nullptr) {
  if (!dst) {
    HIPCHK(h->letters.ensure((size_t)cnt * lw(h, src.L)));
    dst = h->letters.p;
  }
  const int rc = encode_rows(h, src, start, cnt, sweep_set(h, 0), dst);
  return rc ? rc : check_flags(h);
}

// the slab budget of every sweep: CRBM_SLAB_BYTES or 256 MB, and whether it was set by hand (a sweep over host input
// then does not cap its slabs at 32 MB)
struct SlabBudget {
  size_t bytes;
  bool was_set;
};
SlabBudget slab_budget() { return SlabBudget{(size_t)env_int("CRBM_SLAB_BYTES", 256 << 20), getenv("CRBM_SLAB_BYTES") != nullptr}; }

// rows of a slab whose staged input plus outputs take `bytes_per_row` of the slab budget
int slab_rows(int n, size_t bytes_per_row) {
  const size_t budget = slab_budget().bytes;
  size_t rows = budget / std::max<size_t>(bytes_per_row, 1);
  if (rows < 1) rows = 1;
  return (int)std::min<size_t>(rows, (size_t)n);
}
// rows per slab of a two-stream sweep: host input uses small slabs so that there is something to overlap
int sweep_slab(const RowSource& src, size_t out_bytes_per_row) {
  const size_t per_row = src.in_bytes_per_row() + out_bytes_per_row;
  int slab = slab_rows(src.n, per_row);
  if (!src.resident && !slab_budget().was_set) slab = std::min<size_t>(slab, std::max<size_t>(1, (32u << 20) / std::max<size_t>(per_row, 1)));
  return slab;
}
// tables built and visible to both streams before a sweep starts (the slab tables of a generic DNA model too: a slab on
// the second stream must not find them being rebuilt on the main one)
int sweep_begin(crbm_handle* h) {
  int rc = ensure_tables(h);
  if (rc) return rc;
  if (h->slab.K) {
    rc = slab_ensure_tables(h, h->stream);
    if (rc) return rc;
  }
  HIPCHK(hipStreamSynchronize(h->stream));
  return CRBM_OK;
}
// both streams idle, then the one-hot / code validity flags of every slab at once
int sweep_finish(crbm_handle* h, const RowSource& src) {
  HIPCHK(hipStreamSynchronize(h->stream2));
  HIPCHK(hipStreamSynchronize(h->stream));
  return src.resident ? CRBM_OK : check_flags(h);
}
// a sweep that failed half-way: whatever it has enqueued runs out before the next call resizes a buffer under it, and no
// validity flag stays raised for the next call to trip over (the error already stands in h->err)
void sweep_drain(crbm_handle* h) {
  (void)hipStreamSynchronize(h->stream2);
  (void)hipStreamSynchronize(h->stream);
  (void)hipMemsetAsync(h->d_flags.p, 0, sizeof(uint32_t), h->stream);
  (void)hipStreamSynchronize(h->stream);
}

// run_slabs over a source, in slabs of `slab` rows.  launch(set, rows, start, cnt) enqueues the kernels of rows
// [start, start+cnt) on `set`; `rows` are their packed letters, a resident source's own or a host source's staged and
// encoded into the set's letters just before.  collect(set, rows, start, cnt) copies that slab's outputs out on the
// set's stream and waits for them.  Depth 2 (after sweep_begin): the two streams, the validity flags of all slabs checked
// at the end.  Depth 1: the main stream alone, the flags of each slab checked before its kernels go out.  The staging and
// letter buffers of every set in use are sized here, before anything runs; what the launches write is the caller's to size.
template <class Launch, class Collect>
int sweep_run(crbm_handle* h, const RowSource& src, int slab, int depth, Launch launch, Collect collect) {
  const int LW = lw(h, src.L);
  for (int s = 0; s < (depth == 2 && slab < src.n ? 2 : 1) && !src.resident; ++s) {
    const SweepSet set = sweep_set(h, s);
    HIPCHK(set.letters->ensure((size_t)slab * LW));
    HIPCHK(set.stage->ensure(src.onehot ? (size_t)slab * h->A * src.L : ((size_t)slab * src.L + 3) / 4));
  }
  const uint32_t* rows[2] = {nullptr, nullptr};
  const int rc = run_slabs(src.n, slab, depth,
    [&](int, int s, int start, int cnt) -> int {
      const SweepSet set = sweep_set(h, s);
      rows[s] = src.resident ? src.resident + (size_t)start * LW : set.letters->p;
      int r = src.resident ? CRBM_OK : encode_rows(h, src, start, cnt, set, set.letters->p);
      if (!r && depth == 1 && !src.resident) r = check_flags(h);
      return r ? r : launch(set, rows[s], start, cnt);
    },
    [&](int, int s, int start, int cnt) -> int { return collect(sweep_set(h, s), rows[s], start, cnt); },
    [&] { sweep_drain(h); });
  if (rc || depth == 1) return rc;
  return sweep_finish(h, src);
}

// ---- the stream sweep (crbm_scan_*_codes, crbm_variant_effects_codes, crbm_allele_effects_codes) --------------------
// What every feature over a stream of T codes (0..3 letters, 4 no letter) shares: a two-stream sweep over chunks.  Per
// chunk, on its set's stream: the staged bytes go up (one per code), scan_encode_kernel makes letters and validity
// plane, then the feature's kernels run on the ScanInput the sweep hands it.  A generic DNA model runs the kernels of
// its slab model, blockIdx.y = slab.  The features differ in what a chunk is and where its bytes come from: segments of
// window starts read straight from the stream (run), or variants whose contexts the host gathers first (the stage
// callables of variant_effects_any and allele_effects_any).  In order:
//   admit()        the checks on the stream and the model, under the entry point's name; whose kernels run (kms, kjk)
//   begin()        for the segment sweeps: tables built, the segments planned (stream_plan: segment [start, start + cnt)
//                  needs letters [start, start + cnt + M - 1), a halo of M - 1 behind its own), size_inputs
//   size_inputs()  stage, letters and validity plane of every set, sized for a whole chunk; the feature then sizes what
//                  its own kernels write -- all of it before run_chunks, while neither stream runs
//   run_chunks()   walks (n, slab) as run_slabs does.  stage(si, c) names the chunk's host bytes and what is made of
//                  them (Chunk); launch(set, si, in, start, cnt) enqueues the feature's kernels; collect(...) copies that
//                  chunk's outputs out on the set's stream, which the sweep then waits for: the set's buffers are free
//                  again.  `timing_env` set to 1: events around every chunk's kernels, their sum on stderr, counted in
//                  `unit`.  At the end both streams are idle and a code above 4 anywhere in what was staged is refused
//                  (a feature that has checked the stream on the host pays one 4-byte copy for a flag that is never
//                  raised); a failed sweep is drained (sweep_drain).
//   run()          run_chunks over the plan's segments, staged where they lie in `codes`
const char* const kBadStreamCode = "stream codes must lie in 0..4 (0..3 = A,C,G,T; 4 = no letter)";
// the refusal of the sweep's epilogue, on the host: for what must be refused before anything is launched
int check_stream_codes(crbm_handle* h, const uint8_t* codes, int64_t T) {
  unsigned bad = 0;
  for (int64_t i = 0; i < T; ++i) bad |= codes[i] > 4 ? 1u : 0u;
  ARGCHK(!bad, kBadStreamCode);
  return CRBM_OK;
}

struct StreamSweep {
  crbm_handle* h;
  const char* api;                       // the entry point: named in its refusals and in its timing line
  const ModelShape* kms = nullptr;       // whose kernels run: the model's own, or those of its slab model
  const JitKernels* kjk = nullptr;
  int M = 0, S = 0, nslab = 0;
  StreamPlan plan{};

  // one chunk as its stage() leaves it; start and cnt come in as run_slabs counts them
  struct Chunk {
    int start, cnt;                      // what launch and collect are told
    const uint8_t* bytes;                // host bytes to copy up, `up` of them
    size_t up;
    long n, layout_starts;               // staged codes to encode; scan_layout(n, layout_starts)
    int32_t starts;                      // ScanInput::starts
  };

  int admit(const uint8_t* codes, int64_t T) {
    const std::string who = std::string(api) + ": ";
    ARGCHK(T >= 0 && T <= (int64_t)INT32_MAX, "stream length must lie in [0, 2^31 - 1] (start is 32 bits wide)");
    ARGCHK(codes || T == 0, "null argument");
    ARGCHK(h->A == 4, who + "the alphabet must be DNA's (input_dims == 4)");
    ARGCHK(h->ms().POOL == 1, who + "pooling > 1 is not supported (pool groups have no anchor in a stream)");
    kms = h->big() ? &h->slab.ms : &h->ms();
    kjk = h->big() ? &h->slab.jk : &h->jk;
    ARGCHK((!h->big() || h->slab.K) && tab_bytes(*kms) <= 160 * 1024, who + "models that run on the generic kernels alone (motifs beyond 64 letters) are not supported");
    M = h->M; S = h->ds ? 2 : 1; nslab = h->big() ? h->slab_n : 1;
    return CRBM_OK;
  }

  int size_inputs(int nsets, size_t staged_bytes, const ScanLayout& full) {
    for (int i = 0; i < nsets; ++i) {
      const SweepSet set = sweep_set(h, i);
      HIPCHK(set.stage->ensure((staged_bytes + 3) / 4));
      HIPCHK(set.letters->ensure((size_t)full.letter_words));
      HIPCHK(set.own->scan_valid.ensure((size_t)full.valid_words));
    }
    return CRBM_OK;
  }

  int begin(int64_t T) {                 // T >= M
    const int rc = sweep_begin(h);
    if (rc) return rc;
    const SlabBudget budget = slab_budget();
    plan = stream_plan((long)T, M, nslab, budget.bytes, budget.was_set);
    return size_inputs(plan.nsets, (size_t)plan.seg + M - 1, plan.full);
  }

  // what every stream kernel reads of a chunk encoded into `set`: the one place a ScanInput is filled
  ScanInput input(const SweepSet& set, int32_t starts, int32_t tiles) const {
    ScanInput a;
    a.tables = h->big() ? h->d_slab_tables.p : h->d_tables.p;
    a.letters = set.letters->p; a.valid = set.own->scan_valid.p;
    a.starts = starts; a.tiles = tiles; a.table_stride = kms->TABLES_ALL;
    if (h->big()) a.plan = slab_plan(h);
    else { a.plan.Ks = h->K; a.plan.K = h->K; a.plan.last_k0 = 0; }
    return a;
  }

  template <class Stage, class Launch, class Collect>
  int run_chunks(int n, int slab, const char* timing_env, const char* unit, Stage stage, Launch launch, Collect collect) {
    const bool timing = env_int(timing_env, 0) != 0;
    Event tev[2][2];
    double device_ms = 0.0;
    int timed = 0;
    if (timing)
      for (int i = 0; i < 2; ++i)
        for (int j = 0; j < 2; ++j) HIPCHK(tev[i][j].create());
    ScanInput in[2];
    Chunk chunk[2];
    const int rc = run_slabs(n, slab, 2,
      [&](int, int si, int start, int cnt) -> int {
        const SweepSet set = sweep_set(h, si);
        Chunk& c = chunk[si];
        c = Chunk{start, cnt, nullptr, 0, 0, 0, 0};
        int r = stage(si, c);
        if (r) return r;
        const ScanLayout l = scan_layout(c.n, c.layout_starts);
        HIPCHK(hipMemcpyAsync(set.stage->p, c.bytes, c.up, hipMemcpyHostToDevice, set.st));
        if (timing) HIPCHK(hipEventRecord(tev[si][0], set.st));
        ScanEncodeArgs e;
        e.codes = reinterpret_cast<const unsigned char*>(set.stage->p);
        e.letters = set.letters->p; e.valid = set.own->scan_valid.p; e.flags = h->d_flags.p;
        e.n = c.n; e.valid_words = l.valid_words;
        hipLaunchKernelGGL(scan_encode_kernel, dim3(grid_for(l.valid_words, 256, h->num_cu * 8)), dim3(256), 0, set.st, e);
        HIPCHK(hipGetLastError());
        in[si] = input(set, c.starts, l.tiles);
        r = launch(set, si, in[si], c.start, c.cnt);
        if (!r && timing) HIPCHK(hipEventRecord(tev[si][1], set.st));
        return r;
      },
      [&](int, int si, int, int) -> int {
        const SweepSet set = sweep_set(h, si);
        const int r = collect(set, si, in[si], chunk[si].start, chunk[si].cnt);
        if (r) return r;
        HIPCHK(hipStreamSynchronize(set.st));
        if (timing) {
          float ms = 0.f;
          HIPCHK(hipEventElapsedTime(&ms, tev[si][0], tev[si][1]));
          device_ms += ms;
          ++timed;
        }
        return CRBM_OK;
      },
      [&] { sweep_drain(h); });
    if (rc) return rc;
    if (timing) fprintf(stderr, "%s: kernels %.3f ms over %d %s\n", api, device_ms, timed, unit);
    HIPCHK(hipStreamSynchronize(h->stream2));
    HIPCHK(hipStreamSynchronize(h->stream));
    uint32_t flags = 0;
    HIPCHK(hipMemcpyAsync(&flags, h->d_flags.p, sizeof(flags), hipMemcpyDeviceToHost, h->stream));
    HIPCHK(hipStreamSynchronize(h->stream));
    if (flags) {
      HIPCHK(hipMemsetAsync(h->d_flags.p, 0, sizeof(uint32_t), h->stream));
      HIPCHK(hipStreamSynchronize(h->stream));
      return fail(h, CRBM_ERR_INVALID, kBadStreamCode);
    }
    return CRBM_OK;
  }

  template <class Launch, class Collect>
  int run(const uint8_t* codes, const char* timing_env, Launch launch, Collect collect) {
    return run_chunks(plan.starts_all, plan.seg, timing_env, "segments",
      [&](int, Chunk& c) -> int {        // (start + cnt <= T - M + 1: the halo is inside the stream)
        c.bytes = codes + c.start; c.n = (long)c.cnt + M - 1; c.up = (size_t)c.n;
        c.layout_starts = c.cnt; c.starts = c.cnt;
        return CRBM_OK;
      },
      launch, collect);
  }
};

}  // namespace

// =============================================================================
extern "C" {

int crbm_abi_version(void) { return CRBM_AMD_ABI_VERSION; }

int crbm_device_count(void) {
  int n = 0;
  if (hipGetDeviceCount(&n) != hipSuccess) return 0;
  return n;
}

const char* crbm_last_error(const crbm_handle* h) { return h ? h->err.c_str() : g_create_error.c_str(); }

}  // extern "C"

namespace {

int validate_config(const crbm_config* cfg) {
  crbm_handle* h = nullptr;   // fail() routes to the create-error slot
  if (!cfg) return fail(h, CRBM_ERR_INVALID, "null argument");
  ARGCHK(cfg->num_motifs >= 1, "Number of motifs must be positive.");
  // (beyond 256 motifs / 64 letters / what the LDS holds the generic kernels take over: crbm_create)
  ARGCHK(cfg->num_motifs <= 65536, "num_motifs > 65536 is not supported");
  ARGCHK(cfg->motif_length >= 1, "Motif length must be positive.");
  ARGCHK(cfg->input_dims >= 1, "input_dims must be positive.");
  ARGCHK(cfg->input_dims <= 64, "input_dims > 64 is not supported (v|h keeps a position's activations of all letters in LDS)");
  ARGCHK(cfg->input_dims * cfg->motif_length <= 256 * BIG_ST, "input_dims * motif_length > 2048 is not supported (statistics kernel: one accumulator per letter and filter column, 8 per thread of a 256-thread block; DNA: motif_length <= 512)");
  ARGCHK((long)cfg->num_motifs * cfg->motif_length * cfg->input_dims <= (1L << 26), "num_motifs * input_dims * motif_length too large");
  ARGCHK(cfg->pooling >= 1 && cfg->pooling <= 64, "pooling must be between 1 and 64");
  ARGCHK(cfg->fantasy_hidden_len % cfg->pooling == 0, "pooling must divide the hidden length of the fantasy chains");
  ARGCHK(cfg->batchsize >= 1, "batchsize must be positive.");
  ARGCHK(cfg->cd_k >= 1, "cd_k must be positive.");
  ARGCHK(cfg->fantasy_hidden_len >= 1 && cfg->fantasy_hidden_len <= 65536, "fantasy_hidden_len out of range");
  ARGCHK(cfg->rho > 0.f && cfg->rho < 1.f, "rho must be in (0,1)");
  ARGCHK(cfg->learning_rate > 0.f, "learning_rate must be positive.");
  ARGCHK(cfg->momentum >= 0.f && cfg->momentum < 1.f, "momentum must be between zero and one.");
  ARGCHK(cfg->lambda_rate >= 0.f, "lambda_rate must be non-negative.");
  return CRBM_OK;
}

}  // namespace

extern "C" {

// Compile the kernels of a model into the on-disk cache without touching a GPU
// (used by __graft_entry__.build()).
int crbm_precompile(const crbm_config* cfg) {
  int rc = validate_config(cfg);
  if (rc) return rc;
  // the kernels of the plan crbm_create will derive for this model (on a device of CRBM_NUM_CU compute units, 256 unless set)
  const LaunchPlan p = plan_launches(cfg->num_motifs, cfg->motif_length, cfg->doublestranded ? 1 : 0, cfg->input_dims, cfg->pooling,
                                     cfg->fantasy_hidden_len > 0 ? cfg->fantasy_hidden_len : 200, cfg->batchsize, env_int("CRBM_NUM_CU", 256));
  std::vector<char> code;
  bool cached = false;
  std::string file, err;
  int rc_jit = 0;
  if (!p.big)
    rc_jit = jit_compile(p.ms.K, p.ms.M, p.ms.DS, p.G, p.GS, p.ms.POOL, p.gibbs_wpe, p.gibbs_tb, &code, &cached, &file, &err);
  else if (p.slab_K > 0)      // the generic kernels are compiled ahead of time; the kernels of the model's slab model are specialised
    rc_jit = jit_compile(p.slab_K, p.ms.M, p.ms.DS, p.slab_G, p.slab_G, p.slab_ms.POOL, 0, 256, &code, &cached, &file, &err, true);
  if (rc_jit == 0 && !p.big && (p.geo_plain.on() || p.geo_fused.on())) {
    const int Lf = cfg->fantasy_hidden_len > 0 ? cfg->fantasy_hidden_len : 200;
    rc_jit = jit_compile_geo(p.ms.K, p.ms.M, p.ms.DS, p.ms.POOL, p.gibbs_wpe, jit_geo(p.geo_plain, Lf), jit_geo(p.geo_fused, Lf), &code, &cached, &file, &err);
  }
  if (rc_jit != 0) {
    g_create_error = err;
    return CRBM_ERR_HIP;
  }
  return CRBM_OK;
}

int crbm_create(const crbm_config* cfg, crbm_handle** out) {
  crbm_handle* h = nullptr;   // fail() routes to the create-error slot
  if (!cfg || !out) return fail(h, CRBM_ERR_INVALID, "null argument");
  *out = nullptr;
  int rc = validate_config(cfg);
  if (rc) return rc;
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0)
    return fail(h, CRBM_ERR_NO_GPU, "no HIP device visible (this library has no CPU path)");
  ARGCHK(cfg->device >= 0 && cfg->device < ndev, "device ordinal out of range");

  std::unique_ptr<crbm_handle> hh(new crbm_handle());      // deleted on every early return below
  hh->cfg = *cfg;
  hh->K = cfg->num_motifs; hh->M = cfg->motif_length; hh->ds = cfg->doublestranded ? 1 : 0;
  hh->A = cfg->input_dims;
  hh->KAM = hh->K * hh->A * hh->M;
  hh->Lf = cfg->fantasy_hidden_len; hh->Lv = hh->Lf + hh->M - 1; hh->B = cfg->batchsize;
  hh->seed = cfg->seed;
  hh->device = cfg->device;
  hh->sl = sums_layout(hh->K, hh->M, hh->A);
  HIPCHK(hipSetDevice(hh->device));
  hipDeviceProp_t prop;
  HIPCHK(hipGetDeviceProperties(&prop, hh->device));
  hh->num_cu = prop.multiProcessorCount > 0 ? prop.multiProcessorCount : 256;
  {
    int khz = 0;      // ticks of the GPU's constant-rate clock (s_memrealtime) per millisecond
    if (hipDeviceGetAttribute(&khz, hipDeviceAttributeWallClockRate, hh->device) == hipSuccess && khz > 0) hh->wall_khz = khz;
    (void)hipGetLastError();
  }
  // which kernels, launch geometry (crbm_plan.h), then the model-specific kernels (hiprtc; cached on disk)
  hh->plan = plan_launches(hh->K, hh->M, hh->ds, hh->A, cfg->pooling, hh->Lf, hh->B, hh->num_cu);
  const LaunchPlan& plan = hh->plan;
  hh->NW = plan.ms.NW;
  if (plan.refusal) return fail(h, CRBM_ERR_INVALID, plan.refusal);
  // (generic models: no specialised kernels, no table images; the state layout is the same -- K-bit masks, 2-bit letters)
  hh->LWs = hh->big() ? letter_words_any(hh->A, hh->Lv) : plan.chain[1].gl.LWs;
  hh->variant = 1; hh->topdown_mode = 2;
  if (!hh->big()) {
    // The set-bit walk is the variant of every model (its cost follows the hidden activity,
    // ~2 % under the reference's sparsity target); CRBM_TOPDOWN=dense pins the table variant
    // of small models for A/B runs.  Never switched at run time: the two round differently.
    const char* td = getenv("CRBM_TOPDOWN");
    hh->topdown_mode = (td && !strcmp(td, "dense") && plan.has_dense) ? 1 : 2;
    hh->variant = hh->topdown_mode == 1 ? 0 : 1;
    std::string err;
    if (jit_load(hh->K, hh->M, hh->ds, plan.G, plan.GS, hh->ms().POOL, plan.gibbs_wpe, plan.gibbs_tb, &hh->jk, &err) != 0)
      return fail(h, CRBM_ERR_HIP, "kernel specialisation failed: " + err);
    // (only the set-bit walk has them: a handle pinned to the dense variant never consults jg and does not pay for it)
    if (hh->variant == 1 &&
        jit_load_geo(hh->K, hh->M, hh->ds, hh->ms().POOL, plan.gibbs_wpe, jit_geo(plan.geo_plain, hh->Lf), jit_geo(plan.geo_fused, hh->Lf), &hh->jg, &err) != 0)
      return fail(h, CRBM_ERR_HIP, "kernel specialisation (launch geometry) failed: " + err);
  }
  HIPCHK(hh->stream.create());
  HIPCHK(hh->stream2.create());
  HIPCHK(hh->ev0.create());
  HIPCHK(hh->ev1.create());
  HIPCHK(hh->ev_fork.create_untimed());
  HIPCHK(hh->ev_join.create_untimed());
  if (plan.chain_parts > 1) {
    HIPCHK(hh->ev_parts_fork.create_untimed());
    HIPCHK(hh->ev_cal0.create());
    HIPCHK(hh->ev_cal1.create());
    for (int p = 1; p < plan.chain_parts; ++p) {      // (partition 0 rides on the handle's own stream: one hardware queue fewer)
      Partition& part = hh->part[p];
      HIPCHK(part.stream.create());
      HIPCHK(part.done.create());                // with timestamps: crbm_time_gibbs reads them
      part.worker.reset(new PartWorker());
      part.worker->device = hh->device;
      part.worker->stream = part.stream;
      part.worker->th = std::thread(part_worker_main, part.worker.get());
    }
  }
  hh->overlap = env_int("CRBM_OVERLAP", 0) != 0;   // measured: no gain once the statistics kernel fills the chip
  // (generic handles: W and b carry ten motifs of zero padding behind motif K -- the last slab of the slabbed kernels
  //  starts on a multiple of ten and may reach past the model's end, slab_origin)
  const size_t pad_k = hh->big() ? 10 : 0;
  const size_t kam = (size_t)hh->KAM + pad_k * hh->A * hh->M, k = (size_t)hh->K + pad_k;
  const size_t cb = (size_t)std::max(4, hh->A);
  HIPCHK(hh->dW.alloc_zeroed(kam)); HIPCHK(hh->dvW.alloc_zeroed(kam));
  HIPCHK(hh->db.alloc_zeroed(k));   HIPCHK(hh->dvb.alloc_zeroed(k));
  HIPCHK(hh->dc.alloc_zeroed(cb));  HIPCHK(hh->dvc.alloc_zeroed(cb));
  HIPCHK(hh->dW2.alloc(kam)); HIPCHK(hh->dvW2.alloc(kam));
  HIPCHK(hh->db2.alloc(k));   HIPCHK(hh->dvb2.alloc(k));
  HIPCHK(hh->dc2.alloc(cb));  HIPCHK(hh->dvc2.alloc(cb));
  HIPCHK(hh->d_tables.alloc(hh->big() ? 16 : (size_t)hh->ms().TABLES_ALL));
  if (plan.GS != plan.G) HIPCHK(hh->d_tf_solo.alloc((size_t)plan.ms_solo.TAB));
  const size_t mwords = (size_t)hh->B * hh->Lf * hh->NW;
  HIPCHK(hh->d_hm.alloc_zeroed(mwords));
  HIPCHK(hh->d_hmp.alloc_zeroed(mwords));
  const size_t vwords = (size_t)hh->B * hh->LWs;
  HIPCHK(hh->d_vf.alloc_zeroed(vwords));
  HIPCHK(hh->d_flags.alloc_zeroed(4));
  HIPCHK(hh->d_ones.alloc_zeroed(2));
  {
    // one slot per wave of the largest launch; a partitioned launch is chain_parts launches of the partition's geometry
    size_t slots = plan.part.on() ? (size_t)plan.chain_parts * plan.part.grid * (plan.part.threads / 64) : 0;
    for (const ChainGeom* g : {&plan.chain[0], &plan.chain[1], &plan.solo})
      if (g->on()) slots = std::max(slots, (size_t)g->grid * (g->threads / 64));
    slots += 64;
    HIPCHK(hh->d_nset.alloc_zeroed(slots));
  }
  HIPCHK(hh->d_sums.alloc_zeroed((size_t)hh->sl.count));
  HIPCHK(hh->d_ticket.alloc_zeroed(4));
  HIPCHK(hh->d_probe.alloc_zeroed(4));
  // the memsets above go out on the null stream, which the handle's non-blocking streams do not wait for: without this
  // a zeroing of W, b, c could land after the crbm_set_params that follows (seen: a generic model evaluated with W = 0)
  HIPCHK(hipDeviceSynchronize());
  hh->tables_dirty = true;
  {
    const char* sv = getenv("CRBM_STATS");
    hh->fuse_stats = !hh->big() && hh->ms().FUSE_STATS && hh->variant == 1 && !(sv && !strcmp(sv, "split"));
    hh->one_launch = !(sv && !strcmp(sv, "two"));
    if (hh->fuse_stats) {   // the fused launch appends the statistics slices to the chain image: it must fit the LDS
      const ChainGeom& g = plan.chain[hh->variant];
      const StatsMfmaLayout st = stats_mfma_layout(hh->ms(), 0, hh->Lf, g.threads, 0, false);
      const int lds = std::max((((g.gl.lds_bytes / 4 + 3) & ~3) + st.region_floats) * 4, st.combine_bytes);
      if (lds > 160 * 1024) hh->fuse_stats = false;
    }
  }
  hh->stats_rows = env_int("CRBM_STATS_ROWS", 0);   // 0: one resident wave of blocks
  slab_setup(hh.get());                             // generic DNA models: their statistics on the matrix cores, slab by slab
  *out = hh.release();
  return CRBM_OK;
}

int crbm_destroy(crbm_handle* h) {
  if (!h) return CRBM_OK;
  (void)hipSetDevice(h->device);
  if (h->comm && g_rccl.CommDestroy) {
    (void)hipStreamSynchronize(h->stream);      // the collectives of the communicator ran on it
    g_rccl.CommDestroy(h->comm);
  }
  delete h;      // every member releases what it owns, in the order the struct states
  return CRBM_OK;
}

// ENTER_ASYNC: entry points that may leave work on the partition streams (plain chain launches); every other entry point
// first lets the main stream wait for them (join_parts: two event calls per partition, only when something is pending)
#define ENTER_ASYNC()                                         \
  if (!h) return CRBM_ERR_INVALID;                            \
  h->err.clear();                                             \
  HIPCHK(hipSetDevice(h->device))
#define ENTER()                                               \
  ENTER_ASYNC();                                              \
  do {                                                        \
    const int jrc__ = join_parts(h);                          \
    if (jrc__) return jrc__;                                  \
  } while (0)

int crbm_set_params(crbm_handle* h, const float* W, const float* b, const float* c) {
  ENTER();
  ARGCHK(W && b && c, "null argument");
  HIPCHK(hipMemcpyAsync(h->dW.p, W, (size_t)h->KAM * 4, hipMemcpyHostToDevice, h->stream));
  HIPCHK(hipMemcpyAsync(h->db.p, b, (size_t)h->K * 4, hipMemcpyHostToDevice, h->stream));
  HIPCHK(hipMemcpyAsync(h->dc.p, c, (size_t)h->A * 4, hipMemcpyHostToDevice, h->stream));
  HIPCHK(hipStreamSynchronize(h->stream));
  h->tables_dirty = true;
  h->params_version += 1;
  return CRBM_OK;
}

int crbm_get_params(crbm_handle* h, float* W, float* b, float* c) {
  ENTER();
  ARGCHK(W && b && c, "null argument");
  HIPCHK(hipMemcpyAsync(W, h->dW.p, (size_t)h->KAM * 4, hipMemcpyDeviceToHost, h->stream));
  HIPCHK(hipMemcpyAsync(b, h->db.p, (size_t)h->K * 4, hipMemcpyDeviceToHost, h->stream));
  HIPCHK(hipMemcpyAsync(c, h->dc.p, (size_t)h->A * 4, hipMemcpyDeviceToHost, h->stream));
  HIPCHK(hipStreamSynchronize(h->stream));
  return CRBM_OK;
}

int crbm_set_velocities(crbm_handle* h, const float* vW, const float* vb, const float* vc) {
  ENTER();
  ARGCHK(vW && vb && vc, "null argument");
  HIPCHK(hipMemcpyAsync(h->dvW.p, vW, (size_t)h->KAM * 4, hipMemcpyHostToDevice, h->stream));
  HIPCHK(hipMemcpyAsync(h->dvb.p, vb, (size_t)h->K * 4, hipMemcpyHostToDevice, h->stream));
  HIPCHK(hipMemcpyAsync(h->dvc.p, vc, (size_t)h->A * 4, hipMemcpyHostToDevice, h->stream));
  HIPCHK(hipStreamSynchronize(h->stream));
  return CRBM_OK;
}

int crbm_get_velocities(crbm_handle* h, float* vW, float* vb, float* vc) {
  ENTER();
  ARGCHK(vW && vb && vc, "null argument");
  HIPCHK(hipMemcpyAsync(vW, h->dvW.p, (size_t)h->KAM * 4, hipMemcpyDeviceToHost, h->stream));
  HIPCHK(hipMemcpyAsync(vb, h->dvb.p, (size_t)h->K * 4, hipMemcpyDeviceToHost, h->stream));
  HIPCHK(hipMemcpyAsync(vc, h->dvc.p, (size_t)h->A * 4, hipMemcpyDeviceToHost, h->stream));
  HIPCHK(hipStreamSynchronize(h->stream));
  return CRBM_OK;
}

int crbm_set_fantasy(crbm_handle* h, const float* hid, const float* hid_prime) {
  ENTER();
  ARGCHK(hid, "null argument");
  ARGCHK(!h->ds || hid_prime, "doublestranded model needs hid_prime");
  const size_t count = (size_t)h->B * h->K * h->Lf;
  HIPCHK(h->stage.ensure(count));
  const float* src[2] = {hid, hid_prime};
  uint32_t* dst[2] = {h->d_hm.p, h->d_hmp.p};
  for (int sidx = 0; sidx < 1 + h->ds; ++sidx) {
    HIPCHK(hipMemcpyAsync(h->stage.p, src[sidx], count * 4, hipMemcpyHostToDevice, h->stream));
    HiddenPackArgs a;
    a.dense = h->stage.p; a.masks = dst[sidx]; a.flags = h->d_flags.p;
    a.n = h->B; a.K = h->K; a.Lh = h->Lf; a.NW = h->NW;
    hipLaunchKernelGGL(pack_hidden_kernel, dim3(grid_for((long)h->B * h->Lf, 256, h->num_cu * 8)), dim3(256), 0, h->stream, a);
    HIPCHK(hipGetLastError());
    HIPCHK(hipStreamSynchronize(h->stream));   // staging buffer is reused
  }
  return check_flags(h);
}

int crbm_get_fantasy(crbm_handle* h, float* hid, float* hid_prime) {
  ENTER();
  ARGCHK(hid, "null argument");
  const size_t count = (size_t)h->B * h->K * h->Lf;
  HIPCHK(h->stage.ensure(count));
  float* dsth[2] = {hid, hid_prime};
  uint32_t* src[2] = {h->d_hm.p, h->d_hmp.p};
  for (int sidx = 0; sidx < 1 + h->ds; ++sidx) {
    if (!dsth[sidx]) continue;
    HiddenPackArgs a;
    a.dense = h->stage.p; a.masks = src[sidx]; a.flags = h->d_flags.p;
    a.n = h->B; a.K = h->K; a.Lh = h->Lf; a.NW = h->NW;
    hipLaunchKernelGGL(unpack_hidden_kernel, dim3(grid_for((long)h->B * h->Lf, 256, h->num_cu * 8)), dim3(256), 0, h->stream, a);
    HIPCHK(hipGetLastError());
    HIPCHK(hipMemcpyAsync(dsth[sidx], h->stage.p, count * 4, hipMemcpyDeviceToHost, h->stream));
    HIPCHK(hipStreamSynchronize(h->stream));
  }
  return CRBM_OK;
}

int crbm_get_fantasy_visible(crbm_handle* h, float* v) {
  ENTER();
  ARGCHK(v, "null argument");
  const size_t count = (size_t)h->B * h->A * h->Lv;
  HIPCHK(h->stage.ensure(count));
  DecodeArgs a;
  a.letters = h->d_vf.p; a.v = h->stage.p; a.n = h->B; a.L = h->Lv; a.LW = h->LWs; a.A = h->A;
  if (h->A == 4) hipLaunchKernelGGL(decode_onehot_kernel, dim3(grid_for((long)h->B * h->Lv, 256, h->num_cu * 8)), dim3(256), 0, h->stream, a);
  else hipLaunchKernelGGL(decode_onehot_any_kernel, dim3(grid_for((long)h->B * h->Lv, 256, h->num_cu * 8)), dim3(256), 0, h->stream, a);
  HIPCHK(hipGetLastError());
  HIPCHK(hipMemcpyAsync(v, h->stage.p, count * 4, hipMemcpyDeviceToHost, h->stream));
  HIPCHK(hipStreamSynchronize(h->stream));
  return CRBM_OK;
}

int crbm_set_rng(crbm_handle* h, uint64_t seed, uint32_t gibbs_step, uint32_t eval_step) {
  if (!h) return CRBM_ERR_INVALID;
  h->seed = seed; h->gibbs_step = gibbs_step; h->eval_step = eval_step;
  return CRBM_OK;
}

int crbm_get_rng(crbm_handle* h, uint64_t* seed, uint32_t* gibbs_step, uint32_t* eval_step) {
  if (!h) return CRBM_ERR_INVALID;
  if (seed) *seed = h->seed;
  if (gibbs_step) *gibbs_step = h->gibbs_step;
  if (eval_step) *eval_step = h->eval_step;
  return CRBM_OK;
}

int crbm_set_shard(crbm_handle* h, uint32_t chain_offset) {
  if (!h) return CRBM_ERR_INVALID;
  h->chain_offset = chain_offset;
  return CRBM_OK;
}

// ---- training ----------------------------------------------------------------
int crbm_train_step(crbm_handle* h, const float* D, int32_t n, int32_t L) {
  ENTER();
  ARGCHK(D, "null argument");
  int rc = check_data_shape(h, n, L);
  if (rc) return rc;
  rc = encode_now(h, host_onehot(D, n, L), 0, n);
  if (rc) return rc;
  rc = train_core(h, h->letters.p, n, L);
  if (rc) return rc;
  HIPCHK(hipStreamSynchronize(h->stream));
  return ipc_check(h);
}

int crbm_dataset_select(crbm_handle* h, int32_t slot) {
  ENTER();
  ARGCHK(slot >= 0 && slot < CRBM_DATASET_SLOTS, "no such data-set slot");
  h->slot = slot;
  return CRBM_OK;
}

int crbm_dataset_upload(crbm_handle* h, const float* data, int32_t n, int32_t L) {
  ENTER();
  ARGCHK(data, "null argument");
  int rc = check_data_shape(h, n, L);
  if (rc) return rc;
  const int LW = lw(h, L);
  DevBuf<uint32_t>& ds = h->dataset[h->slot];
  h->dataset_n[h->slot] = 0;
  HIPCHK(ds.ensure((size_t)n * LW));
  // stream the fp32 array through the staging buffer in slabs of <= 64 MiB
  const int slab = std::max(1, (int)std::min<long>(n, (64L << 20) / ((long)h->A * L * 4)));
  const RowSource src = host_onehot(data, n, L);
  for (int start = 0; start < n; start += slab) {
    const int cnt = std::min(slab, n - start);
    rc = encode_now(h, src, start, cnt, ds.p + (size_t)start * LW);
    if (rc) return rc;
  }
  h->dataset_n[h->slot] = n; h->dataset_L[h->slot] = L;
  return CRBM_OK;
}

int crbm_dataset_upload_codes(crbm_handle* h, const uint8_t* codes, int32_t n, int32_t L) {
  ENTER();
  ARGCHK(codes, "null argument");
  int rc = check_data_shape(h, n, L);
  if (rc) return rc;
  const int LW = lw(h, L);
  DevBuf<uint32_t>& ds = h->dataset[h->slot];
  h->dataset_n[h->slot] = 0;
  HIPCHK(ds.ensure((size_t)n * LW));
  const int slab = std::max(1, (int)std::min<long>(n, (256L << 20) / (long)L));
  const RowSource src = host_codes(codes, n, L);
  for (int start = 0; start < n; start += slab) {
    const int cnt = std::min(slab, n - start);
    rc = encode_now(h, src, start, cnt, ds.p + (size_t)start * LW);
    if (rc) return rc;
  }
  h->dataset_n[h->slot] = n; h->dataset_L[h->slot] = L;
  return CRBM_OK;
}

int crbm_train_step_resident(crbm_handle* h, int32_t start, int32_t end) {
  ENTER();
  const int slot = h->slot;
  ARGCHK(h->dataset_n[slot] > 0, "no resident data set (call crbm_dataset_upload)");
  ARGCHK(start >= 0 && end >= start && end <= h->dataset_n[slot], "row range out of bounds");
  ARGCHK(end > start || h->comm || h->ipc_on, "empty row range");
  const int LW = lw(h, h->dataset_L[slot]);
  int rc = train_core(h, h->dataset[slot].p + (size_t)start * LW, end - start, h->dataset_L[slot]);
  if (rc) return rc;
  HIPCHK(hipStreamSynchronize(h->stream));
  return ipc_check(h);
}

// One pass over the resident data set in sequential mini-batches of `batchsize`
// rows (the slices of convRBM.py:722-726, last one short), each a full PCD-k
// update; rank r of a communicator takes its contiguous share of every batch.
// The steps are enqueued back to back: one host synchronisation per epoch
// instead of one per step.
int crbm_train_epoch_resident(crbm_handle* h, int32_t batchsize) {
  ENTER();
  const int slot = h->slot;
  ARGCHK(h->dataset_n[slot] > 0, "no resident data set (call crbm_dataset_upload)");
  ARGCHK(batchsize >= 1, "batchsize must be positive");
  const int total = h->dataset_n[slot], L = h->dataset_L[slot], LW = lw(h, L);
  for (int start = 0; start < total; start += batchsize) {
    const int end = std::min(total, start + batchsize), n = end - start;
    const int lo = start + (int)(((long)n * h->rank) / h->nranks), hi = start + (int)(((long)n * (h->rank + 1)) / h->nranks);
    int rc = train_core(h, h->dataset[slot].p + (size_t)lo * LW, hi - lo, L);
    if (rc) return rc;
  }
  HIPCHK(hipStreamSynchronize(h->stream));
  return ipc_check(h);
}

// The same loop when the selected slot holds only THIS rank's rows: for every
// slice [start, end) of the global data set of `total_rows` rows, rank r owns rows
// [start + n*r/R, start + n*(r+1)/R) (n = end - start) and the resident set is their
// concatenation in slice order (crbm_amd.dist.shard_rows builds it), so a rank
// uploads 1/R of the data instead of all of it.
int crbm_train_epoch_sharded(crbm_handle* h, int32_t batchsize, int32_t total_rows, int32_t L) {
  ENTER();
  const int slot = h->slot;
  ARGCHK(batchsize >= 1 && total_rows >= 1, "batchsize and total_rows must be positive");
  // L comes from the caller, not from this rank's slot: a rank with an empty share has nothing resident,
  // and all ranks must divide the all-reduced sums by the same counts
  int rc = check_data_shape(h, 1, L);
  if (rc) return rc;
  const int LW = lw(h, L);
  long have = 0;
  for (int start = 0; start < total_rows; start += batchsize) {
    const long n = std::min(total_rows, start + batchsize) - start;
    have += (n * (h->rank + 1)) / h->nranks - (n * h->rank) / h->nranks;
  }
  ARGCHK(have == h->dataset_n[slot], "resident rows do not match this rank's share of total_rows");
  ARGCHK(have == 0 || h->dataset_L[slot] == L, "resident rows have another sequence length than L");
  ARGCHK(have > 0 || h->comm || h->ipc_on, "no resident data set (call crbm_dataset_upload)");
  size_t off = 0;
  for (int start = 0; start < total_rows; start += batchsize) {
    const long n = std::min(total_rows, start + batchsize) - start;
    const int mine = (int)((n * (h->rank + 1)) / h->nranks - (n * h->rank) / h->nranks);
    rc = train_core(h, h->dataset[slot].p + off * LW, mine, L);
    if (rc) return rc;
    off += (size_t)mine;
  }
  HIPCHK(hipStreamSynchronize(h->stream));
  return ipc_check(h);
}

int crbm_gibbs_steps_async(crbm_handle* h, int32_t k) {
  ENTER_ASYNC();
  ARGCHK(k >= 1, "k must be positive");
  return launch_gibbs(h, k, nullptr, nullptr, true);
}

int crbm_sync(crbm_handle* h) {
  ENTER();
  HIPCHK(hipStreamSynchronize(h->stream));
  int rc = ipc_check(h);
  if (rc) return rc;
  return refresh_activity(h);
}

// every launch of this handle has completed (no read-back of the activity monitor: crbm_sync does that too)
int crbm_wait_idle(crbm_handle* h) {
  ENTER();
  HIPCHK(hipStreamSynchronize(h->stream));
  return ipc_check(h);
}

int crbm_gibbs_steps(crbm_handle* h, int32_t k) {
  int rc = crbm_gibbs_steps_async(h, k);
  if (rc) return rc;
  return crbm_sync(h);
}

// waits for an event by polling it: the timed entry points return microseconds after their last launch has completed
// (a blocking wait wakes up tens of microseconds late, which a 20-launch benchmark run would see in its host clock)
static hipError_t spin_until(hipEvent_t ev) {
  for (long i = 0;; ++i) {
    const hipError_t e = hipEventQuery(ev);
    if (e != hipErrorNotReady) return e;
    if (i > 2000000) return hipEventSynchronize(ev);   // seconds have passed: nothing left to gain from polling, block like everybody else
  }
}

int crbm_time_gibbs(crbm_handle* h, int32_t k, int32_t launches, float* total_ms) {
  ENTER();
  ARGCHK(k >= 0 && launches >= 1 && total_ms, "bad argument");   // k = 0: state load/store only (profiling)
  // (the launches add their durations to d_probe; the sums before this call were read when the previous one ended:
  //  nothing touches the GPU here before the opening event)
  h->probe_base[0] = h->probe_last[0]; h->probe_base[1] = h->probe_last[1];
  h->probe_on = true;
  const bool want_timeline = env_int("CRBM_GIBBS_TIMELINE", 0) != 0 && launches <= 4096;
  if (want_timeline) {
    const int need = launches * std::max(1, h->plan.chain_parts);
    if (need > h->timeline_cap()) HIPCHK(h->d_timeline.alloc((size_t)need * 2));
    HIPCHK(hipMemset(h->d_timeline.p, 0, (size_t)h->timeline_cap() * 16));
    h->timeline_next = 0;
  } else h->timeline_next = h->timeline_cap();      // no slots handed out
  struct TimelineDump {
    crbm_handle* h; bool on;
    ~TimelineDump() {
      if (!on || !h->d_timeline.p) return;
      (void)hipDeviceSynchronize();
      std::vector<unsigned long long> t((size_t)h->timeline_next * 2);
      if (hipMemcpy(t.data(), h->d_timeline.p, t.size() * 8, hipMemcpyDeviceToHost) != hipSuccess || t.empty()) return;
      unsigned long long t0 = ~0ull;
      for (size_t i = 0; i < t.size(); i += 2) if (t[i]) t0 = std::min(t0, t[i]);
      const double us = 1000.0 / h->wall_khz;
      fprintf(stderr, "chain launches (block 0: start-end in us from the first start; %d partition(s), launch order):", h->plan.chain_parts);
      for (size_t i = 0; i < t.size(); i += 2) {
        if (i == 2 * 60 && t.size() > 2 * 120) { fprintf(stderr, " ..."); i = t.size() - 2 * 60; }
        fprintf(stderr, " %.1f-%.1f", (t[i] - t0) * us, (t[i + 1] - t0) * us);
      }
      fprintf(stderr, "\n");
      h->timeline_next = h->timeline_cap();
    }
  } timeline_dump{h, want_timeline};
  struct ProbeOff { crbm_handle* h; ~ProbeOff() { h->probe_on = false; } } probe_off{h};
  h->main_idle_hint = hipStreamQuery(h->stream) == hipSuccess;   // (the opening event below does not count as work to wait for)
  (void)hipGetLastError();
  HIPCHK(hipEventRecord(h->ev0, h->stream));
  const auto t_enq0 = std::chrono::steady_clock::now();
  const bool trace_enq = env_int("CRBM_TIME_ENQUEUE", 0) >= 2;
  std::vector<double> enq_us;
  for (int i = 0; i < launches; ++i) {
    int rc = launch_gibbs(h, k, nullptr, nullptr, true);
    if (rc) return rc;
    if (trace_enq) enq_us.push_back(std::chrono::duration<double, std::micro>(std::chrono::steady_clock::now() - t_enq0).count());
  }
  if (trace_enq) {
    fprintf(stderr, "enqueue completion times (us):");
    for (size_t i = 0; i < enq_us.size() && i < 60; ++i) fprintf(stderr, " %.0f", enq_us[i]);
    fprintf(stderr, "\n");
  }
  if (env_int("CRBM_TIME_ENQUEUE", 0))     // measurement aid: host time spent enqueuing the launches
    fprintf(stderr, "crbm_time_gibbs: %d launch steps enqueued in %.1f us of host time\n", launches,
            std::chrono::duration<double, std::micro>(std::chrono::steady_clock::now() - t_enq0).count());
  if (h->forked) {
    // partitioned launches: the interval ends when the last partition's last launch does -- an event behind each
    // partition's launches, polled by the host (no device-side join in the timed region; the streams stay forked)
    float worst = 0.f;
    {
      const int rc = drain_part_workers(h);
      if (rc) return rc;
    }
    HIPCHK(hipEventRecord(h->ev1, h->stream));                       // partition 0 = the main stream
    for (int p = 1; p < h->plan.chain_parts; ++p) HIPCHK(hipEventRecord(h->part[p].done, h->part[p].stream));
    HIPCHK(spin_until(h->ev1));
    HIPCHK(hipEventElapsedTime(&worst, h->ev0, h->ev1));
    for (int p = 1; p < h->plan.chain_parts; ++p) {
      float ms = 0.f;
      HIPCHK(spin_until(h->part[p].done));
      HIPCHK(hipEventElapsedTime(&ms, h->ev0, h->part[p].done));
      worst = std::max(worst, ms);
    }
    *total_ms = worst;
    return CRBM_OK;
  }
  h->main_idle_hint = false;
  HIPCHK(hipEventRecord(h->ev1, h->stream));
  HIPCHK(spin_until(h->ev1));
  HIPCHK(hipEventElapsedTime(total_ms, h->ev0, h->ev1));
  return CRBM_OK;
}

int crbm_time_train(crbm_handle* h, int32_t start, int32_t end, int32_t launches, float* total_ms) {
  ENTER();
  const int slot = h->slot;
  ARGCHK(h->dataset_n[slot] > 0, "no resident data set (call crbm_dataset_upload)");
  ARGCHK(start >= 0 && end > start && end <= h->dataset_n[slot] && launches >= 1 && total_ms, "bad argument");
  const int LW = lw(h, h->dataset_L[slot]);
  HIPCHK(hipEventRecord(h->ev0, h->stream));
  for (int i = 0; i < launches; ++i) {
    int rc = train_core(h, h->dataset[slot].p + (size_t)start * LW, end - start, h->dataset_L[slot]);
    if (rc) return rc;
  }
  HIPCHK(hipEventRecord(h->ev1, h->stream));
  HIPCHK(spin_until(h->ev1));
  HIPCHK(hipEventElapsedTime(total_ms, h->ev0, h->ev1));
  return ipc_check(h);
}

// ---- stand-alone passes ------------------------------------------------------
int crbm_h_given_v(crbm_handle* h, const float* v, int32_t n, int32_t L, int32_t flip, uint32_t rng_step,
                   float* act, float* prob, float* sample) {
  ENTER();
  ARGCHK(v, "null argument");
  int rc = check_data_shape(h, n, L);
  if (rc) return rc;
  const int Lh = L - h->M + 1;
  const size_t count = (size_t)n * h->K * Lh;
  rc = encode_now(h, host_onehot(v, n, L), 0, n);
  if (rc) return rc;
  if (act) HIPCHK(h->out_a.ensure(count));
  if (prob) HIPCHK(h->out_b.ensure(count));
  if (sample) HIPCHK(h->out_c.ensure(count));
  rc = launch_hgv(h, h->letters.p, n, L, flip ? 1 : 0, act ? h->out_a.p : nullptr, prob ? h->out_b.p : nullptr,
                  sample ? h->out_c.p : nullptr, nullptr, KIND_API_H, rng_step, h->chain_offset);
  if (rc) return rc;
  if (act && (rc = copy_out(h, act, h->out_a.p, count))) return rc;
  if (prob && (rc = copy_out(h, prob, h->out_b.p, count))) return rc;
  if (sample && (rc = copy_out(h, sample, h->out_c.p, count))) return rc;
  HIPCHK(hipStreamSynchronize(h->stream));
  return CRBM_OK;
}

int crbm_v_given_h(crbm_handle* h, const float* hid, const float* hid_prime, int32_t n, int32_t Lh,
                   uint32_t rng_step, float* act, float* prob, float* sample) {
  ENTER();
  ARGCHK(hid, "null argument");
  ARGCHK(n >= 1 && Lh >= 1, "bad shape");
  const int L = Lh + h->M - 1;
  ARGCHK((long)L * 4 < (1 << 20), "sequence too long");
  const size_t hcount = (size_t)n * h->K * Lh, vcount = (size_t)n * h->A * L;
  HIPCHK(h->stage.ensure(hcount));
  HIPCHK(hipMemcpyAsync(h->stage.p, hid, hcount * 4, hipMemcpyHostToDevice, h->stream));
  if (hid_prime) {
    HIPCHK(h->stage2.ensure(hcount));
    HIPCHK(hipMemcpyAsync(h->stage2.p, hid_prime, hcount * 4, hipMemcpyHostToDevice, h->stream));
  }
  if (act) HIPCHK(h->out_a.ensure(vcount));
  if (prob) HIPCHK(h->out_b.ensure(vcount));
  if (sample) HIPCHK(h->out_c.ensure(vcount));
  VghArgs a;
  a.W = h->dW.p; a.c = h->dc.p; a.K = h->K; a.M = h->M;
  a.hid = h->stage.p; a.hidp = hid_prime ? h->stage2.p : nullptr;
  a.n = n; a.Lh = Lh; a.L = L;
  a.TS = tile_seqs(L, 4096);
  a.divL = make_fastdiv((uint32_t)L);
  a.act = act ? h->out_a.p : nullptr; a.prob = prob ? h->out_b.p : nullptr; a.sample = sample ? h->out_c.p : nullptr;
  a.rng = rng_view(h, rng_step, h->chain_offset);
  a.kind = KIND_API_V;
  const int ntiles = (n + a.TS - 1) / a.TS;
  if (h->A == 4) {
    // (the filters pass through LDS a slab of motifs at a time: vgh_dense_ks, crbm_layout.h -- any accepted model fits)
    hipLaunchKernelGGL(vgh_dense_kernel, dim3(std::max(1, std::min(ntiles, h->num_cu * 8))), dim3(256),
                       vgh_dense_lds(4, h->K, h->M), h->stream, a);
  } else {      // any other alphabet: a position's activations of all letters in LDS, filters from global memory
    VghAnyArgs aa;
    aa.g = a; aa.A = h->A;
    hipLaunchKernelGGL(vgh_dense_any_kernel, dim3(grid_for((long)n * L, 256, h->num_cu * 8)), dim3(256), vgh_dense_lds(h->A, h->K, h->M), h->stream, aa);
  }
  HIPCHK(hipGetLastError());
  int rc;
  if (act && (rc = copy_out(h, act, h->out_a.p, vcount))) return rc;
  if (prob && (rc = copy_out(h, prob, h->out_b.p, vcount))) return rc;
  if (sample && (rc = copy_out(h, sample, h->out_c.p, vcount))) return rc;
  HIPCHK(hipStreamSynchronize(h->stream));
  return CRBM_OK;
}

// ---- evaluation --------------------------------------------------------------
// Every evaluation entry point exists in three forms: fp32 one-hot host input
// (the reference's layout), one byte per base host input (`_codes`), and rows of
// a data set already resident in HBM (`_resident`).  Host input is streamed in
// slabs so that the staged input plus the outputs of one slab stay around
// 256 MB (data sets far larger than the scratch: SURVEY 8(f)-1): slab_rows gives
// the slab, sweep_run walks the slabs.
namespace {

int resident_source(crbm_handle* h, int start, int end, RowSource* src) {
  const int slot = h->slot;
  ARGCHK(h->dataset_n[slot] > 0, "no resident data set (call crbm_dataset_upload)");
  ARGCHK(start >= 0 && end > start && end <= h->dataset_n[slot], "row range out of bounds");
  src->L = h->dataset_L[slot];
  src->n = end - start;
  src->resident = h->dataset[slot].p + (size_t)start * lw(h, src->L);
  return CRBM_OK;
}

int hit_probs_any(crbm_handle* h, const RowSource& src, float* out) {
  int rc = check_data_shape(h, src.n, src.L);
  if (rc) return rc;
  const int L = src.L, Lh = L - h->M + 1;
  const size_t per_seq_out = (size_t)h->K * Lh;
  const int slab = slab_rows(src.n, src.in_bytes_per_row() + per_seq_out * sizeof(float));
  HIPCHK(h->out_b.ensure((size_t)slab * per_seq_out));
  return sweep_run(h, src, slab, 1,
    [&](const SweepSet& set, const uint32_t* rows, int, int cnt) -> int {
      // convRBM.py:507-514: doublestranded -> sigma(x); single-stranded -> sigma(x + x')
      return launch_hgv(h, rows, cnt, L, h->ds ? 0 : 2, nullptr, set.ob->p, nullptr, nullptr, KIND_API_H, 0, 0);
    },
    [&](const SweepSet& set, const uint32_t*, int start, int cnt) -> int {
      HIPCHK(hipMemcpyAsync(out + (size_t)start * per_seq_out, set.ob->p, (size_t)cnt * per_seq_out * sizeof(float), hipMemcpyDeviceToHost, set.st));
      HIPCHK(hipStreamSynchronize(set.st));
      return CRBM_OK;
    });
}

// free energies of n packed rows into the set's outputs (per sequence / per motif), no copy
int launch_free_energy(crbm_handle* h, const uint32_t* rows, int n, int L, const SweepSet& set) {
  int rc = ensure_tables(h);   // no-op inside a two-stream sweep (sweep_begin has done it)
  if (rc) return rc;
  HIPCHK(set.oa->ensure((size_t)n));
  HIPCHK(set.ob->ensure((size_t)n * h->K));
  if (h->big()) return big_launch_eval(h, rows, n, L, 0, set.oa->p, set.ob->p, nullptr, nullptr, nullptr, set.fe_scratch, set.st);
  FeArgs a;
  a.tables = h->d_tables.p;
  a.letters = rows;
  a.n = n; a.L = L; a.Lh = L - h->M + 1; a.LW = lw(h, L);
  a.fe = set.oa->p; a.fem = set.ob->p;
  const unsigned gx = (unsigned)std::max(1, std::min((n + 3) / 4, h->num_cu * 8));
  HIPCHK(jit_launch(h->jk.free_energy, a, gx, 1, 256, (unsigned)tab_bytes(h->ms()), set.st));
  return CRBM_OK;
}

int free_energy_any(crbm_handle* h, const RowSource& src, float* fe, float* fem) {
  int rc = check_data_shape(h, src.n, src.L);
  if (rc) return rc;
  rc = sweep_begin(h);
  if (rc) return rc;
  const int K = h->K, slab = sweep_slab(src, ((size_t)K + 1) * sizeof(float));
  for (int i = 0; i < (slab < src.n ? 2 : 1); ++i) {        // everything both streams write, at its size, before either starts
    const SweepSet set = sweep_set(h, i);
    HIPCHK(set.oa->ensure((size_t)slab));
    HIPCHK(set.ob->ensure((size_t)slab * K));
    if (slab_fe_on(h)) HIPCHK(set.fe_scratch->ensure((size_t)slab * h->slab.K * h->slab_n));
  }
  return sweep_run(h, src, slab, 2,
    [&](const SweepSet& set, const uint32_t* rows, int, int cnt) -> int { return launch_free_energy(h, rows, cnt, src.L, set); },
    [&](const SweepSet& set, const uint32_t*, int start, int cnt) -> int {
      if (fe) HIPCHK(hipMemcpyAsync(fe + start, set.oa->p, (size_t)cnt * sizeof(float), hipMemcpyDeviceToHost, set.st));
      if (fem) HIPCHK(hipMemcpyAsync(fem + (size_t)start * K, set.ob->p, (size_t)cnt * K * sizeof(float), hipMemcpyDeviceToHost, set.st));
      HIPCHK(hipStreamSynchronize(set.st));
      return CRBM_OK;
    });
}

int eval_data_any(crbm_handle* h, const RowSource& src, float* mfe, float* nmh) {
  int rc = check_data_shape(h, src.n, src.L);
  if (rc) return rc;
  const int n = src.n, L = src.L;
  const int slab = slab_rows(n, src.in_bytes_per_row() + ((size_t)h->K + 1) * sizeof(float));
  std::vector<float> fe((size_t)slab);
  double tot = 0.0;
  HIPCHK(hipMemsetAsync(h->d_ones.p, 0, sizeof(unsigned long long), h->stream));
  rc = sweep_run(h, src, slab, 1,
    [&](const SweepSet& set, const uint32_t* rows, int start, int cnt) -> int {
      const int r = launch_free_energy(h, rows, cnt, L, set);
      // mean of a fresh forward-strand sample (convRBM.py:469-472); rows keep their index within the call
      return r ? r : launch_hgv(h, rows, cnt, L, 0, nullptr, nullptr, nullptr, h->d_ones.p, KIND_EVAL_H, h->eval_step, (uint32_t)start);
    },
    [&](const SweepSet& set, const uint32_t*, int, int cnt) -> int {
      HIPCHK(hipMemcpyAsync(fe.data(), set.oa->p, (size_t)cnt * sizeof(float), hipMemcpyDeviceToHost, set.st));
      HIPCHK(hipStreamSynchronize(set.st));
      for (int i = 0; i < cnt; ++i) tot += fe[i];
      return CRBM_OK;
    });
  if (rc) return rc;
  *mfe = (float)(tot / n);                       // convRBM.py:636-638
  h->eval_step += 1;
  unsigned long long ones = 0;
  HIPCHK(hipMemcpyAsync(&ones, h->d_ones.p, sizeof(ones), hipMemcpyDeviceToHost, h->stream));
  HIPCHK(hipStreamSynchronize(h->stream));
  *nmh = (float)((double)ones / ((double)n * h->K * (L - h->M + 1)));
  return CRBM_OK;
}

// max / mean over positions per (sequence, motif) and mean over sequences per (motif, position)
int hit_summary_any(crbm_handle* h, const RowSource& src, float* hmax, float* hmean, float* posmean) {
  int rc = check_data_shape(h, src.n, src.L);
  if (rc) return rc;
  const int n = src.n, L = src.L, Lh = L - h->M + 1, K = h->K;
  const int tabs = h->big() ? 0 : tab_bytes(h->ms());
  // a block covers one chunk of 64*HIT_NI positions; its (PC,K) sums share the LDS with the tables
  const int PC = 64 * h->ms().HIT_NI;
  const int nchunks = h->big() ? 1 : (Lh + PC - 1) / PC;           // (the big path's kernel takes a whole sequence per block)
  const unsigned lds = (unsigned)(tabs + (size_t)PC * K * 8);    // tables + the block's fixed-point position sums
  ARGCHK(h->big() || lds <= 160u * 1024u, "model too large for the hit-summary kernel");
  // sums over sequences per (motif, position): 64-bit fixed point (HIT_FX units), so that the order in which blocks,
  // slabs and the two streams add does not show in the result
  unsigned long long* pos_fx = nullptr;
  if (posmean) {
    HIPCHK(h->out_c.ensure((size_t)2 * K * Lh + 2));
    pos_fx = reinterpret_cast<unsigned long long*>(h->out_c.p);
    HIPCHK(hipMemsetAsync(pos_fx, 0, (size_t)K * Lh * 8, h->stream));
  }
  rc = sweep_begin(h);          // also orders the memset before both streams' kernels
  if (rc) return rc;
  const int slab = sweep_slab(src, (size_t)2 * K * sizeof(float));
  for (int i = 0; i < (slab < n ? 2 : 1); ++i) {        // everything both streams write, at its size, before either starts
    HIPCHK(sweep_set(h, i).oa->ensure((size_t)slab * K));
    HIPCHK(sweep_set(h, i).ob->ensure((size_t)slab * K * (nchunks > 1 ? 3 : 1)));
  }
  // layout of a set's `ob` when the positions come in several chunks: [cnt*K fixed-point sums][cnt*K means]
  auto mean_of = [&](const SweepSet& set, int cnt) { return nchunks > 1 ? set.ob->p + (size_t)2 * cnt * K : set.ob->p; };
  rc = sweep_run(h, src, slab, 2,
    [&](const SweepSet& set, const uint32_t* rows, int, int cnt) -> int {
      if (nchunks > 1) {
        HIPCHK(hipMemsetAsync(set.oa->p, 0, (size_t)cnt * K * 4, set.st));
        HIPCHK(hipMemsetAsync(set.ob->p, 0, (size_t)cnt * K * 8, set.st));
      }
      HitArgs a;
      a.tables = h->d_tables.p; a.letters = rows;
      a.n = cnt; a.L = L; a.Lh = Lh; a.LW = lw(h, L);
      a.hmax = hmax ? set.oa->p : nullptr;
      a.hsum = (hmean && nchunks == 1) ? set.ob->p : nullptr;
      a.hsum_fx = (hmean && nchunks > 1) ? reinterpret_cast<unsigned long long*>(set.ob->p) : nullptr;
      a.inv_Lh = 1.0f / (float)Lh;
      a.pos_fx = pos_fx;                          // both streams add (integers: any order)
      const unsigned gx = (unsigned)std::max(1, std::min((cnt + 3) / 4, std::max(1, h->num_cu * 8 / nchunks)));
      if (h->big()) {
        const int r = big_launch_eval(h, rows, cnt, L, 1, nullptr, nullptr, a.hmax, a.hsum, pos_fx, nullptr, set.st);
        if (r) return r;
      } else
      HIPCHK(jit_launch(h->jk.hit_summary, a, gx, (unsigned)nchunks, 256, lds, set.st));
      if (a.hsum_fx) {
        hipLaunchKernelGGL(hit_finalize_kernel, dim3(grid_for((long)cnt * K, 256, h->num_cu * 4)), dim3(256), 0, set.st, a.hsum_fx,
                           mean_of(set, cnt), (size_t)cnt * K, a.inv_Lh / HIT_FX);
        HIPCHK(hipGetLastError());
      }
      return CRBM_OK;
    },
    [&](const SweepSet& set, const uint32_t*, int start, int cnt) -> int {
      if (hmax) HIPCHK(hipMemcpyAsync(hmax + (size_t)start * K, set.oa->p, (size_t)cnt * K * sizeof(float), hipMemcpyDeviceToHost, set.st));
      if (hmean) HIPCHK(hipMemcpyAsync(hmean + (size_t)start * K, mean_of(set, cnt), (size_t)cnt * K * sizeof(float), hipMemcpyDeviceToHost, set.st));
      HIPCHK(hipStreamSynchronize(set.st));
      return CRBM_OK;
    });
  if (rc) return rc;
  if (posmean) {
    std::vector<unsigned long long> fx((size_t)K * Lh);
    HIPCHK(hipMemcpyAsync(fx.data(), pos_fx, fx.size() * 8, hipMemcpyDeviceToHost, h->stream));
    HIPCHK(hipStreamSynchronize(h->stream));
    const double inv = 1.0 / ((double)n * (double)HIT_FX);
    for (size_t i = 0; i < fx.size(); ++i) posmean[i] = (float)((double)fx[i] * inv);
  }
  return CRBM_OK;
}

// ---- motif sites (crbm_motif_sites*) ------------------------------------------------------------------------------
static_assert(sizeof(SiteRec) == sizeof(crbm_site) && sizeof(crbm_site) == 20, "crbm_site is the kernels' SiteRec");

// records of one slab (seq within the slab) -> sorted by (seq, motif, start, strand), + before -: a counting pass over
// the rows, then a sort of each row's few records
void sort_sites(const std::vector<SiteRec>& in, int nrows, std::vector<SiteRec>* out) {
  std::vector<size_t> first((size_t)nrows + 1, 0);
  for (const SiteRec& r : in) ++first[(size_t)r.seq + 1];
  for (int i = 0; i < nrows; ++i) first[i + 1] += first[i];
  out->resize(in.size());
  std::vector<size_t> at(first.begin(), first.end() - 1);
  for (const SiteRec& r : in) (*out)[at[r.seq]++] = r;
  auto before = [](const SiteRec& a, const SiteRec& b) {
    if (a.motif != b.motif) return a.motif < b.motif;
    if (a.start != b.start) return a.start < b.start;
    return (a.strand < 0 ? 1 : 0) < (b.strand < 0 ? 1 : 0);
  };
  for (int i = 0; i < nrows; ++i)
    if (first[i + 1] - first[i] > 1) std::sort(out->begin() + first[i], out->begin() + first[i + 1], before);
}

// Thresholded sites and best sites over a source, a two-stream sweep.  Specialised models: the fused crbm_motif_sites
// pass (motif_sites_body).  Generic models (h->big()): the dense h|v of hit_probs_any into the set's outputs (oa: the
// forward strand, or sigma(x + x') single-stranded; ob: the reverse-complemented filter), then motif_sites_select_kernel.
// Every set owns its records, counter and keys (sized before the sweep); a slab whose count exceeds its set's record
// buffer is run again into a larger one before anything is copied (its rows are still in the set's buffers: the set is
// next used by the slab after the one enqueued before this collect).
int motif_sites_any(crbm_handle* h, const RowSource& src, float threshold, int64_t capacity, crbm_site* sites,
                    int64_t* count, int32_t* best_start, int32_t* best_strand, float* best_prob) {
  ARGCHK(threshold >= 0.f && threshold <= 1.f, "threshold must lie in [0, 1]");   // (NaN fails both)
  ARGCHK(capacity >= 0, "capacity must be >= 0");
  ARGCHK(!sites || count, "count is required with sites");
  const bool want_recs = sites != nullptr, want_best = best_start || best_strand || best_prob;
  ARGCHK(want_recs || want_best, "null argument");
  int rc = check_data_shape(h, src.n, src.L);
  if (rc) return rc;
  const int n = src.n, L = src.L, Lh = L - h->M + 1, K = h->K, S = h->ds ? 2 : 1;
  const int PC = 64 * h->ms().HIT_NI;
  const int nchunks = h->big() ? 1 : (Lh + PC - 1) / PC;
  const unsigned lds = h->big() ? 0u : (unsigned)tab_bytes(h->ms());
  ARGCHK(h->big() || lds <= 160u * 1024u, "model too large for the motif-site kernel");
  rc = sweep_begin(h);
  if (rc) return rc;
  const size_t dense_per_row = h->big() ? (size_t)S * K * Lh * sizeof(float) : 0;
  const int slab = sweep_slab(src, (size_t)K * 8 + dense_per_row);
  const size_t rec0 = std::min((size_t)slab * K * S * Lh, std::max<size_t>((size_t)1 << 16, (size_t)4 * slab * K));
  for (int i = 0; i < (slab < n ? 2 : 1); ++i) {        // everything both streams write, at its size, before either starts
    const SweepSet set = sweep_set(h, i);
    if (want_recs) {
      HIPCHK(set.own->site_recs.ensure(rec0));
      HIPCHK(set.own->site_count.ensure(1));
    }
    if (want_best) HIPCHK(set.own->site_keys.ensure((size_t)slab * K));
    if (h->big()) {
      HIPCHK(set.oa->ensure((size_t)slab * K * Lh));
      if (S == 2) HIPCHK(set.ob->ensure((size_t)slab * K * Lh));
    }
  }
  auto launch = [&](const SweepSet& set, const uint32_t* rows, int, int cnt) -> int {
    SitesOut o;
    o.recs = want_recs ? set.own->site_recs.p : nullptr;
    o.capacity = want_recs ? set.own->site_recs.cap : 0;
    o.count = want_recs ? set.own->site_count.p : nullptr;
    o.best = want_best ? set.own->site_keys.p : nullptr;
    o.threshold = threshold;
    if (want_recs) HIPCHK(hipMemsetAsync(o.count, 0, sizeof(unsigned long long), set.st));
    if (h->big()) {
      // convRBM.py:507-514 as hit_probs_any: doublestranded -> sigma(x) (and the flipped filter), else sigma(x + x')
      int r = big_launch_hgv(h, rows, cnt, L, h->ds ? 0 : 2, nullptr, set.oa->p, nullptr, nullptr, nullptr, KIND_API_H, 0, 0, set.st);
      if (!r && S == 2) r = big_launch_hgv(h, rows, cnt, L, 1, nullptr, set.ob->p, nullptr, nullptr, nullptr, KIND_API_H, 0, 0, set.st);
      if (r) return r;
      SitesSelectArgs a;
      a.p0 = set.oa->p; a.p1 = S == 2 ? set.ob->p : nullptr;
      a.n = cnt; a.K = K; a.Lh = Lh; a.ds = h->ds;
      a.o = o;
      hipLaunchKernelGGL(motif_sites_select_kernel, dim3(grid_for((long)cnt * K, 4, h->num_cu * 8)), dim3(256), 0, set.st, a);
      HIPCHK(hipGetLastError());
      return CRBM_OK;
    }
    if (want_best && nchunks > 1) HIPCHK(hipMemsetAsync(o.best, 0, (size_t)cnt * K * 8, set.st));   // (atomicMax across chunks)
    SitesArgs a;
    a.tables = h->d_tables.p; a.letters = rows;
    a.n = cnt; a.L = L; a.Lh = Lh; a.LW = lw(h, L);
    a.o = o;
    const unsigned gx = (unsigned)std::max(1, std::min((cnt + 3) / 4, std::max(1, h->num_cu * 8 / nchunks)));
    HIPCHK(jit_launch(h->jk.motif_sites, a, gx, (unsigned)nchunks, 256, lds, set.st));
    return CRBM_OK;
  };
  int64_t total = 0;
  std::vector<SiteRec> raw, sorted;
  std::vector<unsigned long long> keys;
  auto collect = [&](const SweepSet& set, const uint32_t* rows, int start, int cnt) -> int {
    if (want_best) {
      keys.resize((size_t)cnt * K);
      HIPCHK(hipMemcpyAsync(keys.data(), set.own->site_keys.p, keys.size() * 8, hipMemcpyDeviceToHost, set.st));
    }
    unsigned long long c = 0;
    if (want_recs) HIPCHK(hipMemcpyAsync(&c, set.own->site_count.p, sizeof(c), hipMemcpyDeviceToHost, set.st));
    HIPCHK(hipStreamSynchronize(set.st));
    if (want_recs && total < capacity) {
      if (c > set.own->site_recs.cap) {       // more records than the set's buffer took: again, into one that takes them
        HIPCHK(set.own->site_recs.ensure((size_t)c));
        const int r = launch(set, rows, start, cnt);
        if (r) return r;
        HIPCHK(hipStreamSynchronize(set.st));
      }
      raw.resize((size_t)c);
      HIPCHK(hipMemcpyAsync(raw.data(), set.own->site_recs.p, (size_t)c * sizeof(SiteRec), hipMemcpyDeviceToHost, set.st));
      HIPCHK(hipStreamSynchronize(set.st));
      sort_sites(raw, cnt, &sorted);
      const size_t keep = (size_t)std::min<int64_t>((int64_t)c, capacity - total);
      for (size_t r = 0; r < keep; ++r) {
        const SiteRec& x = sorted[r];
        sites[total + (int64_t)r] = crbm_site{x.seq + start, x.motif, x.start, x.strand, x.prob};
      }
    }
    total += (int64_t)c;
    if (want_best) {
      for (size_t r = 0; r < keys.size(); ++r) {
        const size_t o = (size_t)start * K + r;
        const uint32_t code = 0xFFFFFFFFu - (uint32_t)keys[r];
        float p;
        const uint32_t bits = (uint32_t)(keys[r] >> 32);
        std::memcpy(&p, &bits, 4);
        if (best_start) best_start[o] = (int32_t)(code >> 1);
        if (best_strand) best_strand[o] = h->ds ? ((code & 1u) ? -1 : 1) : 0;
        if (best_prob) best_prob[o] = p;
      }
    }
    return CRBM_OK;
  };
  rc = sweep_run(h, src, slab, 2, launch, collect);
  if (rc) return rc;
  if (count) *count = want_recs ? total : 0;
  return CRBM_OK;
}

// ---- stream scan (crbm_scan_sites_codes) ---------------------------------------------------------------------------
// The sites of a stream, a StreamSweep.  Per segment: crbm_scan_sites counts (pass 0), scan_offsets_kernel scans the
// tile counts, crbm_scan_sites writes the records at their offsets (pass 1) -- in final order, so that a model on its
// own kernels is copied straight into the caller's array.  Every slab of a generic DNA model has its own counts,
// offsets and records; the slabs' runs, each sorted by start and owning ascending motifs, are merged on the host by
// (start, slab).  Every set owns what it writes, sized for a whole segment before the sweep starts; only the records
// may have to grow, as in motif_sites_any: pass 1 is then run again before anything is copied.  Since records are in
// final order, a segment needs no more room than what the caller's capacity still takes.
int scan_sites_any(crbm_handle* h, const uint8_t* codes, int64_t T, float threshold, int64_t capacity, crbm_site* sites,
                   int64_t* count) {
  ARGCHK(count, "null argument");
  ARGCHK(threshold >= 0.f && threshold <= 1.f, "threshold must lie in [0, 1]");   // (NaN fails both)
  ARGCHK(capacity >= 0, "capacity must be >= 0");
  ARGCHK(sites || capacity == 0, "sites is required with a capacity");
  StreamSweep sw{h, "crbm_scan_sites_codes"};
  int rc = sw.admit(codes, T);
  if (rc) return rc;
  *count = 0;
  if (T < sw.M) return CRBM_OK;
  rc = sw.begin(T);
  if (rc) return rc;
  const int nslab = sw.nslab, seg = sw.plan.seg, full_tiles = sw.plan.full.tiles;
  const bool want_recs = capacity > 0;
  size_t rcap[2] = {0, 0};                               // records per slab a set's buffer is used for
  for (int i = 0; i < sw.plan.nsets; ++i) {              // everything both streams write, at its size, before either starts
    const SweepSet set = sweep_set(h, i);
    HIPCHK(set.own->scan_lanes.ensure((size_t)nslab * 64 * full_tiles));
    HIPCHK(set.own->scan_tiles.ensure((size_t)nslab * full_tiles));
    HIPCHK(set.own->scan_off.ensure((size_t)nslab * full_tiles + nslab));
    if (want_recs) {
      rcap[i] = (size_t)std::min<unsigned long long>({(unsigned long long)capacity, (unsigned long long)seg * sw.kms->K * sw.S,
                                                     std::max<unsigned long long>(1ull << 16, (unsigned long long)seg / 4)});
      HIPCHK(set.own->site_recs.ensure(rcap[i] * nslab));
    }
  }
  auto launch_pass = [&](const SweepSet& set, int si, const ScanInput& in, int start, int pass) -> int {
    ScanArgs a{in};
    a.lane_cnt = set.own->scan_lanes.p; a.tile_cnt = set.own->scan_tiles.p; a.tile_off = set.own->scan_off.p;
    a.recs = set.own->site_recs.p; a.capacity = rcap[si];
    a.pos0 = start; a.pass = pass; a.threshold = threshold; a.pad_ = 0;
    const unsigned gx = (unsigned)std::max(1, std::min((in.tiles + 3) / 4, std::max(1, h->num_cu * 8 / nslab)));
    HIPCHK(jit_launch(sw.kjk->scan_sites, a, gx, (unsigned)nslab, 256, (unsigned)tab_bytes(*sw.kms), set.st));
    return CRBM_OK;
  };
  int64_t total = 0;
  bool wrote[2] = {false, false};                        // the set's segment went through pass 1
  std::vector<unsigned long long> tot((size_t)nslab);
  std::vector<std::vector<SiteRec>> runs((size_t)(nslab > 1 ? nslab : 0));
  // CRBM_SCAN_TIMING=1: tools/bench_scan.py
  rc = sw.run(codes, "CRBM_SCAN_TIMING",
    [&](const SweepSet& set, int si, const ScanInput& in, int start, int) -> int {
      int r = launch_pass(set, si, in, start, 0);
      if (r) return r;
      ScanOffsetsArgs o;
      o.tile_cnt = set.own->scan_tiles.p; o.tile_off = set.own->scan_off.p;
      o.total = set.own->scan_off.p + (size_t)nslab * in.tiles; o.tiles = in.tiles;
      hipLaunchKernelGGL(scan_offsets_kernel, dim3(nslab), dim3(1024), 1024 * sizeof(unsigned long long), set.st, o);
      HIPCHK(hipGetLastError());
      wrote[si] = want_recs && total < capacity;         // (`total` lags by one segment and only grows: never skipped wrongly)
      return wrote[si] ? launch_pass(set, si, in, start, 1) : CRBM_OK;
    },
    [&](const SweepSet& set, int si, const ScanInput& in, int start, int) -> int {
      HIPCHK(hipMemcpyAsync(tot.data(), set.own->scan_off.p + (size_t)nslab * in.tiles, (size_t)nslab * 8, hipMemcpyDeviceToHost, set.st));
      HIPCHK(hipStreamSynchronize(set.st));
      unsigned long long c = 0, most = 0;
      for (int y = 0; y < nslab; ++y) c += tot[y];
      if (wrote[si] && total < capacity && c > 0) {
        const unsigned long long keep = std::min<unsigned long long>(c, (unsigned long long)(capacity - total));
        for (int y = 0; y < nslab; ++y) most = std::max(most, std::min(tot[y], keep));
        if (most > rcap[si]) {        // more records than the set's buffer took: pass 1 again, into one that takes them
          HIPCHK(set.own->site_recs.ensure((size_t)most * nslab));
          rcap[si] = (size_t)most;
          const int r = launch_pass(set, si, in, start, 1);
          if (r) return r;
        }
        if (nslab == 1) {
          HIPCHK(hipMemcpyAsync(sites + total, set.own->site_recs.p, (size_t)keep * sizeof(SiteRec), hipMemcpyDeviceToHost, set.st));
          HIPCHK(hipStreamSynchronize(set.st));
        } else {
          for (int y = 0; y < nslab; ++y) {
            runs[y].resize((size_t)std::min(tot[y], keep));
            if (!runs[y].empty())
              HIPCHK(hipMemcpyAsync(runs[y].data(), set.own->site_recs.p + (size_t)y * rcap[si], runs[y].size() * sizeof(SiteRec), hipMemcpyDeviceToHost, set.st));
          }
          HIPCHK(hipStreamSynchronize(set.st));
          std::vector<size_t> at((size_t)nslab, 0);
          for (unsigned long long r = 0; r < keep; ++r) {       // the smallest start, then the lowest slab: (start, motif, strand)
            int best = -1;
            for (int y = 0; y < nslab; ++y)
              if (at[y] < runs[y].size() && (best < 0 || runs[y][at[y]].start < runs[best][at[best]].start)) best = y;
            const SiteRec& x = runs[best][at[best]++];
            sites[total + (int64_t)r] = crbm_site{x.seq, x.motif, x.start, x.strand, x.prob};
          }
        }
      }
      total += (int64_t)c;
      return CRBM_OK;
    });
  if (rc) return rc;
  *count = total;
  return CRBM_OK;
}

// ---- score histogram (crbm_scan_histogram_codes) --------------------------------------------------------------------
// A StreamSweep with one launch per segment: crbm_scan_hist adds the segment's scores into h->hist.  The histogram is
// zeroed on the main stream, which is then waited for, before the first segment; both streams add into it with
// integer atomics; it is copied back once, after both streams are idle.  A segment has nothing to collect.
// CRBM_HIST_VARIANT picks how a wave spreads its LDS adds (scan_hist_body: 0 in order, 1 lane-rotated motif order,
// 2 counter sets per wave); CRBM_HIST_TIMING=1: tools/bench_calibrate.py.
int scan_hist_any(crbm_handle* h, const uint8_t* codes, int64_t T, float lo, float hi, int32_t nbins, uint64_t* counts,
                  int64_t* windows) {
  ARGCHK(counts, "null argument");
  ARGCHK(nbins >= 1 && nbins <= 1024, "nbins must lie in [1, 1024]");
  ARGCHK(std::isfinite(lo) && std::isfinite(hi) && lo < hi, "lo and hi must be finite with lo < hi");
  StreamSweep sw{h, "crbm_scan_histogram_codes"};
  int rc = sw.admit(codes, T);
  if (rc) return rc;
  const int nslab = sw.nslab;
  const int variant = env_int("CRBM_HIST_VARIANT", 1);
  const HistPlan hp = hist_plan(tab_bytes(*sw.kms), sw.kms->NQ, sw.S, nbins, variant == 2 ? 8 : 1);
  ARGCHK(hp.gq >= 1, "crbm_scan_histogram_codes: the counters of four motifs do not fit beside the model's gather table (fewer bins)");
  const float inv_w = (float)nbins / (hi - lo);
  ARGCHK(std::isfinite(inv_w) && inv_w > 0.f, "hi - lo is too small or too large for nbins");
  const size_t cells = (size_t)h->K * sw.S * nbins;
  if (T < sw.M) {
    std::memset(counts, 0, cells * sizeof(uint64_t));
    if (windows) *windows = 0;
    return CRBM_OK;
  }
  rc = sw.begin(T);
  if (rc) return rc;
  HIPCHK(h->hist.ensure(cells + 1));
  HIPCHK(hipMemsetAsync(h->hist.p, 0, (cells + 1) * sizeof(unsigned long long), h->stream));
  HIPCHK(hipStreamSynchronize(h->stream));                 // zero before either stream adds
  rc = sw.run(codes, "CRBM_HIST_TIMING",
    [&](const SweepSet& set, int, const ScanInput& in, int, int) -> int {
      ScanHistArgs a{in};
      a.hist = h->hist.p;
      a.nbins = nbins; a.gq = hp.gq; a.copies = hp.copies; a.rotate = variant == 1;
      a.lo = lo; a.inv_w = inv_w;
      // eight waves a block; as many blocks as the CUs hold at this LDS footprint, each with at least two tiles a wave
      const int per_cu = (int)std::max<long>(1, std::min<long>(4, 160L * 1024 / hp.lds));
      const unsigned gx = (unsigned)std::max(1, std::min((in.tiles + 15) / 16, std::max(1, h->num_cu * per_cu / nslab)));
      HIPCHK(jit_launch(sw.kjk->scan_hist, a, gx, (unsigned)nslab, 512, (unsigned)hp.lds, set.st));
      return CRBM_OK;
    },
    [](const SweepSet&, int, const ScanInput&, int, int) -> int { return CRBM_OK; });
  if (rc) return rc;
  std::vector<unsigned long long> out(cells + 1);
  HIPCHK(hipMemcpyAsync(out.data(), h->hist.p, (cells + 1) * sizeof(unsigned long long), hipMemcpyDeviceToHost, h->stream));
  HIPCHK(hipStreamSynchronize(h->stream));
  for (size_t i = 0; i < cells; ++i) counts[i] = (uint64_t)out[i];
  if (windows) *windows = (int64_t)out[cells];
  return CRBM_OK;
}

// ---- record summaries (crbm_scan_records_codes) ---------------------------------------------------------------------
// A StreamSweep with one launch per segment, like the histogram: crbm_scan_records adds the segment's windows and
// letters into the call's accumulators (h->rec_acc: sums, keys, counts), zeroed on the main stream before the first
// segment and copied back once after both streams are idle; records_finish (crbm_sweep.h) makes the outputs of them.
// Everything that can be refused on the host is refused before anything is launched.  A stream shorter than a motif
// has no window: its letters are counted on the host.  CRBM_RECORDS_TIMING=1: tools/bench_records.py.
int scan_records_any(crbm_handle* h, const uint8_t* codes, int64_t T, const int64_t* rec_start, int64_t nrec, int64_t* windows,
                     int64_t* letters, float* fe, float* fe_per_motif, int32_t* best_start, int32_t* best_strand, float* best_prob,
                     double* unit) {
  StreamSweep sw{h, "crbm_scan_records_codes"};
  int rc = sw.admit(codes, T);
  if (rc) return rc;
  ARGCHK(rec_start, "null argument");
  ARGCHK(nrec >= 0 && nrec <= (int64_t)INT32_MAX, "nrec must lie in [0, 2^31 - 1]");
  ARGCHK(nrec > 0 || T == 0, "crbm_scan_records_codes: no records, but letters");
  if (nrec > 0) {
    const char* bad = records_check(codes, T, rec_start, nrec);
    ARGCHK(!bad, std::string("crbm_scan_records_codes: ") + (bad ? bad : ""));
  }
  const int K = h->K, M = sw.M;
  rc = sweep_begin(h);                   // (the parameters are at rest)
  if (rc) return rc;
  std::vector<float> W((size_t)K * 4 * M), b((size_t)K);
  float c[4];
  HIPCHK(hipMemcpyAsync(W.data(), h->dW.p, W.size() * sizeof(float), hipMemcpyDeviceToHost, h->stream));
  HIPCHK(hipMemcpyAsync(b.data(), h->db.p, b.size() * sizeof(float), hipMemcpyDeviceToHost, h->stream));
  HIPCHK(hipMemcpyAsync(c, h->dc.p, sizeof(c), hipMemcpyDeviceToHost, h->stream));
  HIPCHK(hipStreamSynchronize(h->stream));
  const int e = records_unit_exp(records_x_max(W.data(), b.data(), K, M), sw.S);
  if (unit) *unit = records_unit(e);
  if (nrec == 0) return CRBM_OK;
  const bool want_counts = windows || letters || fe, want_fe = fe || fe_per_motif, want_best = best_start || best_strand || best_prob;
  ARGCHK(want_counts || want_fe || want_best, "null argument: at least one output is required");
  const size_t cells = (size_t)nrec * K;
  const size_t off_keys = want_fe ? cells : 0, off_counts = off_keys + (want_best ? cells : 0);
  const size_t words = off_counts + (want_counts ? (size_t)nrec * 5 : 0);
  std::vector<unsigned long long> acc(words, 0ull);
  if (T < M) {                           // no window anywhere
    rc = check_stream_codes(h, codes, T);
    if (rc) return rc;
    if (want_counts)
      for (int64_t r = 0; r < nrec; ++r)
        for (int64_t i = rec_start[r]; i < rec_start[r + 1] - 1; ++i)
          if (codes[i] < 4) ++acc[off_counts + 5 * (size_t)r + 1 + codes[i]];
  } else {
    rc = sw.begin(T);
    if (rc) return rc;
    static_assert(sizeof(long long) == sizeof(int64_t), "rec_start goes up as it is");
    HIPCHK(h->rec_acc.ensure(words));
    HIPCHK(h->rec_start.ensure((size_t)nrec + 1));
    HIPCHK(hipMemsetAsync(h->rec_acc.p, 0, words * sizeof(unsigned long long), h->stream));
    HIPCHK(hipMemcpyAsync(h->rec_start.p, rec_start, ((size_t)nrec + 1) * sizeof(int64_t), hipMemcpyHostToDevice, h->stream));
    HIPCHK(hipStreamSynchronize(h->stream));               // zeroed and in place before either stream adds
    const int nslab = sw.nslab, starts_all = sw.plan.starts_all;
    rc = sw.run(codes, "CRBM_RECORDS_TIMING",
      [&](const SweepSet& set, int, const ScanInput& in, int start, int cnt) -> int {
        ScanRecordsArgs a{in};
        a.rec_start = h->rec_start.p;
        a.sums = want_fe ? h->rec_acc.p : nullptr;
        a.best = want_best ? h->rec_acc.p + off_keys : nullptr;
        a.counts = want_counts ? h->rec_acc.p + off_counts : nullptr;
        a.pos0 = start; a.nrec = (int32_t)nrec;
        a.own = start + cnt == starts_all ? cnt + M - 1 : cnt;   // the last segment counts the letters behind its starts
        a.scale = ldexpf(1.f, e); a.pad_ = 0;
        // four waves a block, two blocks a CU: a wave's run is long (32 tiles of a 4M-start segment on 256 CUs), because a
        // run ends in a flush, and the flushes of one long record all meet on the same K addresses
        const int tiles = (a.own + 63) / 64;
        const unsigned gx = (unsigned)std::max(1, std::min((tiles + 31) / 32, std::max(1, h->num_cu * 2 / nslab)));
        HIPCHK(jit_launch(sw.kjk->scan_records, a, gx, (unsigned)nslab, 256, (unsigned)tab_bytes(*sw.kms), set.st));
        return CRBM_OK;
      },
      [](const SweepSet&, int, const ScanInput&, int, int) -> int { return CRBM_OK; });
    if (rc) return rc;
    HIPCHK(hipMemcpyAsync(acc.data(), h->rec_acc.p, words * sizeof(unsigned long long), hipMemcpyDeviceToHost, h->stream));
    HIPCHK(hipStreamSynchronize(h->stream));
  }
  records_finish(nrec, K, h->ds, e, c, want_fe ? acc.data() : nullptr, want_best ? acc.data() + off_keys : nullptr,
                 want_counts ? acc.data() + off_counts : nullptr, windows, letters, fe, fe_per_motif, best_start, best_strand, best_prob);
  return CRBM_OK;
}

// ---- variant effects (crbm_variant_effects_codes) -------------------------------------------------------------------
// A StreamSweep whose chunks are variants (crbm_sweep.h, variant_plan).  Everything that can be refused is refused on
// the host before anything is launched: outputs are then left as they were.  A chunk's stage gathers the contexts
// (crbm_sweep.h, gather_contexts) and the alt bytes into the set's host buffer, which the sweep copies up and encodes;
// crbm_variant_effects leaves per_motif [cnt][K] (set.oa) and the valid windows, variant_combine_kernel forms dfe
// (set.ob); the outputs asked for are copied straight into the caller's arrays at the chunk's offset.  Every set owns
// what it writes, sized for a whole chunk before the sweep starts.  CRBM_VARIANT_TIMING=1: tools/bench_variants.py.
int variant_effects_any(crbm_handle* h, const uint8_t* codes, int64_t T, int64_t nvar, const int64_t* pos, const uint8_t* alt,
                        float* dfe, float* per_motif, int32_t* windows) {
  StreamSweep sw{h, "crbm_variant_effects_codes"};
  int rc = sw.admit(codes, T);
  if (rc) return rc;
  ARGCHK(dfe || per_motif || windows, "null argument: at least one output is required");
  ARGCHK(nvar >= 0 && nvar <= (int64_t)INT32_MAX, "nvar must lie in [0, 2^31 - 1]");
  if (nvar == 0) return CRBM_OK;
  ARGCHK(pos && alt, "null argument");
  rc = check_stream_codes(h, codes, T);
  if (rc) return rc;
  {
    unsigned bad = 0;
    for (int64_t i = 0; i < nvar; ++i) bad |= (pos[i] < 0 || pos[i] >= T ? 1u : 0u) | (alt[i] > 3 ? 2u : 0u);
    ARGCHK(!(bad & 1u), "crbm_variant_effects_codes: every pos must lie in [0, T)");
    ARGCHK(!(bad & 2u), "crbm_variant_effects_codes: every alt must be a letter code 0..3");
  }
  rc = sweep_begin(h);
  if (rc) return rc;
  const int M = sw.M, K = h->K, nslab = sw.nslab;
  const SlabBudget budget = slab_budget();
  const VariantPlan vp = variant_plan((long)nvar, M, K, budget.bytes, budget.was_set);
  const int CW = vp.CW;
  auto ctx_bytes = [&](int cnt) { return ((size_t)cnt * CW + 3) & ~(size_t)3; };   // the alt bytes follow the contexts
  std::vector<uint8_t> host[2];
  for (int i = 0; i < vp.nsets; ++i) host[i].resize(ctx_bytes(vp.chunk) + (size_t)vp.chunk);
  rc = sw.size_inputs(vp.nsets, host[0].size(), vp.full);
  if (rc) return rc;
  for (int i = 0; i < vp.nsets; ++i) {                     // what both streams write, at its size, before either starts
    const SweepSet set = sweep_set(h, i);
    HIPCHK(set.oa->ensure((size_t)vp.chunk * K));
    HIPCHK(set.ob->ensure((size_t)vp.chunk));
    HIPCHK(set.own->var_windows.ensure((size_t)vp.chunk));
  }
  return sw.run_chunks((int)nvar, vp.chunk, "CRBM_VARIANT_TIMING", "chunks",
    [&](int si, StreamSweep::Chunk& c) -> int {
      uint8_t* ctx = host[si].data();
      gather_contexts(codes, T, pos + c.start, c.cnt, M, ctx);
      std::memcpy(ctx + ctx_bytes(c.cnt), alt + c.start, (size_t)c.cnt);
      c.bytes = ctx; c.up = ctx_bytes(c.cnt) + (size_t)c.cnt;
      c.n = (long)c.cnt * CW; c.layout_starts = c.cnt; c.starts = (int32_t)(c.n - M + 1);
      return CRBM_OK;
    },
    [&](const SweepSet& set, int, const ScanInput& in, int, int cnt) -> int {
      const unsigned char* staged = reinterpret_cast<const unsigned char*>(set.stage->p);
      VariantArgs a{in};
      a.alt = staged + ctx_bytes(cnt);
      a.per_motif = set.oa->p; a.windows = set.own->var_windows.p;
      a.cnt = cnt; a.pad_ = 0;
      const unsigned gx = (unsigned)std::max(1, std::min((in.tiles + 3) / 4, std::max(1, h->num_cu * 8 / nslab)));
      HIPCHK(jit_launch(sw.kjk->variant_effects, a, gx, (unsigned)nslab, 256, (unsigned)tab_bytes(*sw.kms), set.st));
      if (dfe) {
        VariantCombineArgs c;
        c.per_motif = set.oa->p; c.codes = staged; c.alt = a.alt; c.c = h->dc.p; c.dfe = set.ob->p;
        c.cnt = cnt; c.K = K; c.CW = CW; c.M = M;
        hipLaunchKernelGGL(variant_combine_kernel, dim3(grid_for(cnt, 256, h->num_cu * 8)), dim3(256), 0, set.st, c);
        HIPCHK(hipGetLastError());
      }
      return CRBM_OK;
    },
    [&](const SweepSet& set, int, const ScanInput&, int start, int cnt) -> int {
      const size_t at = (size_t)start;
      if (dfe) HIPCHK(hipMemcpyAsync(dfe + at, set.ob->p, (size_t)cnt * sizeof(float), hipMemcpyDeviceToHost, set.st));
      if (per_motif) HIPCHK(hipMemcpyAsync(per_motif + at * K, set.oa->p, (size_t)cnt * K * sizeof(float), hipMemcpyDeviceToHost, set.st));
      if (windows) HIPCHK(hipMemcpyAsync(windows + at, set.own->var_windows.p, (size_t)cnt * sizeof(int32_t), hipMemcpyDeviceToHost, set.st));
      return CRBM_OK;
    });
}

// ---- allele effects (crbm_allele_effects_codes) ---------------------------------------------------------------------
// variant_effects_any for alleles of any length: a StreamSweep over the chunks of allele_plan (crbm_sweep.h), which hold
// different numbers of variants -- the sweep walks the chunks one at a time and the stage names each chunk's variants.
// Everything that can be refused is refused on the host before anything is launched.  A chunk's stage gathers both
// haplotypes of every variant and their table entries (gather_haplotypes) into the set's host buffer, which the sweep
// copies up and encodes; crbm_allele_effects leaves per_motif [cnt][K] (set.oa) and the valid windows [cnt][2],
// allele_combine_kernel forms dfe (set.ob); the outputs asked for are copied straight into the caller's arrays.  Every
// set owns what it writes, sized for the largest chunk before the sweep starts.
// CRBM_ALLELE_TIMING=1: tools/bench_alleles.py.
int allele_effects_any(crbm_handle* h, const uint8_t* codes, int64_t T, int64_t nvar, const int64_t* pos, const int32_t* ref_len,
                       const int64_t* alt_off, const uint8_t* alt_codes, float* dfe, float* per_motif, int32_t* windows) {
  StreamSweep sw{h, "crbm_allele_effects_codes"};
  int rc = sw.admit(codes, T);
  if (rc) return rc;
  ARGCHK(dfe || per_motif || windows, "null argument: at least one output is required");
  ARGCHK(nvar >= 0 && nvar <= (int64_t)INT32_MAX, "nvar must lie in [0, 2^31 - 1]");
  if (nvar == 0) return CRBM_OK;
  ARGCHK(pos && ref_len && alt_off, "null argument");
  rc = check_stream_codes(h, codes, T);
  if (rc) return rc;
  {
    unsigned bad = 0;
    ARGCHK(alt_off[0] == 0, "crbm_allele_effects_codes: alt_off must ascend from 0");
    for (int64_t i = 0; i < nvar; ++i) {
      const int64_t A = alt_off[i + 1] - alt_off[i];
      bad |= (A < 0 ? 1u : 0u) | (A > 65535 ? 2u : 0u) | (ref_len[i] < 0 || ref_len[i] > 65535 ? 4u : 0u);
      bad |= pos[i] < 0 || pos[i] > T || (ref_len[i] >= 0 && pos[i] + ref_len[i] > T) ? 8u : 0u;
      if (bad & 1u) break;               // (what follows a descending offset is not to be trusted)
    }
    ARGCHK(!(bad & 1u), "crbm_allele_effects_codes: alt_off must ascend from 0");
    ARGCHK(!(bad & 2u), "crbm_allele_effects_codes: an alt of more than 65535 letters");
    ARGCHK(!(bad & 4u), "crbm_allele_effects_codes: every ref_len must lie in [0, 65535]");
    ARGCHK(!(bad & 8u), "crbm_allele_effects_codes: every span [pos, pos + ref_len) must lie inside [0, T]");
    const int64_t nalt = alt_off[nvar];
    ARGCHK(alt_codes || nalt == 0, "null argument");
    for (int64_t i = 0; i < nalt; ++i) bad |= alt_codes[i] > 3 ? 16u : 0u;
    ARGCHK(!(bad & 16u), "crbm_allele_effects_codes: every alt code must be a letter code 0..3");
  }
  rc = sweep_begin(h);
  if (rc) return rc;
  const int M = sw.M, K = h->K, nslab = sw.nslab;
  const SlabBudget budget = slab_budget();
  const AllelePlan ap = allele_plan((long)nvar, ref_len, alt_off, M, K, budget.bytes, budget.was_set);
  auto code_bytes = [](long n) { return ((size_t)n + 15) & ~(size_t)15; };         // the table follows the codes
  std::vector<uint8_t> host[2];
  for (int i = 0; i < ap.nsets; ++i) host[i].resize(code_bytes(ap.max_codes) + (size_t)ap.max_cnt * sizeof(AlleleEntry));
  rc = sw.size_inputs(ap.nsets, host[0].size(), ap.full);
  if (rc) return rc;
  for (int i = 0; i < ap.nsets; ++i) {                     // what both streams write, at its size, before either starts
    const SweepSet set = sweep_set(h, i);
    HIPCHK(set.oa->ensure((size_t)ap.max_cnt * K));
    HIPCHK(set.ob->ensure((size_t)ap.max_cnt));
    HIPCHK(set.own->var_windows.ensure((size_t)2 * ap.max_cnt));
  }
  return sw.run_chunks((int)ap.cuts.size() - 1, 1, "CRBM_ALLELE_TIMING", "chunks",
    [&](int si, StreamSweep::Chunk& c) -> int {            // (comes in as chunk c.start of the plan)
      const int64_t start = ap.cuts[c.start];
      const int cnt = (int)(ap.cuts[c.start + 1] - start);
      uint8_t* hap = host[si].data();
      // (the table's place does not depend on the codes gathered: sized from the plan's arithmetic, checked below)
      long n = 0;
      for (int i = 0; i < cnt; ++i) n += allele_codes(ref_len[start + i], alt_off[start + i + 1] - alt_off[start + i], M);
      AlleleEntry* table = reinterpret_cast<AlleleEntry*>(hap + code_bytes(n));
      const long wrote = gather_haplotypes(codes, T, pos + start, ref_len + start, alt_off + start, alt_codes, cnt, M, hap, table);
      if (wrote != n || n > ap.max_codes || cnt > ap.max_cnt) return fail(h, CRBM_ERR_INVALID, "crbm_allele_effects_codes: a chunk outgrew its plan");
      c.start = (int)start; c.cnt = cnt;
      c.bytes = hap; c.up = code_bytes(n) + (size_t)cnt * sizeof(AlleleEntry);
      c.n = n; c.layout_starts = n; c.starts = (int32_t)n;
      return CRBM_OK;
    },
    [&](const SweepSet& set, int, const ScanInput& in, int, int cnt) -> int {
      const unsigned char* staged = reinterpret_cast<const unsigned char*>(set.stage->p);
      AlleleArgs a{in};
      a.table = reinterpret_cast<const AlleleEntry*>(staged + code_bytes(in.starts));
      a.per_motif = set.oa->p; a.windows = set.own->var_windows.p;
      a.cnt = cnt; a.pad_ = 0;
      // a wave per variant, four waves a block
      const unsigned gx = (unsigned)std::max(1, std::min((cnt + 3) / 4, std::max(1, h->num_cu * 8 / nslab)));
      HIPCHK(jit_launch(sw.kjk->allele_effects, a, gx, (unsigned)nslab, 256, (unsigned)tab_bytes(*sw.kms), set.st));
      if (dfe) {
        AlleleCombineArgs c;
        c.per_motif = set.oa->p; c.codes = staged; c.table = a.table; c.c = h->dc.p; c.dfe = set.ob->p;
        c.cnt = cnt; c.K = K; c.M = M; c.pad_ = 0;
        hipLaunchKernelGGL(allele_combine_kernel, dim3(grid_for(cnt, 256, h->num_cu * 8)), dim3(256), 0, set.st, c);
        HIPCHK(hipGetLastError());
      }
      return CRBM_OK;
    },
    [&](const SweepSet& set, int, const ScanInput&, int start, int n) -> int {
      const size_t at = (size_t)start, cnt = (size_t)n;
      if (dfe) HIPCHK(hipMemcpyAsync(dfe + at, set.ob->p, cnt * sizeof(float), hipMemcpyDeviceToHost, set.st));
      if (per_motif) HIPCHK(hipMemcpyAsync(per_motif + at * K, set.oa->p, cnt * K * sizeof(float), hipMemcpyDeviceToHost, set.st));
      if (windows) HIPCHK(hipMemcpyAsync(windows + 2 * at, set.own->var_windows.p, 2 * cnt * sizeof(int32_t), hipMemcpyDeviceToHost, set.st));
      return CRBM_OK;
    });
}

// ---- in-silico mutagenesis (crbm_mutagenesis*) ----------------------------------------------------------------------
// dF (n,L,A) and / or pll (n) over a source, a two-stream sweep.  Specialised models without pooling: the fused
// crbm_mutagenesis pass (mutagenesis_body; as many waves per block as the LDS holds accumulators beside the tables).
// Everything else -- pooled models, generic models, CRBM_MUT_FUSED=0, sequences whose accumulator does not fit beside
// the tables -- takes the general path: mutagenesis_expand_kernel writes the slab's base rows and their (A-1) L copies,
// the class's own free-energy launch (launch_free_energy) leaves their per-motif terms in the set's outputs,
// mutagenesis_combine_kernel forms dF and pll.  Every set owns what it writes, sized before the sweep; the slab comes
// from the slab budget with the copies, their free energies and the outputs counted per row.
int mutagenesis_any(crbm_handle* h, const RowSource& src, float* dfe, float* pll) {
  ARGCHK(dfe || pll, "null argument");
  int rc = check_data_shape(h, src.n, src.L);
  if (rc) return rc;
  const int n = src.n, L = src.L, A = h->A, K = h->K, LW = lw(h, L);
  int waves = 0;
  if (!h->big() && h->ms().POOL == 1 && env_int("CRBM_MUT_FUSED", 1) != 0)
    for (waves = 4; waves >= 1; waves >>= 1)
      if ((size_t)tab_bytes(h->ms()) + (size_t)waves * 3 * mut_plane(L) * sizeof(float) <= 160u * 1024u) break;
  const bool fused = waves >= 1;
  const unsigned lds = fused ? (unsigned)(tab_bytes(h->ms()) + waves * 3 * mut_plane(L) * (int)sizeof(float)) : 0u;
  h->mut_route = fused ? 1 : 2;
  rc = sweep_begin(h);
  if (rc) return rc;
  const size_t per = (size_t)mut_rows_per_seq(A, L);
  const bool slabbed_fe = !fused && h->big() && slab_fe_on(h);
  // bytes per row: the outputs; on the general path also the row's expanded rows, their free energies (per sequence
  // and per motif) and, where the free energies run slab by slab, that pass's scratch (slab_launch_fe)
  size_t row_bytes = (dfe ? (size_t)L * A * sizeof(float) : 0) + sizeof(float);
  if (!fused) {
    row_bytes += per * ((size_t)LW * sizeof(uint32_t) + ((size_t)K + 1) * sizeof(float));
    if (slabbed_fe) row_bytes += per * (size_t)h->slab.K * h->slab_n * sizeof(float);
  }
  int slab = sweep_slab(src, row_bytes);
  if (!fused) slab = (int)std::max<size_t>(1, std::min<size_t>((size_t)slab, ((size_t)1 << 30) / per));   // expanded rows are counted in int
  // slabs of equal size: the two streams' launches run side by side, a short last slab would leave one of them idle
  if (slab < n) slab = (n + (n + slab - 1) / slab - 1) / ((n + slab - 1) / slab);
  for (int i = 0; i < (slab < n ? 2 : 1); ++i) {        // everything both streams write, at its size, before either starts
    const SweepSet set = sweep_set(h, i);
    HIPCHK(set.own->mut_pll.ensure((size_t)slab));
    if (dfe) HIPCHK(set.own->mut_df.ensure((size_t)slab * L * A));
    if (!fused) {
      HIPCHK(set.own->mut_rows.ensure((size_t)slab * per * LW));
      HIPCHK(set.oa->ensure((size_t)slab * per));
      HIPCHK(set.ob->ensure((size_t)slab * per * K));
      if (slabbed_fe) HIPCHK(set.fe_scratch->ensure((size_t)slab * per * h->slab.K * h->slab_n));
    }
  }
  return sweep_run(h, src, slab, 2,
    [&](const SweepSet& set, const uint32_t* rows, int, int cnt) -> int {
      float* d_df = dfe ? set.own->mut_df.p : nullptr;
      float* d_pll = set.own->mut_pll.p;
      if (fused) {
        MutArgs a;
        a.tables = h->d_tables.p; a.letters = rows;
        a.n = cnt; a.L = L; a.Lh = L - h->M + 1; a.LW = LW;
        a.dfe = d_df; a.pll = d_pll;
        // num_cu * 8 blocks like the other sweep kernels; a grid of only the resident blocks (5 per CU at config #2: no
        // second table copy) measured no faster, 8.70 against 8.46 ms over 10^5 x 200 bp: the kernel is bound by its VALU work
        const unsigned gx = (unsigned)std::max(1, std::min((cnt + waves - 1) / waves, h->num_cu * 8));
        HIPCHK(jit_launch(h->jk.mutagenesis, a, gx, 1, 64u * (unsigned)waves, lds, set.st));
        return CRBM_OK;
      }
      const size_t R = (size_t)cnt * per;
      MutExpandArgs e;
      e.rows = rows; e.out = set.own->mut_rows.p;
      e.n = cnt; e.L = L; e.LW = LW; e.A = A;
      hipLaunchKernelGGL(mutagenesis_expand_kernel, dim3(grid_for((long)(R * LW), 256, h->num_cu * 8)), dim3(256), 0, set.st, e);
      HIPCHK(hipGetLastError());
      const int r = launch_free_energy(h, e.out, (int)R, L, set);
      if (r) return r;
      MutCombineArgs c;
      c.fem = set.ob->p; c.c = h->dc.p; c.rows = rows;
      c.n = cnt; c.L = L; c.LW = LW; c.A = A; c.K = K;
      c.dfe = d_df; c.pll = d_pll;
      hipLaunchKernelGGL(mutagenesis_combine_kernel, dim3(std::max(1, std::min((cnt + 3) / 4, h->num_cu * 8))), dim3(256), 0, set.st, c);
      HIPCHK(hipGetLastError());
      return CRBM_OK;
    },
    [&](const SweepSet& set, const uint32_t*, int start, int cnt) -> int {
      if (dfe) HIPCHK(hipMemcpyAsync(dfe + (size_t)start * L * A, set.own->mut_df.p, (size_t)cnt * L * A * sizeof(float), hipMemcpyDeviceToHost, set.st));
      if (pll) HIPCHK(hipMemcpyAsync(pll + start, set.own->mut_pll.p, (size_t)cnt * sizeof(float), hipMemcpyDeviceToHost, set.st));
      HIPCHK(hipStreamSynchronize(set.st));
      return CRBM_OK;
    });
}

}  // namespace

int crbm_hit_probs(crbm_handle* h, const float* v, int32_t n, int32_t L, float* out) {
  ENTER();
  ARGCHK(v && out, "null argument");
  return hit_probs_any(h, host_onehot(v, n, L), out);
}

int crbm_hit_probs_codes(crbm_handle* h, const uint8_t* codes, int32_t n, int32_t L, float* out) {
  ENTER();
  ARGCHK(codes && out, "null argument");
  return hit_probs_any(h, host_codes(codes, n, L), out);
}

int crbm_hit_probs_resident(crbm_handle* h, int32_t start, int32_t end, float* out) {
  ENTER();
  ARGCHK(out, "null argument");
  RowSource src;
  int rc = resident_source(h, start, end, &src);
  if (rc) return rc;
  return hit_probs_any(h, src, out);
}

int crbm_free_energy(crbm_handle* h, const float* v, int32_t n, int32_t L, float* out) {
  ENTER();
  ARGCHK(v && out, "null argument");
  return free_energy_any(h, host_onehot(v, n, L), out, nullptr);
}

int crbm_free_energy_per_motif(crbm_handle* h, const float* v, int32_t n, int32_t L, float* out) {
  ENTER();
  ARGCHK(v && out, "null argument");
  return free_energy_any(h, host_onehot(v, n, L), nullptr, out);
}

int crbm_free_energy_codes(crbm_handle* h, const uint8_t* codes, int32_t n, int32_t L, float* fe, float* fe_per_motif) {
  ENTER();
  ARGCHK(codes && (fe || fe_per_motif), "null argument");
  return free_energy_any(h, host_codes(codes, n, L), fe, fe_per_motif);
}

int crbm_free_energy_resident(crbm_handle* h, int32_t start, int32_t end, float* fe, float* fe_per_motif) {
  ENTER();
  ARGCHK(fe || fe_per_motif, "null argument");
  RowSource src;
  int rc = resident_source(h, start, end, &src);
  if (rc) return rc;
  return free_energy_any(h, src, fe, fe_per_motif);
}

int crbm_eval_data(crbm_handle* h, const float* v, int32_t n, int32_t L, float* mfe, float* nmh) {
  ENTER();
  ARGCHK(v && mfe && nmh, "null argument");
  return eval_data_any(h, host_onehot(v, n, L), mfe, nmh);
}

// The per-epoch evaluation of fit() (convRBM.py:616-625) in one call: the selected resident set is walked in mini-batches
// of `batchsize` rows exactly as a loop over crbm_eval_data_resident would -- batch b draws its hidden sample with sampler
// step eval_step + b and rows indexed from 0 -- but every launch is enqueued before the one read-back.  Returns the MEAN
// OVER BATCHES of the batches' mean free energy and of their mean sampled hidden activity (what the reference's status
// line prints: a short last batch weighs as much as a full one), each batch value rounded to float as the per-batch
// entry point returns it.
int crbm_eval_epoch_resident(crbm_handle* h, int32_t batchsize, double* mean_fe, double* mean_nmh) {
  ENTER();
  ARGCHK(mean_fe && mean_nmh, "null argument");
  ARGCHK(batchsize >= 1, "batchsize must be positive");
  const int slot = h->slot;
  ARGCHK(h->dataset_n[slot] > 0, "no resident data set (call crbm_dataset_upload)");
  const int n = h->dataset_n[slot], L = h->dataset_L[slot], LW = lw(h, L), Lh = L - h->M + 1;
  int rc = check_data_shape(h, n, L);
  if (rc) return rc;
  const int nb = (n + batchsize - 1) / batchsize;
  HIPCHK(h->eval_ones.ensure((size_t)nb));
  HIPCHK(hipMemsetAsync(h->eval_ones.p, 0, (size_t)nb * sizeof(unsigned long long), h->stream));
  const uint32_t* rows = h->dataset[slot].p;
  rc = launch_free_energy(h, rows, n, L, sweep_set(h, 0));        // a row's free energy does not depend on its batch
  if (rc) return rc;
  for (int b = 0; b < nb; ++b) {
    const int start = b * batchsize, cnt = std::min(batchsize, n - start);
    rc = launch_hgv(h, rows + (size_t)start * LW, cnt, L, 0, nullptr, nullptr, nullptr, h->eval_ones.p + b, KIND_EVAL_H,
                    h->eval_step + (uint32_t)b, 0u);
    if (rc) return rc;
  }
  h->eval_step += (uint32_t)nb;
  std::vector<float> fe((size_t)n);
  std::vector<unsigned long long> ones((size_t)nb);
  HIPCHK(hipMemcpyAsync(fe.data(), h->out_a.p, (size_t)n * sizeof(float), hipMemcpyDeviceToHost, h->stream));
  HIPCHK(hipMemcpyAsync(ones.data(), h->eval_ones.p, (size_t)nb * sizeof(unsigned long long), hipMemcpyDeviceToHost, h->stream));
  HIPCHK(hipStreamSynchronize(h->stream));
  double sfe = 0.0, snmh = 0.0;
  for (int b = 0; b < nb; ++b) {
    const int start = b * batchsize, cnt = std::min(batchsize, n - start);
    double tot = 0.0;
    for (int i = 0; i < cnt; ++i) tot += fe[(size_t)start + i];
    sfe += (double)(float)(tot / cnt);                                              // convRBM.py:636-638 per batch
    snmh += (double)(float)((double)ones[(size_t)b] / ((double)cnt * h->K * Lh));     // :469-472
  }
  *mean_fe = sfe / nb;
  *mean_nmh = snmh / nb;
  return CRBM_OK;
}

int crbm_eval_data_resident(crbm_handle* h, int32_t start, int32_t end, float* mfe, float* nmh) {
  ENTER();
  ARGCHK(mfe && nmh, "null argument");
  RowSource src;
  int rc = resident_source(h, start, end, &src);
  if (rc) return rc;
  return eval_data_any(h, src, mfe, nmh);
}

int crbm_hit_summary(crbm_handle* h, const float* v, int32_t n, int32_t L, float* hit_max, float* hit_mean,
                     float* position_mean) {
  ENTER();
  ARGCHK(v && (hit_max || hit_mean || position_mean), "null argument");
  return hit_summary_any(h, host_onehot(v, n, L), hit_max, hit_mean, position_mean);
}

int crbm_hit_summary_codes(crbm_handle* h, const uint8_t* codes, int32_t n, int32_t L, float* hit_max, float* hit_mean,
                           float* position_mean) {
  ENTER();
  ARGCHK(codes && (hit_max || hit_mean || position_mean), "null argument");
  return hit_summary_any(h, host_codes(codes, n, L), hit_max, hit_mean, position_mean);
}

int crbm_hit_summary_resident(crbm_handle* h, int32_t start, int32_t end, float* hit_max, float* hit_mean,
                              float* position_mean) {
  ENTER();
  ARGCHK(hit_max || hit_mean || position_mean, "null argument");
  RowSource src;
  int rc = resident_source(h, start, end, &src);
  if (rc) return rc;
  return hit_summary_any(h, src, hit_max, hit_mean, position_mean);
}

int crbm_motif_sites(crbm_handle* h, const float* v, int32_t n, int32_t L, float threshold, int64_t capacity,
                     crbm_site* sites, int64_t* count, int32_t* best_start, int32_t* best_strand, float* best_prob) {
  ENTER();
  ARGCHK(v, "null argument");
  return motif_sites_any(h, host_onehot(v, n, L), threshold, capacity, sites, count, best_start, best_strand, best_prob);
}

int crbm_motif_sites_codes(crbm_handle* h, const uint8_t* codes, int32_t n, int32_t L, float threshold, int64_t capacity,
                           crbm_site* sites, int64_t* count, int32_t* best_start, int32_t* best_strand, float* best_prob) {
  ENTER();
  ARGCHK(codes, "null argument");
  return motif_sites_any(h, host_codes(codes, n, L), threshold, capacity, sites, count, best_start, best_strand, best_prob);
}

int crbm_motif_sites_resident(crbm_handle* h, int32_t start, int32_t end, float threshold, int64_t capacity,
                              crbm_site* sites, int64_t* count, int32_t* best_start, int32_t* best_strand,
                              float* best_prob) {
  ENTER();
  RowSource src;
  int rc = resident_source(h, start, end, &src);
  if (rc) return rc;
  return motif_sites_any(h, src, threshold, capacity, sites, count, best_start, best_strand, best_prob);
}

int crbm_scan_sites_codes(crbm_handle* h, const uint8_t* codes, int64_t T, float threshold, int64_t capacity,
                          crbm_site* sites, int64_t* count) {
  ENTER();
  return scan_sites_any(h, codes, T, threshold, capacity, sites, count);
}

int crbm_scan_histogram_codes(crbm_handle* h, const uint8_t* codes, int64_t T, float lo, float hi, int32_t nbins,
                              uint64_t* counts, int64_t* windows) {
  ENTER();
  return scan_hist_any(h, codes, T, lo, hi, nbins, counts, windows);
}

int crbm_scan_records_codes(crbm_handle* h, const uint8_t* codes, int64_t T, const int64_t* rec_start, int64_t nrec,
                            int64_t* windows, int64_t* letters, float* fe, float* fe_per_motif, int32_t* best_start,
                            int32_t* best_strand, float* best_prob, double* unit) {
  ENTER();
  return scan_records_any(h, codes, T, rec_start, nrec, windows, letters, fe, fe_per_motif, best_start, best_strand, best_prob, unit);
}

int crbm_variant_effects_codes(crbm_handle* h, const uint8_t* codes, int64_t T, int64_t nvar, const int64_t* pos,
                               const uint8_t* alt, float* dfe, float* dfe_per_motif, int32_t* windows) {
  ENTER();
  return variant_effects_any(h, codes, T, nvar, pos, alt, dfe, dfe_per_motif, windows);
}

int crbm_allele_effects_codes(crbm_handle* h, const uint8_t* codes, int64_t T, int64_t nvar, const int64_t* pos,
                              const int32_t* ref_len, const int64_t* alt_off, const uint8_t* alt_codes, float* dfe,
                              float* dfe_per_motif, int32_t* windows) {
  ENTER();
  return allele_effects_any(h, codes, T, nvar, pos, ref_len, alt_off, alt_codes, dfe, dfe_per_motif, windows);
}

int crbm_mutagenesis(crbm_handle* h, const float* v, int32_t n, int32_t L, float* dfe, float* pll) {
  ENTER();
  ARGCHK(v, "null argument");
  return mutagenesis_any(h, host_onehot(v, n, L), dfe, pll);
}

int crbm_mutagenesis_codes(crbm_handle* h, const uint8_t* codes, int32_t n, int32_t L, float* dfe, float* pll) {
  ENTER();
  ARGCHK(codes, "null argument");
  return mutagenesis_any(h, host_codes(codes, n, L), dfe, pll);
}

int crbm_mutagenesis_resident(crbm_handle* h, int32_t start, int32_t end, float* dfe, float* pll) {
  ENTER();
  RowSource src;
  int rc = resident_source(h, start, end, &src);
  if (rc) return rc;
  return mutagenesis_any(h, src, dfe, pll);
}

// Steps [t0,t1) of an annealed-importance-sampling ladder (include/crbm_amd.h; kernel: ais_body).  One wave per run, as
// many waves per block (at most four) as the LDS holds run slices beside the tables; the ladder goes out in launches of
// at most CRBM_AIS_STEPS steps (default 64: one launch then takes 2.0 ms for 8192 runs of 200 bp on config #2's model and 13.5 ms for 1024 runs of
// 1000 bp on config #4's, profiles/ais_bench.json), the letters and the float32 log weights of the runs
// passing from launch to launch in the handle's own buffers.
int crbm_ais(crbm_handle* h, int32_t L, int32_t runs, uint32_t run_offset, const float* betas, int32_t nbetas,
             int32_t t0, int32_t t1, const float* base_c, uint64_t seed, uint8_t* state, float* logw) {
  ENTER();
  ARGCHK(h->ms().POOL == 1, "crbm_ais: pooling > 1 is not supported (the pooled sampler and the pooled free energy normalise differently)");
  ARGCHK(h->A == 4, "crbm_ais: alphabets other than DNA's (input_dims != 4) are not supported");
  ARGCHK(!h->big(), "crbm_ais: models on the generic kernels are not supported");
  ARGCHK(betas && logw, "null argument");
  ARGCHK(L >= h->M, "sequence length must be >= motif_length");
  ARGCHK((long)L * 4 < (1 << 20), "sequence too long");
  ARGCHK(runs > 0, "runs must be positive");
  ARGCHK(nbetas >= 2, "nbetas must be at least 2");
  ARGCHK(0 <= t0 && t0 < t1 && t1 <= nbetas - 1, "t0, t1 must satisfy 0 <= t0 < t1 <= nbetas - 1");
  for (int i = 0; i < nbetas; ++i) {
    ARGCHK(std::isfinite(betas[i]), "betas must be finite");
    ARGCHK(betas[i] >= 0.f && betas[i] <= 1.f, "betas must lie inside [0,1]");
    ARGCHK(i == 0 || betas[i] >= betas[i - 1], "betas must not decrease");
  }
  ARGCHK(t0 == 0 || state, "t0 > 0 needs the state of the runs");
  if (base_c)
    for (int a = 0; a < 4; ++a) ARGCHK(std::isfinite(base_c[a]), "base_c must be finite");
  const AisLayout al = ais_layout(h->ms(), L);
  int waves = 4;
  while (waves >= 1 && ais_lds_bytes(h->ms(), al, waves) > 160L * 1024L) waves >>= 1;
  ARGCHK(waves >= 1, "crbm_ais: a run of this length does not fit the LDS beside the model's tables");
  const size_t nstate = (size_t)runs * L;
  if (t0 > 0)
    for (size_t i = 0; i < nstate; ++i) ARGCHK(state[i] < 4, "state holds a letter code outside 0..3");
  const int max_steps = std::max(1, env_int("CRBM_AIS_STEPS", 64));
  int rc = ensure_tables(h);
  if (rc) return rc;
  HIPCHK(h->ais_betas.ensure((size_t)nbetas));
  HIPCHK(h->ais_base.ensure(4));
  HIPCHK(h->ais_logw.ensure((size_t)runs));
  HIPCHK(h->ais_state.ensure(nstate));
  HIPCHK(hipMemcpyAsync(h->ais_betas.p, betas, (size_t)nbetas * sizeof(float), hipMemcpyHostToDevice, h->stream));
  if (base_c) HIPCHK(hipMemcpyAsync(h->ais_base.p, base_c, 4 * sizeof(float), hipMemcpyHostToDevice, h->stream));
  else HIPCHK(hipMemcpyAsync(h->ais_base.p, h->dc.p, 4 * sizeof(float), hipMemcpyDeviceToDevice, h->stream));
  if (t0 > 0) {
    HIPCHK(hipMemcpyAsync(h->ais_state.p, state, nstate, hipMemcpyHostToDevice, h->stream));
    HIPCHK(hipMemcpyAsync(h->ais_logw.p, logw, (size_t)runs * sizeof(float), hipMemcpyHostToDevice, h->stream));
  }
  AisArgs a;
  a.tables = h->d_tables.p; a.base_c = h->ais_base.p; a.betas = h->ais_betas.p;
  a.state = h->ais_state.p; a.logw = h->ais_logw.p;
  a.runs = runs; a.L = L; a.Lh = L - h->M + 1;
  a.nvb = al.nvb; a.Lrow = al.Lrow; a.LWs = al.LWs; a.run_words = al.run_words;
  a.rng.seed_lo = (uint32_t)(seed & 0xffffffffu); a.rng.seed_hi = (uint32_t)(seed >> 32);
  a.rng.step = 0; a.rng.seq_offset = run_offset;
  const unsigned gx = (unsigned)std::max(1, std::min((runs + waves - 1) / waves, h->num_cu * 8));
  const unsigned lds = (unsigned)ais_lds_bytes(h->ms(), al, waves);
  for (int t = t0; t < t1; t += max_steps) {
    a.t0 = t; a.t1 = std::min(t1, t + max_steps);
    HIPCHK(jit_launch(h->jk.ais, a, gx, 1, 64u * (unsigned)waves, lds, h->stream));
  }
  HIPCHK(hipMemcpyAsync(logw, h->ais_logw.p, (size_t)runs * sizeof(float), hipMemcpyDeviceToHost, h->stream));
  if (state) HIPCHK(hipMemcpyAsync(state, h->ais_state.p, nstate, hipMemcpyDeviceToHost, h->stream));
  HIPCHK(hipStreamSynchronize(h->stream));
  return CRBM_OK;
}

int crbm_eval_params(crbm_handle* h, float* twn, float* ic, float* medic) {
  ENTER();
  ARGCHK(twn && ic && medic, "null argument");
  const int K = h->K, M = h->M;
  std::vector<float> W((size_t)h->KAM);
  HIPCHK(hipMemcpyAsync(W.data(), h->dW.p, W.size() * 4, hipMemcpyDeviceToHost, h->stream));
  HIPCHK(hipStreamSynchronize(h->stream));
  // convRBM.py:475-485 on A*K*M numbers: host arithmetic in double
  const int A = h->A;
  double sq = 0.0, entsum = 0.0, medsum = 0.0;
  std::vector<double> ent((size_t)M), w((size_t)A);
  for (int k = 0; k < K; ++k) {
    for (int j = 0; j < M; ++j) {
      double mx = -1e300, z = 0.0, e = 0.0;
      for (int a = 0; a < A; ++a) {
        w[a] = W[(size_t)(k * A + a) * M + j];
        sq += w[a] * w[a];
        mx = std::max(mx, w[a]);
      }
      for (int a = 0; a < A; ++a) z += std::exp(w[a] - mx);
      for (int a = 0; a < A; ++a) {
        const double p = std::exp(w[a] - mx) / z;
        if (p > 0.0) e -= p * std::log2(p);
      }
      ent[j] = e;
      entsum += e;
    }
    std::sort(ent.begin(), ent.end());
    medsum += ent[(size_t)(M / 2)];
  }
  *twn = (float)std::sqrt(sq / (double)h->KAM);
  const double full = std::log2((double)A);     // log2 of the alphabet size (:481-484); 2 bits for DNA
  *ic = (float)(full - entsum / ((double)K * M));
  *medic = (float)(full - medsum / (double)K);
  return CRBM_OK;
}

// ---- data parallel -------------------------------------------------------------
int crbm_comm_unique_id(uint8_t id[CRBM_UNIQUE_ID_BYTES]) {
  if (!id) return CRBM_ERR_INVALID;
  if (!load_rccl()) { g_create_error = g_rccl.error; return CRBM_ERR_RCCL; }
  ncclUniqueId uid;
  static_assert(sizeof(uid) == CRBM_UNIQUE_ID_BYTES, "ncclUniqueId size");
  ncclResult_t r = g_rccl.GetUniqueId(&uid);
  if (r != ncclSuccess) { g_create_error = std::string("ncclGetUniqueId: ") + g_rccl.GetErrorString(r); return CRBM_ERR_RCCL; }
  memcpy(id, &uid, sizeof(uid));
  return CRBM_OK;
}

int crbm_comm_init(crbm_handle* h, const uint8_t id[CRBM_UNIQUE_ID_BYTES], int32_t nranks, int32_t rank) {
  ENTER();
  ARGCHK(id && nranks >= 1 && rank >= 0 && rank < nranks, "bad argument");
  if (!load_rccl()) return fail(h, CRBM_ERR_RCCL, g_rccl.error);
  if (h->comm) { g_rccl.CommDestroy(h->comm); h->comm = nullptr; }
  ncclUniqueId uid;
  memcpy(&uid, id, sizeof(uid));
  ncclResult_t r = g_rccl.CommInitRank(&h->comm, nranks, uid, rank);
  if (r != ncclSuccess) {
    h->comm = nullptr;
    return fail(h, CRBM_ERR_RCCL, std::string("ncclCommInitRank: ") + g_rccl.GetErrorString(r));
  }
  h->nranks = nranks; h->rank = rank;
  return CRBM_OK;
}

int crbm_comm_destroy(crbm_handle* h) {
  ENTER();
  if (h->comm) {
    HIPCHK(hipStreamSynchronize(h->stream));
    g_rccl.CommDestroy(h->comm);
    h->comm = nullptr;
  }
  h->nranks = 1; h->rank = 0;
  return CRBM_OK;
}

// Replicas must start identical: only raw statistic sums are all-reduced, so a
// rank that begins from different parameters would apply the common update to a
// different model for ever.  ncclBroadcast of W, b, c and the three velocities
// from `root` (no-op without a communicator).
int crbm_comm_broadcast_state(crbm_handle* h, int32_t root) {
  ENTER();
  if (!h->comm) return CRBM_OK;
  ARGCHK(root >= 0 && root < h->nranks, "root out of range");
  struct { float* p; size_t n; } bufs[] = {{h->dW.p, (size_t)h->KAM}, {h->db.p, (size_t)h->K}, {h->dc.p, (size_t)h->A},
                                           {h->dvW.p, (size_t)h->KAM}, {h->dvb.p, (size_t)h->K}, {h->dvc.p, (size_t)h->A}};
  for (auto& b : bufs) {
    ncclResult_t r = g_rccl.Broadcast(b.p, b.p, b.n, ncclFloat, root, h->comm, h->stream);
    if (r != ncclSuccess) return fail(h, CRBM_ERR_RCCL, std::string("ncclBroadcast: ") + g_rccl.GetErrorString(r));
  }
  HIPCHK(hipStreamSynchronize(h->stream));
  h->tables_dirty = true;
  h->params_version += 1;
  return CRBM_OK;
}

// ---- all-reduce through mapped buffers (no collective launch) -------------------------------------
int crbm_ipc_export(crbm_handle* h, uint8_t handle[CRBM_IPC_HANDLE_BYTES]) {
  ENTER();
  ARGCHK(handle, "null argument");
  static_assert(sizeof(hipIpcMemHandle_t) == CRBM_IPC_HANDLE_BYTES, "hipIpcMemHandle_t size");
  int rc = ipc_allocate(h);
  if (rc) return rc;
  // flags and status start from zero with every attachment (the step count does too): cleared here, before the
  // handle leaves -- no peer pushes into this buffer before it has seen the handles of all ranks
  HIPCHK(hipStreamSynchronize(h->stream));
  HIPCHK(hipMemset(h->ipc_buf.p, 0, ipc_bytes(h)));
  hipIpcMemHandle_t mh;
  HIPCHK(hipIpcGetMemHandle(&mh, h->ipc_buf.p));
  memcpy(handle, &mh, sizeof(mh));
  return CRBM_OK;
}

int crbm_ipc_attach(crbm_handle* h, const uint8_t* handles, int32_t nranks, int32_t rank) {
  ENTER();
  ARGCHK(handles && nranks >= 1 && nranks <= IPC_MAX_RANKS && rank >= 0 && rank < nranks, "bad argument (at most 8 ranks: one node)");
  ARGCHK(!h->comm, "the handle already has an RCCL communicator");
  ARGCHK(!h->big(), "the mapped-buffer all-reduce serves models of the LDS-resident kernels; this one (generic kernels) takes RCCL");
  int rc = ipc_allocate(h);
  if (rc) return rc;
  for (int r = 0; r < nranks; ++r) {
    if (r == rank) { h->ipc_peer.set_own(r, h->ipc_buf.p); continue; }
    hipIpcMemHandle_t mh;
    memcpy(&mh, handles + (size_t)r * CRBM_IPC_HANDLE_BYTES, sizeof(mh));
    hipError_t e = h->ipc_peer.open(r, mh);
    if (e != hipSuccess) return fail(h, CRBM_ERR_HIP, std::string("hipIpcOpenMemHandle (rank ") + std::to_string(r) + "): " + hipGetErrorString(e));
  }
  h->nranks = nranks; h->rank = rank;
  h->ipc_on = true;
  h->ipc_step = 0;
  // the bound of an update launch's wait for its peers, in ticks of the GPU's constant-rate clock (s_memrealtime;
  // its rate in kHz = ticks per millisecond, 100 MHz on every part so far)
  int khz = 0;
  if (hipDeviceGetAttribute(&khz, hipDeviceAttributeWallClockRate, h->device) != hipSuccess || khz <= 0) {
    (void)hipGetLastError();
    khz = 100000;
  }
  h->ipc_timeout_ticks = (unsigned long long)std::max(1, env_int("CRBM_IPC_TIMEOUT_MS", 30000)) * (unsigned long long)khz;
  return CRBM_OK;
}

int crbm_ipc_detach(crbm_handle* h) {
  ENTER();
  HIPCHK(hipStreamSynchronize(h->stream));
  h->ipc_peer.close();
  h->ipc_on = false;
  h->nranks = 1; h->rank = 0;
  return CRBM_OK;
}

int crbm_ipc_status(crbm_handle* h, int32_t* timed_out) {
  ENTER();
  ARGCHK(timed_out, "null argument");
  *timed_out = 0;
  if (!h->ipc_buf.p) return CRBM_OK;
  uint32_t st = 0;
  HIPCHK(hipStreamSynchronize(h->stream));
  HIPCHK(hipMemcpy(&st, ipc_status_of(h->ipc_buf.p, h), sizeof(st), hipMemcpyDeviceToHost));
  *timed_out = (int32_t)st;
  return CRBM_OK;
}

int crbm_sums_count(const crbm_handle* h) { return h ? h->sl.count : 0; }

int crbm_train_local(crbm_handle* h, const float* D, int32_t n, int32_t L, float* sums_out) {
  ENTER();
  ARGCHK(sums_out && (D || n == 0), "null argument");
  int rc = check_data_shape(h, std::max(n, 1), L);
  if (rc) return rc;
  ARGCHK(n >= 0, "n must be non-negative");
  if (n > 0) {   // n == 0: a rank that owns no row of a short last mini-batch contributes zeros
    rc = encode_now(h, host_onehot(D, n, L), 0, n);
    if (rc) return rc;
  }
  rc = train_local_dev(h, h->letters.p, n, L);
  if (rc) return rc;
  rc = copy_out(h, sums_out, h->d_sums.p, (size_t)h->sl.count);
  if (rc) return rc;
  HIPCHK(hipStreamSynchronize(h->stream));
  return CRBM_OK;
}

int crbm_train_apply(crbm_handle* h, const float* sums_in, int32_t L_data) {
  ENTER();
  ARGCHK(sums_in && L_data >= h->M, "bad argument");
  HIPCHK(hipMemcpyAsync(h->d_sums.p, sums_in, (size_t)h->sl.count * 4, hipMemcpyHostToDevice, h->stream));
  int rc = launch_update(h, L_data);
  if (rc) return rc;
  HIPCHK(hipStreamSynchronize(h->stream));
  return CRBM_OK;
}

int crbm_time_allreduce(crbm_handle* h, int32_t launches, float* total_ms) {
  ENTER();
  ARGCHK(launches >= 1 && total_ms, "bad argument");
  *total_ms = 0.f;
  if (!h->comm) return CRBM_OK;
  HIPCHK(hipEventRecord(h->ev0, h->stream));
  for (int i = 0; i < launches; ++i) {
    ncclResult_t r = g_rccl.AllReduce(h->d_sums.p, h->d_sums.p, (size_t)h->sl.count, ncclFloat, ncclSum, h->comm, h->stream);
    if (r != ncclSuccess) return fail(h, CRBM_ERR_RCCL, std::string("ncclAllReduce: ") + g_rccl.GetErrorString(r));
  }
  HIPCHK(hipEventRecord(h->ev1, h->stream));
  HIPCHK(spin_until(h->ev1));
  HIPCHK(hipEventElapsedTime(total_ms, h->ev0, h->ev1));
  return CRBM_OK;
}

int crbm_get_launch_info(const crbm_handle* h, crbm_launch_info* out) {
  if (!h || !out) return CRBM_ERR_INVALID;
  if (h->big()) {          // generic kernels: no specialised geometry to report
    *out = crbm_launch_info();
    out->gibbs_sparse = 1; out->chain_parts = 1; out->gibbs_block = 256;
    out->activity_ppm = h->activity < 0.0 ? -1 : (int32_t)(h->activity * 1e6 + 0.5);
    out->mutagenesis_route = h->mut_route;
    return CRBM_OK;
  }
  // the data-half statistics kernel at the chains' shape (stats_mfma_body)
  const int tabs = h->ms().TAB * 4;
  const StatsMfmaLayout st = stats_mfma_layout(h->ms(), 1, h->Lf, 0, tabs);
  const int lds = std::max(st.region_floats * 4 + tabs, st.combine_bytes);
  // a plain chain launch (crbm_gibbs_steps*): its letter grouping, its geometry
  const ChainGeom& g = plain_geom(h->plan, h->variant);
  out->nq = h->ms().NQ; out->group = h->plan.GS;
  out->chain_parts = h->variant == 1 ? h->plan.chain_parts : 1;
  out->gibbs_grid = g.grid; out->gibbs_block = g.threads;
  out->gibbs_seqs_per_tile = g.gl.S; out->gibbs_lds_bytes = g.gl.lds_bytes;
  out->stats_grid_x = h->stats_rows > 0 ? h->stats_rows
                                        : h->num_cu * std::max(1, std::min(2048 / st.threads, (160 * 1024) / std::max(1, lds)));
  out->stats_grid_y = 1;
  out->stats_block = st.threads; out->stats_lds_bytes = lds;
  out->stats_fused = h->fuse_stats ? 1 : 0;
  out->gibbs_sparse = h->variant;
  out->activity_ppm = h->activity < 0.0 ? -1 : (int32_t)(h->activity * 1e6 + 0.5);
  out->mutagenesis_route = h->mut_route;
  return CRBM_OK;
}

// Device-copy bandwidth of this GPU, measured with a float4 copy kernel on the
// library's stream (HIP events): the practical ceiling next to the 8 TB/s spec
// that bench.py quotes its roofline fraction against as well.
int crbm_copy_bandwidth(crbm_handle* h, int64_t bytes, int32_t reps, float* gb_per_s) {
  ENTER();
  ARGCHK(bytes >= (1 << 20) && reps >= 1 && gb_per_s, "bad argument");
  const size_t n4 = (size_t)bytes / 16;
  DevBuf<float4> src, dst;
  HIPCHK(src.alloc(n4));
  HIPCHK(dst.alloc(n4));
  (void)hipMemsetAsync(src.p, 1, n4 * 16, h->stream);
  const unsigned grid = (unsigned)((n4 + 1023) / 1024);
  for (int i = 0; i < 1 + reps; ++i) {
    if (i == 1) (void)hipEventRecord(h->ev0, h->stream);
    hipLaunchKernelGGL(copy_float4_kernel, dim3(grid), dim3(256), 0, h->stream, src.p, dst.p, n4);
  }
  (void)hipEventRecord(h->ev1, h->stream);
  hipError_t e = hipEventSynchronize(h->ev1);
  float ms = 0.f;
  if (e == hipSuccess) e = hipEventElapsedTime(&ms, h->ev0, h->ev1);
  if (e != hipSuccess) return fail(h, CRBM_ERR_HIP, std::string("copy bandwidth: ") + hipGetErrorString(e));
  *gb_per_s = (float)(2.0 * (double)n4 * 16.0 * reps / (ms * 1e-3) / 1e9);   // bytes read + written
  return CRBM_OK;
}

int crbm_live_resources(int64_t counts[5]) {      // buffers, bytes, streams, events, modules (crbm_own.h: LiveKind)
  if (!counts) return CRBM_ERR_INVALID;
  for (int i = 0; i < LIVE_KINDS; ++i) counts[i] = live(i).load(std::memory_order_relaxed);
  return CRBM_OK;
}

int crbm_geometry_launches(const crbm_handle* h, int64_t* compiled_in, int64_t* run_time) {
  if (!h) return CRBM_ERR_INVALID;
  if (compiled_in) *compiled_in = h->geo_launches[1];
  if (run_time) *run_time = h->geo_launches[0];
  return CRBM_OK;
}

// Shader clock during the launches of the last crbm_time_gibbs call: block 0 of every launch (of partition 0) adds its
// duration in wall-clock ticks and in shader cycles (GibbsArgs::clock); MHz = cycles / ticks x tick rate.  0 if unknown.
int crbm_last_shader_clock(crbm_handle* h, float* mhz) {
  ENTER();
  ARGCHK(mhz, "null argument");
  *mhz = 0.f;
  HIPCHK(hipStreamSynchronize(h->stream));
  HIPCHK(hipMemcpy(h->probe_last, h->d_probe.p, sizeof(h->probe_last), hipMemcpyDeviceToHost));
  const unsigned long long ticks = h->probe_last[0] - h->probe_base[0], cycles = h->probe_last[1] - h->probe_base[1];
  if (ticks) *mhz = (float)((double)cycles / ((double)ticks / (h->wall_khz / 1000.0)));
  return CRBM_OK;
}

int64_t crbm_gibbs_state_bytes(const crbm_handle* h) {
  if (!h) return 0;
  const int64_t masks = (int64_t)h->B * h->Lf * h->NW * 4 * (1 + h->ds);
  const int64_t vout = (int64_t)h->B * h->LWs * 4;
  return 2 * masks + vout;   // masks read + written, last visible sample written
}

}  // extern "C"

// ---- t-SNE (crbm_tsne.h): the handle lends its device, stream and error string; the model plays no part --------------
namespace {

// device buffers of one call, freed whichever way the call ends
struct CallBufs {
  std::deque<DevBuf<unsigned char>> bufs;
  template <typename T>
  hipError_t get(T** out, size_t count) {
    bufs.emplace_back();
    const hipError_t e = bufs.back().alloc(std::max<size_t>(count, 1) * sizeof(T));
    *out = reinterpret_cast<T*>(bufs.back().p);
    return e;
  }
};

unsigned tsne_grid(int64_t blocks) { return (unsigned)std::min<int64_t>(std::max<int64_t>(blocks, 1), 65535); }

}  // namespace

extern "C" {

int crbm_tsne_neighbors(crbm_handle* h, const float* X, int64_t n, int32_t D, int32_t k, int32_t* idx, float* d2) {
  ENTER();
  ARGCHK(X && idx && d2, "null argument");
  if (const char* why = tsne::neighbors_refusal(n, D, k)) return fail(h, CRBM_ERR_INVALID, why);
  for (int64_t e = 0; e < n * D; ++e) ARGCHK(std::isfinite(X[e]), "X is not finite");
  int waves = 8;                                     // queries per block; fewer where the lists and rows do not fit
  while (waves > 1 && tsne::knn_lds_bytes(D, k, waves) > 128 * 1024) waves >>= 1;
  const size_t lds = tsne::knn_lds_bytes(D, k, waves);
  ARGCHK(lds <= 160 * 1024, "k and D leave no room in the LDS");
  CallBufs s;
  float *dX = nullptr, *dd2 = nullptr;
  int32_t* didx = nullptr;
  HIPCHK(s.get(&dX, (size_t)n * D));
  HIPCHK(s.get(&didx, (size_t)n * k));
  HIPCHK(s.get(&dd2, (size_t)n * k));
  HIPCHK(hipMemcpyAsync(dX, X, (size_t)n * D * 4, hipMemcpyHostToDevice, h->stream));
  HIPCHK(hipFuncSetAttribute(reinterpret_cast<const void*>(tsne::tsne_knn_kernel), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
  const tsne::KnnArgs a{dX, didx, dd2, (int)n, D, k};
  hipLaunchKernelGGL(tsne::tsne_knn_kernel, dim3(tsne_grid((n + waves - 1) / waves)), dim3(64 * waves), lds, h->stream, a);
  HIPCHK(hipGetLastError());
  HIPCHK(hipMemcpyAsync(idx, didx, (size_t)n * k * 4, hipMemcpyDeviceToHost, h->stream));
  HIPCHK(hipMemcpyAsync(d2, dd2, (size_t)n * k * 4, hipMemcpyDeviceToHost, h->stream));
  HIPCHK(hipStreamSynchronize(h->stream));
  return CRBM_OK;
}

int crbm_tsne_affinities(crbm_handle* h, const float* d2, int64_t n, int32_t k, float perplexity, float* p, float* beta) {
  ENTER();
  ARGCHK(d2 && p && beta, "null argument");
  if (const char* why = tsne::affinities_refusal(n, k, perplexity)) return fail(h, CRBM_ERR_INVALID, why);
  for (int64_t e = 0; e < n * k; ++e) ARGCHK(std::isfinite(d2[e]) && d2[e] >= 0.f, "a distance is negative or not finite");
  CallBufs s;
  float *dd2 = nullptr, *dp = nullptr, *dbeta = nullptr;
  HIPCHK(s.get(&dd2, (size_t)n * k));
  HIPCHK(s.get(&dp, (size_t)n * k));
  HIPCHK(s.get(&dbeta, (size_t)n));
  HIPCHK(hipMemcpyAsync(dd2, d2, (size_t)n * k * 4, hipMemcpyHostToDevice, h->stream));
  const tsne::AffinityArgs a{dd2, dp, dbeta, (int)n, k, std::log((double)perplexity)};
  hipLaunchKernelGGL(tsne::tsne_affinity_kernel, dim3(tsne_grid((n + 63) / 64)), dim3(64), 0, h->stream, a);
  HIPCHK(hipGetLastError());
  HIPCHK(hipMemcpyAsync(p, dp, (size_t)n * k * 4, hipMemcpyDeviceToHost, h->stream));
  HIPCHK(hipMemcpyAsync(beta, dbeta, (size_t)n * 4, hipMemcpyDeviceToHost, h->stream));
  HIPCHK(hipStreamSynchronize(h->stream));
  return CRBM_OK;
}

int crbm_tsne_descend(crbm_handle* h, int64_t n, const int64_t* indptr, const int32_t* indices, const float* values, float* y,
                      float* velocity, float* gains, int32_t iterations, float exaggeration, float learning_rate, float momentum,
                      float* grad_last, double* kl, double* z) {
  ENTER();
  ARGCHK(indptr && y && velocity && gains, "null argument");
  ARGCHK(n >= 2 && n <= tsne::MAX_N, "t-SNE needs at least two rows (and at most 2^30)");
  ARGCHK(indptr[0] == 0 && indptr[n] >= 0, "indptr must start at 0 and ascend");
  ARGCHK(indptr[n] == 0 || (indices && values), "null argument");
  if (const char* why = tsne::descend_refusal(n, indptr, indices, iterations)) return fail(h, CRBM_ERR_INVALID, why);
  const size_t nnz = (size_t)indptr[n];
  const int S = tsne::slices(n);
  const int64_t chunks = tsne::sum_chunks(n);
  CallBufs s;
  int64_t* dptr = nullptr;
  int32_t* dind = nullptr;
  float* dval = nullptr;
  float2 *dy[2] = {nullptr, nullptr}, *dvel = nullptr, *dgain = nullptr, *dgrad = nullptr;
  float4 *dpart = nullptr, *drs = nullptr;
  double *dchunk = nullptr, *dklrow = nullptr, *dscalar = nullptr;   // dscalar: Z, KL
  HIPCHK(s.get(&dptr, (size_t)n + 1));
  HIPCHK(s.get(&dind, nnz));
  HIPCHK(s.get(&dval, nnz));
  HIPCHK(s.get(&dy[0], (size_t)n));
  HIPCHK(s.get(&dy[1], (size_t)n));
  HIPCHK(s.get(&dvel, (size_t)n));
  HIPCHK(s.get(&dgain, (size_t)n));
  HIPCHK(s.get(&dgrad, (size_t)n));
  HIPCHK(s.get(&dpart, (size_t)n * S));
  HIPCHK(s.get(&drs, (size_t)n));
  HIPCHK(s.get(&dchunk, (size_t)chunks));
  HIPCHK(s.get(&dklrow, (size_t)n));
  HIPCHK(s.get(&dscalar, 2));
  HIPCHK(hipMemcpyAsync(dptr, indptr, ((size_t)n + 1) * 8, hipMemcpyHostToDevice, h->stream));
  if (nnz) {
    HIPCHK(hipMemcpyAsync(dind, indices, nnz * 4, hipMemcpyHostToDevice, h->stream));
    HIPCHK(hipMemcpyAsync(dval, values, nnz * 4, hipMemcpyHostToDevice, h->stream));
  }
  HIPCHK(hipMemcpyAsync(dy[0], y, (size_t)n * 8, hipMemcpyHostToDevice, h->stream));
  HIPCHK(hipMemcpyAsync(dvel, velocity, (size_t)n * 8, hipMemcpyHostToDevice, h->stream));
  HIPCHK(hipMemcpyAsync(dgain, gains, (size_t)n * 8, hipMemcpyHostToDevice, h->stream));
  HIPCHK(hipMemsetAsync(dscalar, 0, 16, h->stream));
  // iterations == 0: one evaluation at y (gradient, KL, Z), nothing moves
  const int passes = iterations > 0 ? iterations : 1;
  const unsigned row_grid = tsne_grid((n + 255) / 256), chunk_grid = tsne_grid(chunks);
  int cur = 0;
  HIPCHK(hipEventRecord(h->ev0, h->stream));
  for (int it = 0; it < passes; ++it) {
    const bool last = it == passes - 1;
    const tsne::RepulsionArgs ra{dy[cur], dpart, (int)n, S, tsne::slice_tiles(n)};
    hipLaunchKernelGGL(tsne::tsne_repulsion_kernel, dim3(row_grid, S), dim3(256), tsne::TJ * 8, h->stream, ra);
    const tsne::CombineArgs ca{dpart, drs, dchunk, (int)n, S};
    hipLaunchKernelGGL(tsne::tsne_combine_kernel, dim3(chunk_grid), dim3(256), tsne::SUM_CHUNK * 8, h->stream, ca);
    const tsne::SumArgs za{dchunk, dscalar, chunks};
    hipLaunchKernelGGL(tsne::tsne_final_sum_kernel, dim3(1), dim3(256), tsne::SUM_CHUNK * 8, h->stream, za);
    const bool want_kl = last && kl;
    const tsne::StepArgs sa{dptr, dind, dval, dy[cur], dy[cur ^ 1], dvel, dgain, drs, dscalar, (last && grad_last) ? dgrad : nullptr,
                            want_kl ? dklrow : nullptr, (int)n, iterations > 0 ? 1 : 0, exaggeration, learning_rate, momentum};
    hipLaunchKernelGGL(tsne::tsne_step_kernel, dim3(row_grid), dim3(256), 0, h->stream, sa);
    if (want_kl) {
      const tsne::SumArgs ka{dklrow, dchunk, n};
      hipLaunchKernelGGL(tsne::tsne_chunk_sum_kernel, dim3(chunk_grid), dim3(256), tsne::SUM_CHUNK * 8, h->stream, ka);
      const tsne::SumArgs kf{dchunk, dscalar + 1, chunks};
      hipLaunchKernelGGL(tsne::tsne_final_sum_kernel, dim3(1), dim3(256), tsne::SUM_CHUNK * 8, h->stream, kf);
    }
    HIPCHK(hipGetLastError());
    if (iterations > 0) cur ^= 1;
  }
  HIPCHK(hipEventRecord(h->ev1, h->stream));
  double scalars[2] = {0.0, 0.0};
  HIPCHK(hipMemcpyAsync(scalars, dscalar, 16, hipMemcpyDeviceToHost, h->stream));
  if (iterations > 0) {
    HIPCHK(hipMemcpyAsync(y, dy[cur], (size_t)n * 8, hipMemcpyDeviceToHost, h->stream));
    HIPCHK(hipMemcpyAsync(velocity, dvel, (size_t)n * 8, hipMemcpyDeviceToHost, h->stream));
    HIPCHK(hipMemcpyAsync(gains, dgain, (size_t)n * 8, hipMemcpyDeviceToHost, h->stream));
  }
  if (grad_last) HIPCHK(hipMemcpyAsync(grad_last, dgrad, (size_t)n * 8, hipMemcpyDeviceToHost, h->stream));
  HIPCHK(hipStreamSynchronize(h->stream));
  HIPCHK(hipEventElapsedTime(&h->tsne_ms, h->ev0, h->ev1));
  if (z) *z = scalars[0];
  if (kl) *kl = scalars[1];
  return CRBM_OK;
}

int crbm_tsne_descend_ms(crbm_handle* h, float* ms) {
  if (!h || !ms) return CRBM_ERR_INVALID;
  *ms = h->tsne_ms;
  return CRBM_OK;
}

}  // extern "C"

// ---- Markov backgrounds (crbm_background.h): the handle lends its device, its two streams and its error string; the
// model plays no part (StreamSweep::admit refuses by model and is not used) ---------------------------------------------
namespace {

// events of one call, destroyed whichever way the call ends
struct CallEvents {
  Event walk[2];                       // a set's walk kernel has left the carry of the next segment
  Event t[2][2];                       // around a set's kernels
  hipError_t create() {
    hipError_t rc = hipSuccess;
    for (Event& e : walk) if (rc == hipSuccess) rc = e.create_untimed();
    for (auto& set : t) for (Event& e : set) if (rc == hipSuccess) rc = e.create();
    return rc;
  }
};

// positions per segment: the slab budget (CRBM_SLAB_BYTES) at `bytes_per_position`, within 32 MB unless set by hand
int bg_segment(int64_t T, size_t bytes_per_position) {
  const SlabBudget budget = slab_budget();
  size_t seg = std::max<size_t>(budget.bytes / bytes_per_position, 1);
  if (!budget.was_set) seg = std::min(seg, std::max<size_t>(1, (32u << 20) / bytes_per_position));
  return (int)std::min<size_t>(seg, (size_t)std::max<int64_t>(T, 1));
}

void bg_drain(crbm_handle* h) {
  (void)hipStreamSynchronize(h->stream2);
  (void)hipStreamSynchronize(h->stream);
}

template <int ORDER>
int bg_sample_launch(crbm_handle* h, const bg::SampleArgs& a, hipStream_t st, hipEvent_t wait_for, hipEvent_t walked) {
  constexpr int NS = bg::contexts(ORDER);
  const unsigned lanes_grid = (unsigned)grid_for((long)a.chunks, 64, h->num_cu * 32), group_grid = (unsigned)grid_for((long)a.groups, 64, h->num_cu * 32);
  hipLaunchKernelGGL(bg::sample_maps_kernel<ORDER>, dim3(lanes_grid), dim3(64), NS * 16, st, a);
  hipLaunchKernelGGL(bg::sample_groups_kernel<ORDER>, dim3(group_grid), dim3(64), 0, st, a);
  if (wait_for) HIPCHK(hipStreamWaitEvent(st, wait_for, 0));          // the carry of the segment before
  hipLaunchKernelGGL(bg::sample_walk_kernel<ORDER>, dim3(1), dim3(256), bg::WALK_TILE * NS, st, a);
  HIPCHK(hipEventRecord(walked, st));
  hipLaunchKernelGGL(bg::sample_entries_kernel<ORDER>, dim3(group_grid), dim3(64), 0, st, a);
  hipLaunchKernelGGL(bg::sample_letters_kernel<ORDER>, dim3(lanes_grid), dim3(64), NS * 16, st, a);
  HIPCHK(hipGetLastError());
  return CRBM_OK;
}

}  // namespace

extern "C" {

int crbm_stream_kmer_counts(crbm_handle* h, const uint8_t* codes, int64_t T, int32_t order, uint64_t* counts) {
  ENTER();
  if (const char* why = bg::counts_refusal(codes, T, order, counts)) return fail(h, CRBM_ERR_INVALID, std::string("crbm_stream_kmer_counts: ") + why);
  const int slots = bg::kmer_slots(order), seg = bg_segment(T, 1), nsets = seg < T ? 2 : 1;
  CallBufs s;
  unsigned long long* dcounts = nullptr;
  uint8_t* dcodes[2] = {nullptr, nullptr};
  HIPCHK(s.get(&dcounts, (size_t)slots));
  for (int i = 0; i < nsets; ++i) HIPCHK(s.get(&dcodes[i], (size_t)seg + order));
  CallEvents ev;
  HIPCHK(ev.create());
  HIPCHK(hipMemsetAsync(dcounts, 0, (size_t)slots * 8, h->stream));
  HIPCHK(hipStreamSynchronize(h->stream));               // (the second stream adds to the counters too)
  double device_ms = 0.0;
  const int rc = run_slabs((int)T, seg, 2,
    [&](int, int si, int start, int cnt) -> int {
      const hipStream_t st = si ? h->stream2 : h->stream;
      const int64_t n = std::min<int64_t>((int64_t)cnt + order, T - start);   // the halo: `order` codes behind the segment's own
      HIPCHK(hipMemcpyAsync(dcodes[si], codes + start, (size_t)n, hipMemcpyHostToDevice, st));
      HIPCHK(hipEventRecord(ev.t[si][0], st));
      const bg::KmerArgs a{dcodes[si], dcounts, n, cnt, order};
      hipLaunchKernelGGL(bg::kmer_count_kernel, dim3(grid_for(cnt, 256, h->num_cu * 8)), dim3(256), (size_t)slots * 4, st, a);
      HIPCHK(hipGetLastError());
      HIPCHK(hipEventRecord(ev.t[si][1], st));
      return CRBM_OK;
    },
    [&](int, int si, int, int) -> int {
      HIPCHK(hipStreamSynchronize(si ? h->stream2 : h->stream));
      float ms = 0.f;
      HIPCHK(hipEventElapsedTime(&ms, ev.t[si][0], ev.t[si][1]));
      device_ms += ms;
      return CRBM_OK;
    },
    [&] { bg_drain(h); });
  if (rc) return rc;
  std::vector<unsigned long long> got((size_t)slots);
  HIPCHK(hipMemcpyAsync(got.data(), dcounts, (size_t)slots * 8, hipMemcpyDeviceToHost, h->stream));
  HIPCHK(hipStreamSynchronize(h->stream));
  for (int e = 0; e < slots; ++e) counts[e] = got[e];
  h->bg_ms = (float)device_ms;
  return CRBM_OK;
}

int crbm_background_sample(crbm_handle* h, const uint32_t* thr, int32_t order, int64_t T, int64_t pos0, uint64_t seed,
                           const uint8_t* tmpl, uint8_t* out) {
  ENTER();
  if (const char* why = bg::sample_refusal(thr, order, T, pos0, tmpl, out)) return fail(h, CRBM_ERR_INVALID, std::string("crbm_background_sample: ") + why);
  h->bg_ms = 0.f;
  if (T == 0) return CRBM_OK;
  const int NS = bg::contexts(order), chunk = bg::chunk_length(env_int("CRBM_BG_CHUNK", bg::CHUNK_DEFAULT));
  const int seg = bg_segment(T, 3), nsets = seg < T ? 2 : 1;
  const int64_t seg_chunks = ((int64_t)seg + chunk - 1) / chunk, seg_groups = (seg_chunks + bg::GROUP - 1) / bg::GROUP;
  uint32_t rows[4 * bg::contexts(bg::MAX_ORDER)];
  bg::build_rows(thr, order, rows);
  CallBufs s;
  uint4* drows = nullptr;
  uint8_t *dcarry = nullptr, *dtmpl[2] = {nullptr, nullptr}, *dout[2] = {nullptr, nullptr}, *dcmap[2] = {nullptr, nullptr},
          *dgmap[2] = {nullptr, nullptr}, *dcentry[2] = {nullptr, nullptr}, *dgentry[2] = {nullptr, nullptr};
  HIPCHK(s.get(&drows, (size_t)NS));
  HIPCHK(s.get(&dcarry, 4));
  for (int i = 0; i < nsets; ++i) {
    if (tmpl) HIPCHK(s.get(&dtmpl[i], (size_t)seg));
    HIPCHK(s.get(&dout[i], (size_t)seg));
    HIPCHK(s.get(&dcmap[i], (size_t)seg_chunks * NS));
    HIPCHK(s.get(&dgmap[i], (size_t)seg_groups * NS));
    HIPCHK(s.get(&dcentry[i], (size_t)seg_chunks));
    HIPCHK(s.get(&dgentry[i], (size_t)seg_groups));
  }
  CallEvents ev;
  HIPCHK(ev.create());
  HIPCHK(hipMemcpyAsync(drows, rows, (size_t)NS * 16, hipMemcpyHostToDevice, h->stream));
  HIPCHK(hipMemsetAsync(dcarry, 0, 4, h->stream));       // the empty context
  HIPCHK(hipStreamSynchronize(h->stream));               // (the second stream reads both)
  double device_ms = 0.0;
  const int rc = run_slabs((int)T, seg, 2,
    [&](int i, int si, int start, int cnt) -> int {
      const hipStream_t st = si ? h->stream2 : h->stream;
      if (tmpl) HIPCHK(hipMemcpyAsync(dtmpl[si], tmpl + start, (size_t)cnt, hipMemcpyHostToDevice, st));
      HIPCHK(hipEventRecord(ev.t[si][0], st));
      bg::SampleArgs a;
      a.rows = drows; a.tmpl = tmpl ? dtmpl[si] : nullptr; a.out = dout[si];
      a.cmap = dcmap[si]; a.gmap = dgmap[si]; a.centry = dcentry[si]; a.gentry = dgentry[si]; a.carry = dcarry;
      a.n = cnt; a.pos0 = pos0 + start;
      a.chunks = ((int64_t)cnt + chunk - 1) / chunk; a.groups = (a.chunks + bg::GROUP - 1) / bg::GROUP;
      a.chunk = chunk; a.seed_lo = (uint32_t)(seed & 0xffffffffu); a.seed_hi = (uint32_t)(seed >> 32);
      const hipEvent_t before = i > 0 ? ev.walk[si ^ 1] : nullptr;
      int r = CRBM_OK;
      switch (order) {
        case 0: r = bg_sample_launch<0>(h, a, st, before, ev.walk[si]); break;
        case 1: r = bg_sample_launch<1>(h, a, st, before, ev.walk[si]); break;
        case 2: r = bg_sample_launch<2>(h, a, st, before, ev.walk[si]); break;
        default: r = bg_sample_launch<3>(h, a, st, before, ev.walk[si]); break;
      }
      if (r) return r;
      HIPCHK(hipEventRecord(ev.t[si][1], st));
      return CRBM_OK;
    },
    [&](int, int si, int start, int cnt) -> int {
      const hipStream_t st = si ? h->stream2 : h->stream;
      HIPCHK(hipMemcpyAsync(out + start, dout[si], (size_t)cnt, hipMemcpyDeviceToHost, st));
      HIPCHK(hipStreamSynchronize(st));
      float ms = 0.f;
      HIPCHK(hipEventElapsedTime(&ms, ev.t[si][0], ev.t[si][1]));
      device_ms += ms;
      return CRBM_OK;
    },
    [&] { bg_drain(h); });
  if (rc) return rc;
  h->bg_ms = (float)device_ms;
  return CRBM_OK;
}

int crbm_background_ms(crbm_handle* h, float* ms) {
  if (!h || !ms) return CRBM_ERR_INVALID;
  *ms = h->bg_ms;
  return CRBM_OK;
}

}  // extern "C"

// ---- the analytic null (crbm_null.h): the handle lends its device, its main stream and its error string --------------
extern "C" {

int crbm_score_distribution(crbm_handle* h, const int32_t* q, int32_t R, int32_t M, int32_t order, const double* trans,
                            const double* init, int64_t G, double* pmf) {
  ENTER();
  null::Plan plan;
  if (const char* why = null::plan_or_refusal(q, R, M, order, trans, init, G, pmf, null::env_i64("CRBM_NULL_BYTES", null::BYTES_DEFAULT),
                                              null::env_i64("CRBM_NULL_TILE", null::TILE_DEFAULT), &plan))
    return fail(h, CRBM_ERR_INVALID, std::string("crbm_score_distribution: ") + why);
  h->null_ms = 0.f;
  const int NS = plan.contexts, variant = env_int("CRBM_NULL_VARIANT", null::VARIANT_DEFAULT), rpg = plan.rows_per_group;
  std::vector<null::Pred> table((size_t)NS * null::PREDS);
  null::build_table(order, trans, table.data());
  CallBufs s;
  int32_t *dq = nullptr, *dreach = nullptr;
  null::Pred* dtable = nullptr;
  double *dinit = nullptr, *state[2] = {nullptr, nullptr}, *dpmf = nullptr;
  HIPCHK(s.get(&dq, (size_t)R * M * 4));
  HIPCHK(s.get(&dreach, (size_t)R * (M + 1)));
  HIPCHK(s.get(&dtable, table.size()));
  HIPCHK(s.get(&dinit, (size_t)NS));
  HIPCHK(s.get(&state[0], (size_t)plan.state_elems));
  HIPCHK(s.get(&state[1], (size_t)plan.state_elems));
  HIPCHK(s.get(&dpmf, (size_t)rpg * (size_t)G));
  CallEvents ev;
  HIPCHK(ev.create());
  const hipStream_t st = h->stream;
  HIPCHK(hipMemcpyAsync(dq, q, (size_t)R * M * 16, hipMemcpyHostToDevice, st));
  HIPCHK(hipMemcpyAsync(dreach, plan.reach.data(), (size_t)R * (M + 1) * 4, hipMemcpyHostToDevice, st));
  HIPCHK(hipMemcpyAsync(dtable, table.data(), table.size() * sizeof(null::Pred), hipMemcpyHostToDevice, st));
  HIPCHK(hipMemcpyAsync(dinit, init, (size_t)NS * 8, hipMemcpyHostToDevice, st));
  double device_ms = 0.0;
  for (int row0 = 0; row0 < R; row0 += rpg) {
    const int rows = std::min(rpg, R - row0);
    HIPCHK(hipEventRecord(ev.t[0][0], st));
    null::EdgeArgs e;
    e.state = state[0]; e.init = dinit; e.pmf = dpmf; e.reach = dreach + (size_t)row0 * (M + 1);
    e.gmax = plan.gmax; e.G = G; e.M = M; e.tile = plan.tile; e.contexts = NS; e.rows = rows;
    hipLaunchKernelGGL(null::start_kernel, dim3((unsigned)grid_for((long)rows * NS, 256, 1 << 20)), dim3(256), 0, st, e);
    for (int j = 0; j < M; ++j) {
      null::Launch launches[2];
      const int n = null::step_launches(plan, q, M, order, variant, row0, rows, j, launches);
      for (int i = 0; i < n; ++i) {
        const null::Launch& l = launches[i];
        if (l.gy == 0) continue;
        null::StepArgs a;
        a.src = state[j & 1]; a.dst = state[(j & 1) ^ 1];
        a.q = dq + (size_t)row0 * M * 4; a.reach = e.reach; a.table = dtable;
        a.gmax = plan.gmax; a.M = M; a.j = j; a.tile = plan.tile; a.contexts = NS;
        a.ctx0 = l.ctx0; a.nctx = l.nctx; a.lds_width = l.lds_width;
        if (l.siblings) hipLaunchKernelGGL(null::step_siblings_kernel, dim3(l.gx, l.gy), dim3(l.block), l.lds, st, a);
        else hipLaunchKernelGGL(null::step_plain_kernel, dim3(l.gx, l.gy), dim3(l.block), 0, st, a);
      }
    }
    e.state = state[M & 1];
    const unsigned mtiles = (unsigned)((G + plan.tile - 1) / plan.tile);
    hipLaunchKernelGGL(null::marginal_kernel, dim3(mtiles, (unsigned)rows), dim3(null::block_for(plan.tile)), 0, st, e);
    HIPCHK(hipGetLastError());
    HIPCHK(hipEventRecord(ev.t[0][1], st));
    HIPCHK(hipMemcpyAsync(pmf + (size_t)row0 * (size_t)G, dpmf, (size_t)rows * (size_t)G * 8, hipMemcpyDeviceToHost, st));
    HIPCHK(hipStreamSynchronize(st));
    float ms = 0.f;
    HIPCHK(hipEventElapsedTime(&ms, ev.t[0][0], ev.t[0][1]));
    device_ms += ms;
  }
  h->null_ms = (float)device_ms;
  return CRBM_OK;
}

int crbm_null_ms(crbm_handle* h, float* ms) {
  if (!h || !ms) return CRBM_ERR_INVALID;
  *ms = h->null_ms;
  return CRBM_OK;
}

}  // extern "C"

// ---- motif comparison (crbm_compare.h): the handle lends its device, its main stream and its error string -------------
namespace {

// The three stages for every group of queries.  null_of >= 0: crbm_motif_compare_null -- stages one and two only, the
// counters and tables of the single query copied out.
int compare_run(crbm_handle* h, const compare::Plan& plan, const uint16_t* qcols, const int32_t* qstart, int32_t K, const uint16_t* tcols,
                const int32_t* tstart, int32_t N, int32_t bins, int32_t both, int32_t min_overlap, double invC, double* p_min,
                int32_t* offset, int8_t* strand, int32_t* overlap, int32_t* n_off, uint32_t* counts_out, double* tail_out) {
  for (float& ms : h->compare_ms) ms = 0.f;
  const bool place = counts_out == nullptr;
  CallBufs s;
  uint2 *dq = nullptr, *dt = nullptr;
  int32_t *dqs = nullptr, *dts = nullptr, *doff = nullptr, *dovl = nullptr, *dnoff = nullptr;
  int64_t* dbase = nullptr;
  uint32_t* dcounts = nullptr;
  double *dtables = nullptr, *dp = nullptr;
  int8_t* dstrand = nullptr;
  const size_t rows_out = place ? (size_t)plan.rows_max * (size_t)N : 1;
  HIPCHK(s.get(&dq, (size_t)qstart[K]));
  HIPCHK(s.get(&dt, (size_t)plan.tcols));
  HIPCHK(s.get(&dqs, (size_t)K + 1));
  HIPCHK(s.get(&dts, (size_t)N + 1));
  HIPCHK(s.get(&dbase, (size_t)K));
  HIPCHK(s.get(&dcounts, (size_t)plan.count_elems_max));
  HIPCHK(s.get(&dtables, (size_t)plan.table_elems_max));
  HIPCHK(s.get(&dp, rows_out));
  HIPCHK(s.get(&doff, rows_out));
  HIPCHK(s.get(&dstrand, rows_out));
  HIPCHK(s.get(&dovl, rows_out));
  HIPCHK(s.get(&dnoff, rows_out));
  CallEvents ev;
  HIPCHK(ev.create());
  const hipEvent_t mark[4] = {ev.t[0][0], ev.t[0][1], ev.t[1][0], ev.t[1][1]};
  const hipStream_t st = h->stream;
  HIPCHK(hipMemcpyAsync(dq, qcols, (size_t)qstart[K] * 8, hipMemcpyHostToDevice, st));
  HIPCHK(hipMemcpyAsync(dt, tcols, (size_t)plan.tcols * 8, hipMemcpyHostToDevice, st));
  HIPCHK(hipMemcpyAsync(dqs, qstart, ((size_t)K + 1) * 4, hipMemcpyHostToDevice, st));
  HIPCHK(hipMemcpyAsync(dts, tstart, ((size_t)N + 1) * 4, hipMemcpyHostToDevice, st));
  HIPCHK(hipMemcpyAsync(dbase, plan.table_base.data(), (size_t)K * 8, hipMemcpyHostToDevice, st));
  HIPCHK(hipFuncSetAttribute(reinterpret_cast<const void*>(compare::counts_kernel), hipFuncAttributeMaxDynamicSharedMemorySize,
                             (int)compare::counts_lds(compare::MAX_WIDTH, compare::MAX_BINS)));
  const compare::Motifs motifs{dq, dqs, dt, dts};
  double total[4] = {0.0, 0.0, 0.0, 0.0};
  for (int g = 0; g < plan.groups(); ++g) {
    const int q0 = plan.group_start[(size_t)g], rows = plan.group_start[(size_t)g + 1] - q0;
    const int wq = compare::widest(qstart, q0, q0 + rows);
    const size_t ncounts = (size_t)(qstart[q0 + rows] - qstart[q0]) * (size_t)bins;
    HIPCHK(hipEventRecord(mark[0], st));
    HIPCHK(hipMemsetAsync(dcounts, 0, ncounts * 4, st));
    compare::CountArgs c;
    c.m = motifs; c.counts = dcounts; c.tcols = plan.tcols; c.q0 = q0; c.bins = bins; c.both = both;
    hipLaunchKernelGGL(compare::counts_kernel, dim3(compare::count_blocks(plan.tcols), (unsigned)rows), dim3(256),
                       compare::counts_lds(wq, bins), st, c);
    HIPCHK(hipGetLastError());
    HIPCHK(hipEventRecord(mark[1], st));
    compare::NullArgs n;
    n.qstart = dqs; n.counts = dcounts; n.tables = dtables; n.table_base = dbase; n.invC = invC; n.q0 = q0; n.bins = bins; n.l = 0; n.tiles = 0;
    for (int l = 1; l <= wq; ++l) {
      n.l = l;
      n.tiles = (int32_t)compare::conv_tiles(bins, l);
      hipLaunchKernelGGL(compare::conv_kernel, dim3((unsigned)(n.tiles * (wq - l + 1)), (unsigned)rows), dim3(256),
                         compare::conv_lds(bins), st, n);
    }
    hipLaunchKernelGGL(compare::tail_kernel, dim3((unsigned)((wq * (wq + 1) / 2 + 63) / 64), (unsigned)rows), dim3(64), 0, st, n);
    HIPCHK(hipGetLastError());
    HIPCHK(hipEventRecord(mark[2], st));
    if (place) {
      compare::PlaceArgs a;
      a.m = motifs; a.tables = dtables; a.table_base = dbase;
      a.p_min = dp; a.offset = doff; a.strand = dstrand; a.overlap = dovl; a.n_off = dnoff;
      a.q0 = q0; a.N = N; a.bins = bins; a.both = both; a.min_overlap = min_overlap; a.tile = plan.tile;
      a.diagonals = wq + plan.width_max_targets - 1;
      hipLaunchKernelGGL(compare::place_kernel, dim3((unsigned)((N + plan.tile - 1) / plan.tile), (unsigned)rows), dim3(256),
                         compare::place_lds(plan.tile, a.diagonals), st, a);
      HIPCHK(hipGetLastError());
    }
    HIPCHK(hipEventRecord(mark[3], st));
    if (place) {
      const size_t at = (size_t)q0 * (size_t)N, cnt = (size_t)rows * (size_t)N;
      HIPCHK(hipMemcpyAsync(p_min + at, dp, cnt * 8, hipMemcpyDeviceToHost, st));
      HIPCHK(hipMemcpyAsync(offset + at, doff, cnt * 4, hipMemcpyDeviceToHost, st));
      HIPCHK(hipMemcpyAsync(strand + at, dstrand, cnt, hipMemcpyDeviceToHost, st));
      HIPCHK(hipMemcpyAsync(overlap + at, dovl, cnt * 4, hipMemcpyDeviceToHost, st));
      HIPCHK(hipMemcpyAsync(n_off + at, dnoff, cnt * 4, hipMemcpyDeviceToHost, st));
    } else {
      HIPCHK(hipMemcpyAsync(counts_out, dcounts, ncounts * 4, hipMemcpyDeviceToHost, st));
      HIPCHK(hipMemcpyAsync(tail_out, dtables, (size_t)compare::table_elems(bins, qstart[1]) * 8, hipMemcpyDeviceToHost, st));
    }
    HIPCHK(hipStreamSynchronize(st));
    for (int i = 0; i < 3; ++i) {
      float ms = 0.f;
      HIPCHK(hipEventElapsedTime(&ms, mark[i], mark[i + 1]));
      total[i + 1] += ms;
      total[0] += ms;
    }
  }
  for (int i = 0; i < 4; ++i) h->compare_ms[i] = (float)total[i];
  return CRBM_OK;
}

}  // namespace

extern "C" {

int crbm_motif_compare(crbm_handle* h, const uint16_t* qcols, const int32_t* qstart, int32_t K, const uint16_t* tcols,
                       const int32_t* tstart, int32_t N, int32_t bins, int32_t both, int32_t min_overlap, double invC,
                       double* p_min, int32_t* offset, int8_t* strand, int32_t* overlap, int32_t* n_off) {
  ENTER();
  compare::Plan plan;
  if (const char* why = compare::plan_or_refusal(qcols, qstart, K, tcols, tstart, N, bins, both, min_overlap, invC,
                                                 p_min && offset && strand && overlap && n_off,
                                                 compare::env_i64("CRBM_COMPARE_BYTES", compare::BYTES_DEFAULT),
                                                 compare::env_i64("CRBM_COMPARE_TILE", compare::TILE_DEFAULT), &plan))
    return fail(h, CRBM_ERR_INVALID, std::string("crbm_motif_compare: ") + why);
  return compare_run(h, plan, qcols, qstart, K, tcols, tstart, N, bins, both, min_overlap, invC, p_min, offset, strand, overlap, n_off,
                     nullptr, nullptr);
}

int crbm_motif_compare_null(crbm_handle* h, const uint16_t* qcols, int32_t m, const uint16_t* tcols, const int32_t* tstart, int32_t N,
                            int32_t bins, int32_t both, double invC, uint32_t* counts, double* tail) {
  ENTER();
  const int32_t qstart[2] = {0, m};
  compare::Plan plan;
  if (const char* why = compare::plan_or_refusal(qcols, qstart, 1, tcols, tstart, N, bins, both, 1, invC, counts && tail,
                                                 compare::env_i64("CRBM_COMPARE_BYTES", compare::BYTES_DEFAULT),
                                                 compare::env_i64("CRBM_COMPARE_TILE", compare::TILE_DEFAULT), &plan))
    return fail(h, CRBM_ERR_INVALID, std::string("crbm_motif_compare_null: ") + why);
  return compare_run(h, plan, qcols, qstart, 1, tcols, tstart, N, bins, both, 1, invC, nullptr, nullptr, nullptr, nullptr, nullptr,
                     counts, tail);
}

int crbm_compare_ms(crbm_handle* h, float* ms, float* stage_ms) {
  if (!h || !ms) return CRBM_ERR_INVALID;
  *ms = h->compare_ms[0];
  if (stage_ms)
    for (int i = 0; i < 3; ++i) stage_ms[i] = h->compare_ms[i + 1];
  return CRBM_OK;
}

}  // extern "C"
