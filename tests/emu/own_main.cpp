// TEST INFRASTRUCTURE: the owners of crbm_amd/csrc/crbm_own.h against counting stand-ins for the HIP calls they make;
// tests/test_own_host.py builds it with ASan + UBSan and runs it directly.  No HIP runtime is linked.
// usage: own_main <case>     (one of the names in `cases` below, or "all")
// The stand-ins hand out malloc'ed memory for allocations and tagged dummy handles for streams, events, code objects
// and mapped peer buffers, write every create and destroy into `journal`, refuse what was never handed out or has been
// released already, and fail the n-th call of a kind when told to (fail_nth).  Whatever case ran, the program ends with
// status 0 only if every live counter is back at zero and everything handed out has been released exactly once.
#include "crbm_own.h"

#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <map>
#include <set>
#include <string>
#include <thread>
#include <vector>

using namespace crbm;

// ---- the stand-ins -----------------------------------------------------------------------------------------------
enum Kind { MALLOC, MEMSET, STREAM, EVENT, MODULE, PEER, KINDS };
static std::vector<std::string> journal;            // "malloc 704", "free", "stream+ 1", "sync 1", "stream- 1", ...
static std::map<void*, size_t> blocks;              // live allocations and their bytes
static std::set<uintptr_t> handles[KINDS];          // live dummy handles
static long calls[KINDS], fail_nth[KINDS];          // calls of a kind so far; the call of this number fails (0: none)
static long released_twice = 0, next_tag = 1;

static void note(const std::string& what, long tag = -1) { journal.push_back(tag < 0 ? what : what + " " + std::to_string(tag)); }
static bool fails(Kind k) { return ++calls[k] == fail_nth[k]; }
static void fail_next(Kind k, long n = 1) { fail_nth[k] = calls[k] + n; }

template <typename H>
static hipError_t make(Kind k, const char* name, H* out) {
  if (fails(k)) return hipErrorOutOfMemory;
  const uintptr_t tag = (uintptr_t)next_tag++;
  handles[k].insert(tag);
  *out = reinterpret_cast<H>(tag);
  note(std::string(name) + "+", (long)tag);
  return hipSuccess;
}
template <typename H>
static hipError_t end(Kind k, const char* name, H h) {
  const uintptr_t tag = reinterpret_cast<uintptr_t>(h);
  if (!handles[k].erase(tag)) { ++released_twice; return 1; }
  note(std::string(name) + "-", (long)tag);
  return hipSuccess;
}

hipError_t hipMalloc(void** p, size_t bytes) {
  *p = reinterpret_cast<void*>(0x1);               // (what a failed call leaves behind must not be used)
  if (fails(MALLOC)) return hipErrorOutOfMemory;
  *p = malloc(bytes ? bytes : 1);
  memset(*p, 0xAB, bytes);
  blocks[*p] = bytes;
  note("malloc", (long)bytes);
  return hipSuccess;
}
hipError_t hipExtMallocWithFlags(void** p, size_t bytes, unsigned flags) {
  const hipError_t e = flags == hipDeviceMallocFinegrained ? hipMalloc(p, bytes) : 1;
  if (e == hipSuccess) journal.back() = "malloc-fine " + std::to_string(bytes);
  return e;
}
hipError_t hipMemset(void* p, int value, size_t bytes) {
  if (fails(MEMSET)) return 1;
  if (!blocks.count(p) || blocks[p] < bytes) { fprintf(stderr, "hipMemset outside a live block\n"); exit(1); }
  memset(p, value, bytes);
  return hipSuccess;
}
hipError_t hipFree(void* p) {
  if (!blocks.erase(p)) { ++released_twice; return 1; }
  free(p);
  note("free");
  return hipSuccess;
}
hipError_t hipStreamCreateWithFlags(hipStream_t* s, unsigned flags) { return flags == hipStreamNonBlocking ? make(STREAM, "stream", s) : 1; }
hipError_t hipStreamSynchronize(hipStream_t s) {
  if (!handles[STREAM].count(reinterpret_cast<uintptr_t>(s))) { ++released_twice; return 1; }
  note("sync", (long)reinterpret_cast<uintptr_t>(s));
  return hipSuccess;
}
hipError_t hipStreamDestroy(hipStream_t s) { return end(STREAM, "stream", s); }
hipError_t hipEventCreate(hipEvent_t* e) { return make(EVENT, "event", e); }
hipError_t hipEventCreateWithFlags(hipEvent_t* e, unsigned flags) { return flags == hipEventDisableTiming ? make(EVENT, "event-untimed", e) : 1; }
hipError_t hipEventDestroy(hipEvent_t e) { return end(EVENT, "event", e); }
hipError_t hipModuleLoadData(hipModule_t* m, const void* image) { return image ? make(MODULE, "module", m) : 1; }
hipError_t hipModuleUnload(hipModule_t m) { return end(MODULE, "module", m); }
hipError_t hipIpcOpenMemHandle(void** p, hipIpcMemHandle_t, unsigned flags) { return flags == hipIpcMemLazyEnablePeerAccess ? make(PEER, "peer", p) : 1; }
hipError_t hipIpcCloseMemHandle(void* p) { return end(PEER, "peer", p); }

// ---- the checks --------------------------------------------------------------------------------------------------
#define REQUIRE(cond)                                                          \
  do {                                                                         \
    if (!(cond)) {                                                             \
      fprintf(stderr, "%s:%d: REQUIRE(%s) failed\n", __FILE__, __LINE__, #cond); \
      for (const auto& j : journal) fprintf(stderr, "  %s\n", j.c_str());      \
      exit(1);                                                                 \
    }                                                                          \
  } while (0)

struct Counts {
  long long v[LIVE_KINDS];
  bool operator==(const Counts& o) const { return !memcmp(v, o.v, sizeof(v)); }
};
static const Counts NOTHING = {{0, 0, 0, 0, 0}};
static Counts counts() {
  Counts c;
  for (int i = 0; i < LIVE_KINDS; ++i) c.v[i] = live(i).load();
  return c;
}
// the counters say what the stand-ins hold
static void counters_match() {
  long long bytes = 0;
  for (const auto& b : blocks) bytes += (long long)b.second;
  const Counts c = counts();
  REQUIRE(c.v[LIVE_BUFFERS] == (long long)blocks.size() && c.v[LIVE_BYTES] == bytes);
  REQUIRE(c.v[LIVE_STREAMS] == (long long)handles[STREAM].size() && c.v[LIVE_EVENTS] == (long long)handles[EVENT].size());
  REQUIRE(c.v[LIVE_MODULES] == (long long)handles[MODULE].size());
}
static long count_of(const std::string& prefix) {
  long n = 0;
  for (const auto& j : journal) n += j.compare(0, prefix.size(), prefix) == 0;
  return n;
}
static long where(const std::string& entry) {
  for (size_t i = 0; i < journal.size(); ++i)
    if (journal[i] == entry) return (long)i;
  return -1;
}

static void ensure_grows_by_the_rule() {
  DevBuf<float> b;
  REQUIRE(b.ensure(100) == hipSuccess && b.cap == 100 + 100 / 8 + 64 && b.p);
  REQUIRE(journal.back() == "malloc " + std::to_string(176 * sizeof(float)));
  float* first = b.p;
  REQUIRE(b.ensure(176) == hipSuccess && b.p == first && count_of("malloc") == 1);          // fits: nothing happens
  REQUIRE(b.ensure(177) == hipSuccess && b.cap == 177 + 177 / 8 + 64);
  REQUIRE(count_of("malloc") == 2 && count_of("free") == 1 && !blocks.count(first));       // the old block is gone
  REQUIRE(where("free") < where("malloc " + std::to_string(b.cap * sizeof(float))));       // ... before the new one comes
  counters_match();
  REQUIRE(counts().v[LIVE_BUFFERS] == 1 && counts().v[LIVE_BYTES] == (long long)(b.cap * sizeof(float)));
  DevBuf<unsigned long long> wide;
  REQUIRE(wide.ensure(0) == hipSuccess && !wide.p && wide.cap == 0 && count_of("malloc") == 2);   // nothing asked, nothing taken
  REQUIRE(wide.ensure(1) == hipSuccess && wide.cap == 65 && journal.back() == "malloc 520");
}

static void failed_ensure_leaves_the_owner_empty() {
  DevBuf<int> b;
  REQUIRE(b.ensure(10) == hipSuccess);
  fail_next(MALLOC);
  REQUIRE(b.ensure(1000) != hipSuccess && b.p == nullptr && b.cap == 0);
  REQUIRE(blocks.empty() && counts() == NOTHING);
  REQUIRE(b.ensure(5) == hipSuccess && b.cap == 69);                                         // and serves again
  fail_next(MALLOC);
  DevBuf<int> c;
  REQUIRE(c.alloc(8) != hipSuccess && !c.p && !c.cap);
  fail_next(MALLOC);
  REQUIRE(c.alloc(8, true) != hipSuccess && !c.p && !c.cap);
}

static void exact_zeroed_and_fine_grained() {
  DevBuf<uint32_t> b;
  REQUIRE(b.alloc_zeroed(7) == hipSuccess && b.cap == 7 && journal.back() == "malloc 28");
  for (int i = 0; i < 7; ++i) REQUIRE(b.p[i] == 0);
  REQUIRE(b.alloc(3) == hipSuccess && b.cap == 3 && blocks.size() == 1);                     // a second alloc lets the first go
  DevBuf<float> f;
  REQUIRE(f.alloc(33, true) == hipSuccess && f.cap == 33 && journal.back() == "malloc-fine 132");
  counters_match();
  fail_next(MEMSET);
  DevBuf<float> z;
  REQUIRE(z.alloc_zeroed(4) != hipSuccess && z.p && z.cap == 4);                             // the memset failed: still owned, freed below
  counters_match();
}

static void moves_leave_one_owner() {
  DevBuf<float> a;
  REQUIRE(a.ensure(10) == hipSuccess);
  float* pa = a.p;
  const size_t ca = a.cap;
  DevBuf<float> b(std::move(a));
  REQUIRE(!a.p && !a.cap && b.p == pa && b.cap == ca);
  DevBuf<float> c;
  REQUIRE(c.ensure(300) == hipSuccess);
  float* pc = c.p;
  c = std::move(b);                                   // what c held is freed, b is empty
  REQUIRE(!b.p && !b.cap && c.p == pa && c.cap == ca && !blocks.count(pc) && blocks.size() == 1);
  DevBuf<float> d;
  REQUIRE(d.alloc(5) == hipSuccess);
  float* pd = d.p;
  std::swap(c, d);
  REQUIRE(c.p == pd && c.cap == 5 && d.p == pa && d.cap == ca && blocks.size() == 2);
  c.swap(d);                                          // (swap_param_sets: no call of the runtime, nothing counted)
  REQUIRE(c.p == pa && c.cap == ca && d.p == pd && d.cap == 5 && blocks.size() == 2 && count_of("free") == 1);
  std::swap(c, d);
  REQUIRE(c.p == pd && d.p == pa && count_of("free") == 1);
  counters_match();
  Stream s, t;
  REQUIRE(s.create() == hipSuccess);
  const hipStream_t raw = s;
  t = std::move(s);
  REQUIRE(!static_cast<hipStream_t>(s) && static_cast<hipStream_t>(t) == raw && handles[STREAM].size() == 1);
  Stream u(std::move(t));
  REQUIRE(!static_cast<hipStream_t>(t) && static_cast<hipStream_t>(u) == raw);
  Event e, f;
  REQUIRE(e.create() == hipSuccess && f.create_untimed() == hipSuccess);
  REQUIRE(journal[journal.size() - 2].compare(0, 7, "event+ ") == 0 && journal.back().compare(0, 15, "event-untimed+ ") == 0);
  const hipEvent_t re = e, rf = f;
  std::swap(e, f);
  REQUIRE(static_cast<hipEvent_t>(e) == rf && static_cast<hipEvent_t>(f) == re && handles[EVENT].size() == 2);
  f = Event();                                        // a reset: the event goes now
  REQUIRE(!static_cast<hipEvent_t>(f) && handles[EVENT].size() == 1);
  counters_match();
}

static void release_then_destruction_frees_once() {
  {
    DevBuf<float> a;
    REQUIRE(a.ensure(10) == hipSuccess);
    a.release();
    REQUIRE(!a.p && !a.cap && count_of("free") == 1 && blocks.empty());
    a.release();
    Module m;
    const char image[4] = {1, 2, 3, 4};
    REQUIRE(m.load(image) == hipSuccess && handles[MODULE].size() == 1);
    m.reset();
    m.reset();
    REQUIRE(handles[MODULE].empty());
    fail_next(MODULE);
    REQUIRE(m.load(image) != hipSuccess && !static_cast<hipModule_t>(m));
  }
  REQUIRE(count_of("free") == 1 && count_of("module-") == 1 && released_twice == 0);
}

// laid out like the partition state of crbm_api.hip: the event, the stream, the thread that enqueues on the stream
struct Worker {
  std::thread th;
  explicit Worker(hipStream_t s) : th([s] { REQUIRE(hipStreamSynchronize(s) == hipSuccess); }) {}
  ~Worker() { th.join(); note("join"); }
};
struct PartitionLike {
  Event done;
  Stream stream;
  std::unique_ptr<Worker> worker;
};
static void partition_goes_thread_then_stream_then_event() {
  Stream main_stream;
  REQUIRE(main_stream.create() == hipSuccess);
  const long main_tag = (long)reinterpret_cast<uintptr_t>(static_cast<hipStream_t>(main_stream));
  long s_tag = 0, e_tag = 0;
  {
    PartitionLike part[2];                            // [0] is the caller's thread on the main stream: it owns nothing
    REQUIRE(part[1].stream.create() == hipSuccess && part[1].done.create() == hipSuccess);
    s_tag = (long)reinterpret_cast<uintptr_t>(static_cast<hipStream_t>(part[1].stream));
    e_tag = (long)reinterpret_cast<uintptr_t>(static_cast<hipEvent_t>(part[1].done));
    part[1].worker.reset(new Worker(part[1].stream));
  }
  const long join = where("join"), sync = journal.size() - 3;
  REQUIRE(join >= 0 && journal[sync] == "sync " + std::to_string(s_tag) && join < sync);   // (the thread's own sync may come before the join)
  REQUIRE(journal[sync + 1] == "stream- " + std::to_string(s_tag) && journal[sync + 2] == "event- " + std::to_string(e_tag));
  REQUIRE(handles[STREAM].size() == 1 && handles[STREAM].count((uintptr_t)main_tag));        // the main stream survives
  REQUIRE(where("stream- " + std::to_string(main_tag)) < 0);
  counters_match();
}

// a function that returns early the way HIPCHK does, holding owners of every kind
#define CHK(expr)                         \
  do {                                    \
    if ((expr) != hipSuccess) return -1;  \
  } while (0)
static int early_returns() {
  DevBuf<float> a, b;
  Stream s;
  Event e[2];
  Module m;
  PeerMaps<4> peers;
  const char image[1] = {0};
  CHK(a.ensure(100));
  CHK(s.create());
  CHK(e[0].create());
  CHK(b.alloc_zeroed(50));
  CHK(m.load(image));
  CHK(e[1].create_untimed());
  peers.set_own(2, a.p);
  CHK(peers.open(0, hipIpcMemHandle_t()));
  CHK(a.ensure(1000));
  CHK(peers.open(1, hipIpcMemHandle_t()));
  return 0;
}
static void early_return_frees_what_the_function_held() {
  DevBuf<char> outside;                               // something live around the calls
  REQUIRE(outside.alloc(3) == hipSuccess);
  const Counts before = counts();
  const struct { Kind k; long calls_in_function; } kinds[] = {{MALLOC, 3}, {MEMSET, 1}, {STREAM, 1}, {EVENT, 2}, {MODULE, 1}, {PEER, 2}};
  for (const auto& kind : kinds)
    for (long n = 1; n <= kind.calls_in_function; ++n) {
      fail_next(kind.k, n);
      REQUIRE(early_returns() == -1);
      REQUIRE(counts() == before && blocks.size() == 1 && handles[STREAM].empty() && handles[EVENT].empty() &&
              handles[MODULE].empty() && handles[PEER].empty());
    }
  REQUIRE(early_returns() == 0 && counts() == before && blocks.size() == 1 && handles[PEER].empty());
}

static void peers_close_what_was_opened_and_not_the_own_buffer() {
  DevBuf<float> own;
  REQUIRE(own.alloc(16) == hipSuccess);
  {
    PeerMaps<8> peers;
    for (int r = 0; r < 4; ++r) {
      if (r == 2) peers.set_own(r, own.p);
      else REQUIRE(peers.open(r, hipIpcMemHandle_t()) == hipSuccess);
    }
    REQUIRE(peers[2] == own.p && peers[0] && peers[3] && !peers[4] && handles[PEER].size() == 3);
    peers.close();                                    // crbm_ipc_detach
    REQUIRE(handles[PEER].empty() && !peers[0] && !peers[2] && count_of("peer-") == 3 && blocks.size() == 1);
    REQUIRE(peers.open(1, hipIpcMemHandle_t()) == hipSuccess && peers.open(1, hipIpcMemHandle_t()) == hipSuccess);
    REQUIRE(handles[PEER].size() == 1);               // mapped again over itself: the first mapping was closed
    fail_next(PEER);
    REQUIRE(peers.open(5, hipIpcMemHandle_t()) != hipSuccess && !peers[5]);
  }
  REQUIRE(handles[PEER].empty() && blocks.size() == 1 && released_twice == 0);                // destruction closes the rest
}

int main(int argc, char** argv) {
  const struct { const char* name; void (*run)(); } cases[] = {
      {"ensure_grows_by_the_rule", ensure_grows_by_the_rule},
      {"failed_ensure_leaves_the_owner_empty", failed_ensure_leaves_the_owner_empty},
      {"exact_zeroed_and_fine_grained", exact_zeroed_and_fine_grained},
      {"moves_leave_one_owner", moves_leave_one_owner},
      {"release_then_destruction_frees_once", release_then_destruction_frees_once},
      {"partition_goes_thread_then_stream_then_event", partition_goes_thread_then_stream_then_event},
      {"early_return_frees_what_the_function_held", early_return_frees_what_the_function_held},
      {"peers_close_what_was_opened_and_not_the_own_buffer", peers_close_what_was_opened_and_not_the_own_buffer}};
  const std::string want = argc > 1 ? argv[1] : "all";
  int ran = 0;
  for (const auto& c : cases) {
    if (want != "all" && want != c.name) continue;
    journal.clear();
    c.run();
    ++ran;
    // at the end of every case: nothing is live, nothing was released twice, every block that came was freed
    REQUIRE(counts() == NOTHING);
    REQUIRE(blocks.empty() && released_twice == 0 && count_of("malloc") == count_of("free"));
    for (int k = 0; k < KINDS; ++k) REQUIRE(handles[k].empty());
    printf("ok %s\n", c.name);
  }
  if (!ran) { fprintf(stderr, "no such case: %s\n", want.c_str()); return 2; }
  return 0;
}
