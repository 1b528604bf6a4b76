// Owners of the GPU resources the host code holds: device memory, streams, events, code objects and the buffers of peer
// ranks mapped into this process.  Each releases what it holds in its destructor, is move-only (a moved-from owner is
// empty) and hands the raw handle out for launches.  This is the only file of the library that frees a HIP resource.
// Every acquire and release is counted in process-wide relaxed atomics: what is live now (crbm_live_resources).  Host only.
#pragma once
#include <hip/hip_runtime_api.h>

#include <atomic>
#include <cstddef>
#include <memory>
#include <type_traits>
#include <utility>

namespace crbm {

enum LiveKind { LIVE_BUFFERS, LIVE_BYTES, LIVE_STREAMS, LIVE_EVENTS, LIVE_MODULES, LIVE_KINDS };
inline std::atomic<long long>& live(int kind) { static std::atomic<long long> c[LIVE_KINDS]; return c[kind]; }   // (static: zero)
inline void live_add(int kind, long long d) { live(kind).fetch_add(d, std::memory_order_relaxed); }

// Device memory of `cap` elements.  ensure() grows with head room and does not keep the contents; alloc() and
// alloc_zeroed() take exactly n elements (fine_grained: hipExtMallocWithFlags, memory coherent between agents).
template <typename T>
struct DevBuf {
  T* p = nullptr;
  size_t cap = 0;   // elements
  DevBuf() = default;
  DevBuf(const DevBuf&) = delete; DevBuf& operator=(const DevBuf&) = delete;
  DevBuf(DevBuf&& o) noexcept : p(std::exchange(o.p, nullptr)), cap(std::exchange(o.cap, 0)) {}
  DevBuf& operator=(DevBuf&& o) noexcept { DevBuf old(std::move(*this)); p = std::exchange(o.p, nullptr); cap = std::exchange(o.cap, 0); return *this; }
  ~DevBuf() { release(); }
  void swap(DevBuf& o) noexcept { std::swap(p, o.p); std::swap(cap, o.cap); }      // (two words: swap_param_sets runs in every training step)
  hipError_t alloc(size_t n, bool fine_grained = false) {
    release();
    void* q = nullptr;
    const hipError_t e = fine_grained ? hipExtMallocWithFlags(&q, n * sizeof(T), hipDeviceMallocFinegrained) : hipMalloc(&q, n * sizeof(T));
    if (e != hipSuccess || !q) return e;
    p = static_cast<T*>(q); cap = n;
    live_add(LIVE_BUFFERS, 1); live_add(LIVE_BYTES, (long long)(n * sizeof(T)));
    return e;
  }
  hipError_t alloc_zeroed(size_t n) { const hipError_t e = alloc(n); return e != hipSuccess ? e : hipMemset(p, 0, n * sizeof(T)); }
  hipError_t ensure(size_t n) { return n <= cap ? hipSuccess : alloc(n + n / 8 + 64); }
  void release() {
    if (!p) return;
    (void)hipFree(p);
    live_add(LIVE_BUFFERS, -1); live_add(LIVE_BYTES, -(long long)(cap * sizeof(T)));
    p = nullptr; cap = 0;
  }
};

// What Stream, Event and Module share: one raw handle in a unique_ptr (move-only, empty once moved from) whose deleter
// ends it with END and counts it down; launch sites read the owner as the raw handle.
template <typename H, int KIND, void (*END)(H)>
struct Owned {
  struct End { void operator()(H x) const { END(x); live_add(KIND, -1); } };
  std::unique_ptr<std::remove_pointer_t<H>, End> h;
  operator H() const { return h.get(); }
  void reset() { h.reset(); }
  hipError_t took(hipError_t e, const H* raw) {      // the result of the create call that wrote *raw (read here, after the call)
    if (e == hipSuccess) { h.reset(*raw); live_add(KIND, 1); }
    return e;
  }
};
// (a stream is synchronised before it is destroyed: what it still runs has then let go of the buffers, events and code
//  objects that are released after it)
inline void end_stream(hipStream_t s) { (void)hipStreamSynchronize(s); (void)hipStreamDestroy(s); }
inline void end_event(hipEvent_t e) { (void)hipEventDestroy(e); }
inline void end_module(hipModule_t m) { (void)hipModuleUnload(m); }
struct Stream : Owned<hipStream_t, LIVE_STREAMS, end_stream> {      // non-blocking
  hipError_t create() { hipStream_t s = nullptr; return took(hipStreamCreateWithFlags(&s, hipStreamNonBlocking), &s); }
};
struct Event : Owned<hipEvent_t, LIVE_EVENTS, end_event> {
  hipError_t create() { hipEvent_t e = nullptr; return took(hipEventCreate(&e), &e); }      // with timestamps
  hipError_t create_untimed() { hipEvent_t e = nullptr; return took(hipEventCreateWithFlags(&e, hipEventDisableTiming), &e); }
};
struct Module : Owned<hipModule_t, LIVE_MODULES, end_module> {
  hipError_t load(const void* image) { hipModule_t m = nullptr; return took(hipModuleLoadData(&m, image), &m); }
};

// The buffers of the ranks of a node as this process sees them.  The rank's own buffer sits in the table beside the
// mapped ones and belongs to somebody else (`own`); every other entry was opened here and is closed here.
template <int N>
struct PeerMaps {
  void* p[N] = {};
  const void* own = nullptr;
  PeerMaps() = default;
  PeerMaps(const PeerMaps&) = delete; PeerMaps& operator=(const PeerMaps&) = delete;
  ~PeerMaps() { close(); }
  void set_own(int r, void* buf) { drop(r); own = buf; p[r] = buf; }
  hipError_t open(int r, hipIpcMemHandle_t mh) {
    drop(r);
    const hipError_t e = hipIpcOpenMemHandle(&p[r], mh, hipIpcMemLazyEnablePeerAccess);
    if (e != hipSuccess) p[r] = nullptr;
    return e;
  }
  void close() { for (int r = 0; r < N; ++r) drop(r); }
  void* operator[](int r) const { return p[r]; }
  void drop(int r) {
    if (p[r] && p[r] != own) (void)hipIpcCloseMemHandle(p[r]);
    p[r] = nullptr;
  }
};

}  // namespace crbm
