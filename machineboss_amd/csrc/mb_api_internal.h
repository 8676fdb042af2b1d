// mb_api_internal.h -- what the host-side translation units of the C-ABI share (mb_api.hip, mb_profile_api.hip, mb_debug_api.hip).
// Host orchestration only: the kernels include mb_internal.h, never this.
#pragma once
#include <algorithm>
#include <cstring>
#include <vector>

#include "mb_internal.h"
#include "mb_profile_lattice.h"      // env_overlapping

namespace mb {

// Every entry point that touches the process-wide state holds one of these (mb_api.hip: one recursive lock; the outermost
// entry also un-pins the workspaces of the previous call).
struct ApiGuard {
  ApiGuard();
  ~ApiGuard();
  ApiGuard(const ApiGuard &) = delete;
  ApiGuard &operator=(const ApiGuard &) = delete;
};

// the same lock without the "a new call begins" bookkeeping: option and introspection entry points (they touch the environment /
// the planners' process-wide state, which guarded calls of other threads read)
struct ApiLock {
  ApiLock();
  ~ApiLock();
  ApiLock(const ApiLock &) = delete;
  ApiLock &operator=(const ApiLock &) = delete;
};

int ensure_init();

extern thread_local double g_last_ms;
extern thread_local const char *g_last_kernel;

// HIP-event timing on the library stream
struct Timer {
  hipEvent_t a = nullptr, b = nullptr;
  bool ok = false;
  Timer() { ok = hipEventCreate(&a) == hipSuccess && hipEventCreate(&b) == hipSuccess; }
  ~Timer() { if (a) (void)hipEventDestroy(a); if (b) (void)hipEventDestroy(b); }
  void start() { if (ok) (void)hipEventRecord(a, g_stream); }
  double stop() {
    if (!ok) return 0.0;
    (void)hipEventRecord(b, g_stream);
    (void)hipEventSynchronize(b);
    float ms = 0.f;
    (void)hipEventElapsedTime(&ms, a, b);
    return ms;
  }
};

// items [p0, p1) of a batch, one round of launches
struct Chunk { long long p0, p1, cells; };

// device -> host copy into caller-owned (pageable) memory, staged through pinned buffers when it is large
int d2h_large(void *dst, const void *srcDev, size_t bytes);
// an error path is about to release what launched kernels may still read: wait for both streams
void quiesce_streams();

// ---- what the batch calls of every family share ----------------------------------------------------------------------------------
// A call-scoped device buffer of the small-block cache (sm_alloc), one element at the least; it goes back when the scope ends.
template <class T> struct SmBuf {
  T *p = nullptr;
  SmBuf() = default;
  SmBuf(const SmBuf &) = delete;
  SmBuf &operator=(const SmBuf &) = delete;
  ~SmBuf() { sm_free(p); }
  hipError_t alloc(long long n) { return sm_alloc((void **)&p, (size_t)std::max<long long>(n, 1) * sizeof(T)); }
  operator T *() const { return p; }
};

// n elements of a workspace slot (one at the least: a chunk of empty items still gets a pointer)
template <class T> T *ws_array(int slot, long long n) { return (T *)ws_get(slot, (size_t)std::max<long long>(n, 1) * sizeof(T)); }

// The launches of one chunk on the library stream: timed into g_last_ms, counted into g_last_launches.
struct Timed {
  Timer &tm;
  Timed(Timer &t, long long launches) : tm(t) { g_last_launches += launches; tm.start(); }
  ~Timed() { g_last_ms += tm.stop(); }
};

// The chunk loop of every batch call.  build(c, plan) packs the descriptors of chunk c into a fresh Plan (which frees them when it
// goes); body(c, plan, timer) takes the workspaces, launches under a Timed and copies the chunk's results out.  A failed body waits
// for the streams before the descriptors are released, and ends the loop.
template <class Plan, class Build, class Body>
int for_chunks(const std::vector<Chunk> &chunks, Build build, Body body) {
  Timer tm;
  for (const Chunk &c : chunks) {
    Plan pl;
    if (build(c, pl)) return 1;
    const int rc = body(c, pl, tm);
    if (rc) { quiesce_streams(); return rc; }
  }
  return 0;
}

// per-item log-likelihoods into dst[0..n)
inline int fetch_loglike(double *dst, const double *d_ll, long long n) {
  if (n <= 0) return 0;
  return hip_ok(hipMemcpy(dst, d_ll, (size_t)n * sizeof(double), hipMemcpyDeviceToHost), "D2H loglike") ? 0 : 1;
}

// MB_DETERMINISTIC: n global fixed-point accumulators (2^-36) as doubles, in place
inline int decode_fixed_point(double *v, long long n, const char *msg) {
  for (long long e = 0; e < n; ++e) {
    unsigned long long u; std::memcpy(&u, &v[e], 8);
    if (!det_to_double(u, v[e])) { set_error(msg); return 1; }
  }
  return 0;
}
constexpr const char *COUNT_RANGE_ERROR = "MB_DETERMINISTIC: a posterior count left the fixed-point range (6.7e7 per transition and call): split the batch or use the floating-point mode";

// The transition counts of a call: each chunk's device counts added on the host, then the call's tail.
struct CountSum {
  std::vector<double> total, hc;
  explicit CountSum(long long nT) : total((size_t)nT, 0.0), hc((size_t)nT) {}
  int add(const double *d_cc, bool fixedPoint) {
    const long long nT = (long long)total.size();
    if (nT && !hip_ok(hipMemcpy(hc.data(), d_cc, nT * sizeof(double), hipMemcpyDeviceToHost), "D2H counts")) return 1;
    if (fixedPoint && decode_fixed_point(hc.data(), nT, COUNT_RANGE_ERROR)) return 1;
    for (long long e = 0; e < nT; ++e) total[(size_t)e] += hc[(size_t)e];
    return 0;
  }
  void finish(const std::vector<double> &hll, double *counts, double *loglikeSum, double *loglike) const {
    for (size_t e = 0; e < total.size(); ++e) counts[e] += total[e];
    double s = 0.0;
    for (size_t k = 0; k < hll.size(); ++k) { s += hll[k]; if (loglike) loglike[k] = hll[k]; }
    if (loglikeSum) *loglikeSum += s;
  }
};

// argument checks of the profile entry points (mb_profile_api.hip), shared with the prefix search
bool profile_values_ok(const double *v, long long n);
bool merge_map_ok(const mb_machine *m, int32_t nCols, const int32_t *colTok);

// what the closure chooser of the tiled family minimises and what MB_MEDIUM_JIT_VERBOSE prints (mb_api.hip; mb_debug_api.hip)
struct MedProgram;
long long medium_program_cost(const MedProgram &P);

}  // namespace mb
