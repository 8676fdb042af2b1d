// mb_api_internal.h -- what the host-side translation units of the C-ABI share (mb_api.hip, mb_profile_api.hip).
// Host orchestration only: the kernels include mb_internal.h, never this.
#pragma once
#include "mb_internal.h"

namespace mb {

// Every entry point that touches the process-wide state holds one of these (mb_api.hip: one recursive lock; the outermost
// entry also un-pins the workspaces of the previous call).
struct ApiGuard {
  ApiGuard();
  ~ApiGuard();
  ApiGuard(const ApiGuard &) = delete;
  ApiGuard &operator=(const ApiGuard &) = delete;
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
int env_int(const char *name, int dflt);

inline bool env_overlapping(long long s1, long long e1, long long s2, long long e2) { return !(s1 >= e2 || s2 >= e1); }

// argument checks of the profile entry points (mb_profile_api.hip), shared with the prefix search
bool profile_values_ok(const double *v, long long n);
bool merge_map_ok(const mb_machine *m, int32_t nCols, const int32_t *colTok);

}  // namespace mb
