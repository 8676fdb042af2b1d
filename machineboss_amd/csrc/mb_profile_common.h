// mb_profile_common.h -- what the profile sweeps share (mb_profile.hip, mb_profile_merge.hip, mb_profile_pair.hip,
// mb_profile_pair_merge.hip, mb_profile_two.hip, mb_profile_two_merge.hip, mb_profile_post.hip): the reduction of a sweep's mode, the LDS a ring may take and the raising of its limit, the lanes of a workgroup, the reversal of a path, the
// accumulator of the posterior counts, the add of the row posteriors, and the generator and the draw of the path samplers
// (k_profile_pair_sample, k_profile_pair_merge_sample, k_profile_two_sample).  Device code: included by .hip files only.
#pragma once
#include <algorithm>
#include <initializer_list>
#include <type_traits>

#include "mb_device_math.h"
#include "mb_internal.h"

namespace mb {

static constexpr int SWEEP_THREADS = 1024;
static constexpr size_t SWEEP_LDS_MAX = 160 * 1024;      // a ring lives in LDS while it fits, else in global scratch
static constexpr int COUNTS_LDS_MAX = 8192;             // transitions a workgroup's LDS accumulators hold

template <int MODE>
__device__ __forceinline__ double red(double a, double b) { return MODE == MB_VITERBI ? dmax(a, b) : lse2_exact(a, b); }

// lanes of a workgroup whose busiest phase has maxItems work items: whole wavefronts, at least one
inline int sweep_threads(long long maxItems) { return (int)std::min<long long>(SWEEP_THREADS, std::max<long long>(64, (maxItems + 63) / 64 * 64)); }

// Beyond the default 64 KiB of dynamic LDS the kernels must be told: asked for once, and only when a ring needs it.  allowed: the
// caller's static, 64 KiB at first; kernels: every kernel of the caller that may get a ring that large; what: the error's context.
inline bool allow_sweep_lds(size_t &allowed, size_t lds, std::initializer_list<const void *> kernels, const char *what) {
  if (lds <= allowed) return true;
  for (const void *k : kernels)
    if (!hip_ok(hipFuncSetAttribute(k, hipFuncAttributeMaxDynamicSharedMemorySize, (int)SWEEP_LDS_MAX), what)) return false;
  allowed = SWEEP_LDS_MAX;
  return true;
}

template <class T>
__device__ __forceinline__ void swap_entries(T *a, long long u, long long v) { const T e = a[u]; a[u] = a[v]; a[v] = e; }
// A path that a traceback or a sampler wrote from its end, turned round in place: its edges, the rows they fired at and, where the
// input is a profile too, the input rows.
template <class... T>
__device__ __forceinline__ void reverse_path(long long cnt, T *...arrays) {
  for (long long u = 0, v = cnt - 1; u < v; ++u, --v) (swap_entries(arrays, u, v), ...);
}

// Posterior counts of one workgroup.  Partial counts are kept in the workgroup's LDS table (lds[COUNTS_LDS_MAX]) when the
// transition table is small and flushed once with atomics; beyond, every term goes to the global table.  det: both tables hold
// 64-bit fixed point at 2^-36 (mb_internal.h) -- integer adds commute, so the counts are the same bits from call to call.
struct CountsAcc {
  double *lds, *counts, *tab;
  long long nTrans;
  int det;
  bool useLds;
  // every lane of the workgroup: zeroes the LDS table
  __device__ __forceinline__ CountsAcc(double *lds, double *counts, long long nTrans, int det)
      : lds(lds), counts(counts), nTrans(nTrans), det(det), useLds(nTrans <= COUNTS_LDS_MAX) {
    if (useLds) {
      for (int e = threadIdx.x; e < nTrans; e += blockDim.x) lds[e] = 0.0;
      __syncthreads();
    }
    tab = useLds ? lds : counts;
  }
  __device__ __forceinline__ void add(uint32_t e, double c) const {
    if (c != 0.0) {
      if (det) atomicAdd((unsigned long long *)tab + e, (unsigned long long)fmin(fmax(c * MB_DET_GLOBAL_SCALE + 0.5, 0.0), 4611686018427387904.0));
      else atomicAdd(&tab[e], c);
    }
  }
  // every lane of the workgroup, after its last add
  __device__ __forceinline__ void flush() const {
    if (!useLds) return;
    __syncthreads();
    for (int e = threadIdx.x; e < nTrans; e += blockDim.x)
      if (det ? ((const unsigned long long *)lds)[e] != 0ull : lds[e] != 0.0) {
        if (det) atomicAdd((unsigned long long *)counts + e, ((const unsigned long long *)lds)[e]);
        else atomicAdd(&counts[e], lds[e]);
      }
  }
};

// One lane sum into bin `bin` of a row-posterior table (k_profile_pair_rowpost, k_profile_pair_merge_rowpost, k_profile_two_rowpost, k_profile_rowpost), every lane of the wavefront
// together.  whole: all 64 lanes hold items of one line, so the sums are reduced across the lanes and lane 0 alone adds; else every
// lane adds its own.  det: the lane sum becomes 64-bit fixed point at 2^-36 (mb_internal.h) before it meets another.
__device__ __forceinline__ void rowpost_add(double *tab, int bin, double v, bool whole, int lane, int det) {
  if (det) {
    unsigned long long u = (unsigned long long)fmin(fmax(v * MB_DET_GLOBAL_SCALE + 0.5, 0.0), 4611686018427387904.0);
    if (whole) {
      for (int w = 32; w > 0; w >>= 1) u += __shfl_xor(u, w);
      if (lane != 0) u = 0ull;
    }
    if (u != 0ull) atomicAdd((unsigned long long *)tab + bin, u);
  } else {
    if (whole) {
      for (int w = 32; w > 0; w >>= 1) v += __shfl_xor(v, w);
      if (lane != 0) v = 0.0;
    }
    if (v != 0.0) atomicAdd(&tab[bin], v);
  }
}

// Philox4x32-10 (Salmon et al., "Parallel random numbers: as easy as 1, 2, 3", SC'11) and the 53-bit uniform of its first two words,
// the recipe of the Mt19937 variates: ((x0 >> 5) * 2^26 + (x1 >> 6)) * 2^-53.  profile.philox4x32 / sample_uniform are the same text
// in numpy.
__device__ __forceinline__ double philox_uniform(uint32_t c0, uint32_t c1, uint32_t c2, uint32_t c3, uint32_t k0, uint32_t k1) {
  constexpr uint32_t M0 = 0xD2511F53u, M1 = 0xCD9E8D57u;
#pragma unroll
  for (int round = 0; round < 10; ++round) {
    const uint32_t hi0 = __umulhi(M0, c0), lo0 = M0 * c0, hi1 = __umulhi(M1, c2), lo1 = M1 * c2;
    c0 = hi1 ^ c1 ^ k0; c1 = lo1; c2 = hi0 ^ c3 ^ k1; c3 = lo0;
    k0 += 0x9E3779B9u; k1 += 0xBB67AE85u;
  }
  return ((double)(c0 >> 5) * 67108864.0 + (double)(c1 >> 6)) * (1.0 / 9007199254740992.0);
}

// One candidate of a sampling decision: p = exp(term - cur) joins the running sum; the first candidate whose sum passes u is taken,
// and the last one with p > 0 is remembered for the draw that rounding left above the total.
struct SampleDraw {
  double u, cur, acc = 0.0, term = 0.0;
  int a = -1, src = -1, kind = -1;      // the taken candidate: its CSR entry, source state and kind (the caller's numbering)
  bool done = false;
  __device__ __forceinline__ SampleDraw(double u, double cur) : u(u), cur(cur) {}
  __device__ __forceinline__ void offer(double t, int kind_, int a_, int src_) {
    if (done) return;
    const double p = exp(t - cur);
    acc += p;
    if (p > 0.0) { term = t; kind = kind_; a = a_; src = src_; }
    done = u < acc;      // (p > 0 here: the sum has just grown past u)
  }
};

}  // namespace mb
