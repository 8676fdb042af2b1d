// mb_api.hip -- implementation of the C-ABI declared in include/mbhip.h.
//
// Host orchestration only: device memory pools, chunking of a batch so that materialised matrices fit the HBM
// budget (288 GB per MI355X), kernel-family selection, HIP-event timing on the library stream.
#include <algorithm>
#include <chrono>
#include <cmath>
#include <cstring>
#include <functional>
#include <map>
#include <mutex>
#include <string>
#include <vector>

#include "mb_api_internal.h"
#include "mb_internal.h"
#include "mb_jit.h"
#include "mb_medium.h"
#include "mb_prefix.h"
#include "mb_small.h"
#include "mb_usage.h"
#include "mb_wide.h"
#include "mb_wide_jit.h"

namespace mb {

thread_local std::string g_err;
thread_local double g_last_ms = 0.0;
thread_local const char *g_last_kernel = "";
thread_local long long g_last_launches = 0;
hipStream_t g_stream = nullptr;
int g_kernel_choice = 0;
size_t g_mem_budget = 0;
static bool g_init = false;

void set_error(const std::string &msg) { g_err = msg; }

bool hip_ok(hipError_t e, const char *what) {
  if (e == hipSuccess) return true;
  g_err = std::string(what) + ": " + hipGetErrorString(e);
  return false;
}

// One lock for every entry point that touches the process-wide state (stream, workspaces, compiled programs): the reference
// has no threads on this path and the library is built for one host thread per process, but two threads calling in
// must not corrupt the pools.  The outermost entry also un-pins the workspaces of the previous call.
static std::recursive_mutex g_api_mutex;
static int g_api_depth = 0;
static void ws_begin_call();
ApiGuard::ApiGuard() { g_api_mutex.lock(); if (g_api_depth++ == 0) ws_begin_call(); }
ApiGuard::~ApiGuard() { --g_api_depth; g_api_mutex.unlock(); }
// the same lock without the "a new call begins" bookkeeping: option and introspection entry points
ApiLock::ApiLock() { g_api_mutex.lock(); }
ApiLock::~ApiLock() { g_api_mutex.unlock(); }
bool g_deterministic = false;
void latch_deterministic() { g_deterministic = opt_int<MB_DETERMINISTIC>() != 0; }
static int g_device = -1;   // device the library's stream and workspaces live on

int ensure_init() {
  if (g_init) return 0;
  int n = 0;
  if (hipGetDeviceCount(&n) != hipSuccess || n == 0) {
    set_error("no HIP device visible: the Machine Boss DP engine has no CPU fallback");
    return 1;
  }
  MB_HIP(hipGetDevice(&g_device));
  MB_HIP(hipStreamCreateWithFlags(&g_stream, hipStreamNonBlocking));
  g_init = true;
  return 0;
}

// Grow-only device workspaces, kept across calls so that steady-state batch calls do no hipMalloc/hipFree
// (a 200 GB hipMalloc costs far more than the kernels it feeds).  Slot 0/1: matrix pools, 2: halo columns.
struct Workspace { void *p = nullptr; size_t bytes = 0; bool pinned = false; bool held = false; };   // held: a live object owns the slot (prefix node pool)
static const int WS_SLOTS = 16;
static Workspace g_ws[WS_SLOTS];   // 0/1 matrix pools, 2 halo columns, 3..7 Viterbi path buffers, 8.. small-machine family, 15 prefix node pool

static size_t cached_bytes() { size_t t = 0; for (const Workspace &w : g_ws) t += w.bytes; return t; }
// what a call may take back from the cache: a held slot belongs to a live object
static size_t reclaimable_bytes() { size_t t = 0; for (const Workspace &w : g_ws) if (!w.held) t += w.bytes; return t; }

// A slot handed out during the current API call is pinned until the next call begins; growing one slot may release every
// unpinned one (a Viterbi batch that needs 80 % of HBM in slot 0 must be able to reclaim the Backward pool a previous
// count sweep left in slot 1 -- budget_bytes() counts cached bytes as available).
static void ws_begin_call() { for (Workspace &w : g_ws) w.pinned = false; }   // (declared above, next to ApiGuard)
// what the pools cost this process so far (mb_alloc_stats): a 200 GB hipMalloc / hipFree pair takes SECONDS, so a caller -- and the
// tests -- must be able to see that steady-state calls do none
struct AllocStats { long long allocs = 0, frees = 0, evictions = 0; unsigned long long bytes = 0; double ms = 0.0; };
static AllocStats g_alloc;
static void ws_free_slot(Workspace &w) {
  if (!w.p) return;
  const auto t0 = std::chrono::steady_clock::now();
  (void)hipFree(w.p);
  g_alloc.ms += std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
  ++g_alloc.frees;
  w.p = nullptr; w.bytes = 0;
}
static void ws_release_unpinned(int except) {
  for (int k = 0; k < WS_SLOTS; ++k) {
    Workspace &w = g_ws[k];
    if (k == except || w.pinned || w.held || !w.p) continue;
    ws_free_slot(w); ++g_alloc.evictions;
  }
}

size_t ws_bytes(int slot) { return g_ws[slot].p ? g_ws[slot].bytes : 0; }

void *ws_get(int slot, size_t bytes) {
  Workspace &w = g_ws[slot];
  w.pinned = true;
  if (w.bytes >= bytes && w.p) return w.p;
  ws_free_slot(w);
  const size_t want = std::max<size_t>(bytes, 256);
  size_t freeB = 0, totalB = 0;
  // an explicit budget (mb_set_memory_budget) bounds everything the library keeps; otherwise only a shortage evicts
  const bool over = g_mem_budget && cached_bytes() + want > g_mem_budget;
  if (over || (hipMemGetInfo(&freeB, &totalB) == hipSuccess && freeB < want + ((size_t)256 << 20))) ws_release_unpinned(slot);
  const auto t0 = std::chrono::steady_clock::now();
  hipError_t e = hipMalloc(&w.p, want);
  if (e != hipSuccess) {
    (void)hipGetLastError();
    ws_release_unpinned(slot);
    e = hipMalloc(&w.p, want);
  }
  g_alloc.ms += std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
  if (!hip_ok(e, "hipMalloc(workspace)")) { w.p = nullptr; return nullptr; }
  ++g_alloc.allocs; g_alloc.bytes += want;
  w.bytes = want;
  return w.p;
}

// Before a call takes SEVERAL large slots: a grow-only slot that an earlier call left far larger than this call needs (the 230 GB
// pipeline pool of a materialised Forward, then an E-step that wants 2 x 115 GB) would starve the other slot -- ws_get hands the big
// one out as it is, pins it, and the second request finds no memory.  When the growth the listed requests need does not fit beside
// what is allocated, the listed slots that are larger than their request are released first (one re-allocation, not a failure).
void ws_plan(int n, const int *slots, const size_t *bytes) {
  size_t growth = 0, reclaim = 0;
  for (int k = 0; k < n; ++k) {
    const Workspace &w = g_ws[slots[k]];
    if (!w.p || w.bytes < bytes[k]) { growth += std::max<size_t>(bytes[k], 256); reclaim += w.p ? w.bytes : 0; }
  }
  if (!growth) return;
  size_t freeB = 0, totalB = 0;
  if (hipMemGetInfo(&freeB, &totalB) != hipSuccess) { (void)hipGetLastError(); return; }
  if (freeB + reclaim >= growth + ((size_t)256 << 20)) return;
  for (int k = 0; k < n; ++k) {
    Workspace &w = g_ws[slots[k]];
    if (w.p && !w.pinned && w.bytes > bytes[k]) { ws_free_slot(w); ++g_alloc.evictions; }
  }
}

// Small per-call device buffers (pair descriptors, log-likelihoods, offsets): a hipMalloc / hipFree pair per call is
// normally microseconds but now and then tens of milliseconds (measured: 23 ms ahead of a 25 ms Viterbi batch), so freed
// blocks are kept by size class and handed out again.
struct SmallBlock { void *p; size_t bytes; };
static std::vector<SmallBlock> g_smallFree, g_smallLive;
hipError_t sm_alloc(void **out, size_t bytes) {
  size_t cls = 4096;
  while (cls < bytes) cls <<= 1;
  for (size_t k = 0; k < g_smallFree.size(); ++k)
    if (g_smallFree[k].bytes == cls) {
      *out = g_smallFree[k].p;
      g_smallLive.push_back(g_smallFree[k]);
      g_smallFree.erase(g_smallFree.begin() + k);
      return hipSuccess;
    }
  const hipError_t e = hipMalloc(out, cls);
  if (e == hipSuccess) g_smallLive.push_back({*out, cls});
  return e;
}
void sm_free(void *p) {
  if (!p) return;
  for (size_t k = 0; k < g_smallLive.size(); ++k)
    if (g_smallLive[k].p == p) {
      if (g_smallLive[k].bytes <= ((size_t)64 << 20) && g_smallFree.size() < 32) g_smallFree.push_back(g_smallLive[k]);
      else (void)hipFree(p);
      g_smallLive.erase(g_smallLive.begin() + k);
      return;
    }
  (void)hipFree(p);
}

// Large device -> host copies into caller-owned (pageable) memory go through two pinned staging buffers: a hipMemcpy
// straight into fresh pageable pages pins them on the fly, which now and then costs tens of milliseconds for a 15 MB
// path array; the staged copy runs at the PCIe rate and overlaps the host-side memcpy of chunk k with the DMA of k+1.
static void *g_pinned[2] = {nullptr, nullptr};
static const size_t PINNED_CHUNK = (size_t)8 << 20;
int d2h_large(void *dst, const void *srcDev, size_t bytes) {
  if (bytes < ((size_t)1 << 20)) {
    if (!hip_ok(hipMemcpyAsync(dst, srcDev, bytes, hipMemcpyDeviceToHost, g_stream), "D2H")) return 1;
    return hip_ok(hipStreamSynchronize(g_stream), "D2H") ? 0 : 1;
  }
  for (int k = 0; k < 2; ++k)
    if (!g_pinned[k] && !hip_ok(hipHostMalloc(&g_pinned[k], PINNED_CHUNK, hipHostMallocDefault), "hipHostMalloc(staging)")) return 1;
  hipEvent_t ev[2] = {nullptr, nullptr};
  for (int k = 0; k < 2; ++k) if (!hip_ok(hipEventCreateWithFlags(&ev[k], hipEventDisableTiming), "hipEventCreate")) return 1;
  const size_t nChunks = (bytes + PINNED_CHUNK - 1) / PINNED_CHUNK;
  int rc = 0;
  auto issue = [&](size_t c) {
    const size_t off = c * PINNED_CHUNK, n = std::min(PINNED_CHUNK, bytes - off);
    if (!hip_ok(hipMemcpyAsync(g_pinned[c & 1], (const char *)srcDev + off, n, hipMemcpyDeviceToHost, g_stream), "D2H (staged)")) return 1;
    return hip_ok(hipEventRecord(ev[c & 1], g_stream), "hipEventRecord") ? 0 : 1;
  };
  rc = issue(0);
  for (size_t c = 0; c < nChunks && !rc; ++c) {
    if (c + 1 < nChunks) rc = issue(c + 1);
    if (rc || !hip_ok(hipEventSynchronize(ev[c & 1]), "hipEventSynchronize")) { rc = 1; break; }
    const size_t off = c * PINNED_CHUNK, n = std::min(PINNED_CHUNK, bytes - off);
    std::memcpy((char *)dst + off, g_pinned[c & 1], n);
  }
  if (rc) (void)hipStreamSynchronize(g_stream);
  for (int k = 0; k < 2; ++k) (void)hipEventDestroy(ev[k]);
  return rc;
}

int h2d_large(void *dstDev, const void *src, size_t bytes) {
  if (bytes < ((size_t)256 << 10)) {
    if (!hip_ok(hipMemcpyAsync(dstDev, src, bytes, hipMemcpyHostToDevice, g_stream), "H2D")) return 1;
    return 0;   // small pageable copies are staged by the runtime itself before the call returns
  }
  for (int k = 0; k < 2; ++k)
    if (!g_pinned[k] && !hip_ok(hipHostMalloc(&g_pinned[k], PINNED_CHUNK, hipHostMallocDefault), "hipHostMalloc(staging)")) return 1;
  for (size_t off = 0, c = 0; off < bytes; off += PINNED_CHUNK, ++c) {
    const size_t n = std::min(PINNED_CHUNK, bytes - off);
    if (c >= 2 && !hip_ok(hipStreamSynchronize(g_stream), "H2D (staged)")) return 1;   // the buffer about to be overwritten has been read
    std::memcpy(g_pinned[c & 1], (const char *)src + off, n);
    if (!hip_ok(hipMemcpyAsync((char *)dstDev + off, g_pinned[c & 1], n, hipMemcpyHostToDevice, g_stream), "H2D (staged)")) return 1;
  }
  return hip_ok(hipStreamSynchronize(g_stream), "H2D (staged)") ? 0 : 1;
}

static void ws_release() {
  for (Workspace &w : g_ws) if (!w.held) ws_free_slot(w);
  for (SmallBlock &b : g_smallFree) (void)hipFree(b.p);
  g_smallFree.clear();
  for (int k = 0; k < 2; ++k) if (g_pinned[k]) { (void)hipHostFree(g_pinned[k]); g_pinned[k] = nullptr; }
}

size_t budget_bytes() {
  if (g_mem_budget) return g_mem_budget;
  size_t freeB = 0, totalB = 0;
  if (hipMemGetInfo(&freeB, &totalB) != hipSuccess) return (size_t)8 << 30;
  // STICKY: what is free + cached moves by megabytes from call to call (a batch's tokens, a machine's record tables, a small block
  // released), chunk sizes and the pipeline's pool follow the budget, and ws_get re-allocates a pool for a request that grew by ANY
  // amount -- a 230 GB hipFree + hipMalloc pair is seconds (round 5: 7.1 s of wall around 75 ms of kernels in every call that
  // alternated with the one-tape sweeps).  So the budget only ever follows the memory DOWN, or up by more than an eighth.
  // MB_MEM_FRACTION (default 0.90): the share of the device this process may fill -- several ranks on ONE device (the gloo dry runs of
  // bench.py / boss.py, or a host that co-locates processes) must not each claim it.  0.90 and not the earlier 0.80: BASELINE config 5's
  // E-step at 64 x 50 kb needs 2 x 129.6 GB of matrices, which 0.80 of a 309 GB device cuts into two chunks of 32 sequences (555 ms;
  // one chunk: 518 ms); what the library allocates outside the pools (tokens, programs, exchange buffers) is well under 1 GB
  static size_t sticky = 0;
  static double stickyFrac = 0.0;
  double frac = 0.90;
  { const double f = opt_real<MB_MEM_FRACTION>(); if (f > 0.0 && f <= 0.95) frac = f; }
  const size_t cur = (size_t)((double)(freeB + reclaimable_bytes()) * frac);
  if (!sticky || frac != stickyFrac || cur < sticky || cur > sticky + sticky / 8 || !opt_int<MB_POOL_STICKY>()) { sticky = cur; stickyFrac = frac; }
  return sticky;
}

// kernel launchers implemented in the kernel files
int launch_generic_fill(const mb_machine *, int, const PairDesc *, long long, const int *, const int *, double *, int, hipStream_t,
                        const int *, const int *);
int launch_fill_neg_inf(double *, long long, hipStream_t);
int launch_gather_loglike(const PairDesc *, long long, const double *, int, int, double *, hipStream_t);
int launch_generic_counts(const mb_machine *, const PairDesc *, long long, long long, const int *, const int *,
                          const double *, const double *, double *, hipStream_t);
int launch_compact_paths(const uint32_t *, const long long *, const long long *, const long long *, uint32_t *, long long, hipStream_t);
int launch_traceback(const mb_machine *, const PairDesc *, long long, const int *, const int *, const double *,
                     const long long *, uint32_t *, long long *, hipStream_t);
size_t traceback_bytes_lds(const mb_machine *, int);
int launch_traceback_bytes(const mb_machine *, const PairDesc *, long long, const int *, const int *, const unsigned char *, int, const double *,
                           const long long *, uint32_t *, long long *, hipStream_t);

// a second stream for work that is independent of what g_stream runs (created on first use; nullptr if that fails)
static hipStream_t second_stream() {
  static hipStream_t s2 = nullptr;
  static bool tried = false;
  if (!tried) { tried = true; if (hipStreamCreateWithFlags(&s2, hipStreamNonBlocking) != hipSuccess) s2 = nullptr; }
  return s2;
}

// an error path is about to release what launched kernels may still read: wait for both streams (their own errors are not news here)
void quiesce_streams() {
  if (hipStream_t s2 = second_stream()) (void)hipStreamSynchronize(s2);
  (void)hipStreamSynchronize(g_stream);
  (void)hipGetLastError();
}

static int device_cus() {
  static int cus = -1;
  if (cus < 0) {
    int dev = 0; hipDeviceProp_t prop;
    cus = (hipGetDevice(&dev) == hipSuccess && hipGetDeviceProperties(&prop, dev) == hipSuccess) ? prop.multiProcessorCount : 0;
  }
  return cus;
}

// Split [0,nPairs) into chunks whose matrices (nMatrices per pair, doubles) fit the budget.
static bool plan_chunks(const mb_batch *b, int nMatrices, std::vector<Chunk> &out, double bytesPerCell = 0.0) {
  const size_t budget = budget_bytes();
  long long maxCells = bytesPerCell > 0.0 ? (long long)((double)budget / bytesPerCell) : (long long)(budget / (8ull * nMatrices));
  // balance: the same number of chunks as a greedy fill needs, but of even size (a short last chunk would leave
  // most of the chip idle)
  if (b->totalCells > maxCells && maxCells > 0) {
    const long long nChunks = (b->totalCells + maxCells - 1) / maxCells;
    const long long even = (b->totalCells + nChunks - 1) / nChunks + b->maxPairCells;
    if (even < maxCells) maxCells = std::max(even, b->maxPairCells);
  }
  // (a chunk also closes when it has reached its even share of what is LEFT: 64 equal pairs in two chunks are 32 + 32, not 33 + 31 -- the
  //  one-tape E-step runs k = CUs / pairs workgroups per sequence, and 33 pairs get 3 where 32 get 4)
  long long p0 = 0, acc = 0, left = b->totalCells;
  long long chunksLeft = maxCells > 0 ? std::max<long long>(1, (b->totalCells + maxCells - 1) / maxCells) : 1;
  for (long long p = 0; p < b->nPairs; ++p) {
    const PairDesc &pd = b->pairs[p];
    const long long c = (long long)(pd.inLen + 1) * (pd.outLen + 1) * b->m->S;
    if (c > maxCells) {
      set_error("a single DP matrix (" + std::to_string(bytesPerCell > 0.0 ? (long long)((double)c * bytesPerCell) : c * 8ll * nMatrices) + " bytes) exceeds the device memory budget");
      return false;
    }
    const bool shareReached = chunksLeft > 1 && acc > 0 && (acc + c / 2) * chunksLeft > left + acc;      // (left + acc = cells from this chunk's start on)
    if (acc + c > maxCells || shareReached) { out.push_back({p0, p, acc}); p0 = p; acc = 0; chunksLeft = std::max<long long>(1, chunksLeft - 1); }
    acc += c; left -= c;
  }
  if (b->nPairs > p0) out.push_back({p0, b->nPairs, acc});
  return true;
}

// The PairDescs of a chunk with cellBase rebased to the chunk's pool, on the host and (owned) on the device.
struct DescPlan { SmBuf<PairDesc> d; std::vector<PairDesc> hp; };
// tbStride > 0: traceback bytes instead of cells -- cellBase = BYTE offset, tbStride bytes per supercell
static int upload_chunk_descs(const mb_batch *b, const Chunk &c, DescPlan &pl, int tbStride = 0) {
  pl.hp.assign(b->pairs.begin() + c.p0, b->pairs.begin() + c.p1);
  long long base = 0;
  for (auto &pd : pl.hp) { pd.cellBase = base; base += (long long)(pd.inLen + 1) * (pd.outLen + 1) * (tbStride > 0 ? tbStride : b->m->S); }
  MB_HIP(pl.d.alloc((long long)pl.hp.size()));
  if (!hip_ok(hipMemcpyAsync(pl.d, pl.hp.data(), pl.hp.size() * sizeof(PairDesc), hipMemcpyHostToDevice, g_stream), "H2D pair descriptors") ||
      !hip_ok(hipStreamSynchronize(g_stream), "H2D pair descriptors")) return 1;
  return 0;
}
static auto desc_build(const mb_batch *b, int tbStride = 0) { return [b, tbStride](const Chunk &c, DescPlan &pl) { return upload_chunk_descs(b, c, pl, tbStride); }; }

// launches outside a chunk loop, timed into g_last_ms on a timer of their own
template <class F> static int timed(F launches) { Timer tm; Timed t(tm, 0); return launches(); }
static void reset_last() { g_last_ms = 0.0; g_last_launches = 0; g_last_kernel = ""; }
// the token tape of a one-tape machine's batch
static const int *tape_of(const mb_batch *b) { return b->m->nOut ? b->d_out : b->d_in; }
// the batch's envelopes as the tiled family takes them (empty: none)
static MedEnv med_env(const mb_batch *b) {
  MedEnv me;
  if (b->hasEnv) { me.d_start = b->d_envStart; me.d_end = b->d_envEnd; me.h_start = b->h_envStart.data(); me.h_end = b->h_envEnd.data(); }
  return me;
}


// ---- kernel-family state attached to a machine ------------------------------------------------------------
struct FastState {
  bool tried = false, mediumOk = false;
  bool exactOk = false;      // one-tape machines: only the exact (levelled) tiled program is built, for Viterbi (onetape_tiled_viterbi)
  bool exactTried = false;
  int G = 0;
  // exact (leveled) programs: Viterbi and Forward with a custom start state; "sum" programs: Forward / Backward,
  // silent closure when it stays small, otherwise the exact program of that direction
  MedProgram fwdExact, fwdSum, bwdSum;
  MedGeom geoFE, geoFS, geoBS;
  // Viterbi with traceback bytes: the exact program itself, or -- when that one splits high-degree states -- an unsplit twin
  bool tbTried = false, tbOk = false;
  MedProgram fwdTb;
  MedGeom geoTb;
  // Forward fill fused with posterior counts (run-time specialised kernel only)
  bool countOk = false;
  MedProgram fwdCnt;
  MedGeom geoCnt;
  // large one-tape machines (mb_wide.hip): programs built on first use, rebuilt after a weight update
  WideProgram wFwd, wBwd, wVit;
  WideProgram wVitTb;        // ... the max program that keeps one traceback code per cell (`--align` without the fp64 matrix)
  bool wVitTbTried = false;
  WideCountPlan wCnt;        // posterior counts of one-tape machines (any size): lane = transition
  UsagePlan usage;           // tiled family: posterior counts as a third pass over two materialised matrices (mb_usage.hip)
  WideTbPlan wTb;            // Viterbi traceback of one-tape machines too large for the LDS edge tables of mb_generic.hip
  // machines with a handful of states (mb_small.cpp): lane = column, states in registers
  bool smallTried = false, smallOk = false;
  SmallProgram smF, smB;
};

// what the closure chooser minimises (fast_state) and what MB_MEDIUM_JIT_VERBOSE prints (mb_debug_jit_source): candidate slots + the
// price of a round and of a synchronisation point in slots (MB_MEDIUM_ROUND_COST, default 0; MB_MEDIUM_SYNC_COST, default 1)
long long medium_program_cost(const MedProgram &P) {
  const int syncCost = opt_int<MB_MEDIUM_SYNC_COST>(), roundCost = opt_int<MB_MEDIUM_ROUND_COST>();
  long long c = 0;
  for (const MedRoundInfo &ri : P.roundInfo) c += (long long)ri.slots.size() + roundCost + (ri.sync ? syncCost : 0);
  return c;
}

static FastState *fast_state(mb_machine *m) {
  if (!m->fast) m->fast = new FastState();
  FastState *f = (FastState *)m->fast;
  if (!f->tried) {
    f->tried = true;
    // tiny machines run with 8 columns per wavefront (8 lanes per supercell); 1-state machines stay generic
    if (m->S >= opt_int<MB_MEDIUM_MIN_STATES>() && m->S <= 4096 && !wide_applicable(m)) {
      const int wantG = opt_int<MB_MEDIUM_G>();
      int G = wantG;
      if (!medium_valid_G(G)) G = medium_default_G(m->S);
      f->G = G;
      long long nSilent = 0;
      for (long long e = 0; e < m->nTrans; ++e) nSilent += (m->inTok[e] == 0 && m->outTok[e] == 0);
      const bool wantClosure = opt_int<MB_MEDIUM_CLOSURE>() != 0;
      // The silent closure trades synchronisation points (one wave-level LDS round trip per silent level) for
      // candidates.  Closing ALL levels at once is right for psw2dna (10 levels, 146 silent edges -> 360 pairs), but on
      // machines whose silent sub-graph is deep and dense (protpsw.translate.dnapsw: 22 levels, 551 silent edges ->
      // 12 162 pairs) neither extreme is: the levels are closed in K groups, K chosen by a cost model
      // (candidate slots + 6 per synchronisation point), K = 0 meaning the levelled program.
      // (round 4: a synchronisation point is priced at ONE slot, not six -- since the rounds of a stage issue their loads together
      // (mb_medium_jit.cpp) the kernels are bound by vector issue, i.e. by candidates; measured on protpsw.translate.dnapsw: 12 level
      // groups with 54 slots beat 5 with 75, rolling Forward 398 -> 432 G cells/s, psw2dna's choice does not change)
      auto cost = [](const MedProgram &P) { return medium_program_cost(P); };
      // Beyond even level groups: explicit stage boundaries, grown greedily -- the cut that lowers the cost most is added
      // until none does (protpsw.translate.dnapsw, 22 levels: even K = 3 costs 86 slots, cuts at levels 7 and 14 cost 73;
      // psw2dna Backward: 96 -> 80 with one cut at level 2).  Returns K (0 = levelled) and fills `cuts` when cuts win.
      auto choose = [&](bool backward, std::vector<int> &cuts) {
        cuts.clear();
        int bestK = 0; long long best = -1;
        const int forced = opt_int<MB_MEDIUM_CLOSURE_STAGES>();
        if (forced >= 0) return forced;
        if (!wantClosure) return 0;
        const int nLev = backward ? m->nLevB : m->nLevF;
        const bool verbose = opt_present<MB_MEDIUM_JIT_VERBOSE>();
        auto tryBuild = [&](int K, const std::vector<int> &cs, long long &c) {
          MedProgram P; MedGeom g;
          medium_set_cuts(cs);
          const bool ok = medium_build_host(m, backward, K, G, P, g);
          medium_set_cuts({});
          if (!ok) return false;
          if (K && P.nPairs > 16 * nSilent + 4 * m->S) return false;      // record tables would not stay cache-resident
          c = cost(P);
          return true;
        };
        for (int K = 0; K <= std::min(std::max(nLev - 1, 1), 12); ++K) {
          long long c;
          if (!tryBuild(K, {}, c)) continue;
          if (verbose) fprintf(stderr, "[mbhip] %s program, closure stages %d: cost %lld\n", backward ? "backward" : "forward", K, c);
          if (best < 0 || c < best) { best = c; bestK = K; }
        }
        if (opt_int<MB_MEDIUM_CUTS_SEARCH>() && nLev > 2 && !opt_text<MB_MEDIUM_CUTS>()) {
          std::vector<int> cur;
          long long curCost;
          if (tryBuild(1, {}, curCost)) {
            const int step = std::max(1, (nLev - 2 + 31) / 32);
            for (int it = 0; it < 6; ++it) {
              int bestCut = -1; long long bestC = curCost;
              for (int c = 2; c < nLev; c += step) {
                if (std::find(cur.begin(), cur.end(), c) != cur.end()) continue;
                std::vector<int> t = cur; t.push_back(c);
                long long cc;
                if (tryBuild(1, t, cc) && cc < bestC) { bestC = cc; bestCut = c; }
              }
              if (bestCut < 0) break;
              cur.push_back(bestCut); curCost = bestC;
            }
            std::sort(cur.begin(), cur.end());
            if (verbose) { fprintf(stderr, "[mbhip] %s program, stage cuts at levels", backward ? "backward" : "forward"); for (int c : cur) fprintf(stderr, " %d", c); fprintf(stderr, ": cost %lld (even groups: %lld)\n", curCost, best); }
            if (!cur.empty() && (best < 0 || curCost < best)) { cuts = cur; return (int)cur.size() + 1; }
          }
        }
        return bestK;
      };
      std::vector<int> cutsFwd; int KFwd = 0;   // the Forward program's closure: the count program's fill rounds use the same
      auto buildWith = [&](bool backward, MedProgram &P, MedGeom &geo) {
        std::vector<int> cuts;
        const int K = choose(backward, cuts);
        if (!backward) { cutsFwd = cuts; KFwd = K; }
        medium_set_cuts(cuts);
        const bool okb = medium_build(m, backward, K, G, P, geo);
        medium_set_cuts({});
        return okb;
      };
      bool ok = medium_build(m, false, 0, G, f->fwdExact, f->geoFE);
      if (ok) ok = buildWith(false, f->fwdSum, f->geoFS);
      if (ok) ok = buildWith(true, f->bwdSum, f->geoBS);
      f->mediumOk = ok;
      f->exactOk = ok;
      if (ok && opt_int<MB_MEDIUM_COUNTS>()) {
        int Gc = opt_int<MB_MEDIUM_COUNT_G>();
        if (!medium_valid_G(Gc)) Gc = wantG ? G : medium_default_count_G(m->S);
        f->countOk = medium_build_count(m, Gc, f->fwdCnt, f->geoCnt, KFwd, cutsFwd);
      }
    }
  }
  return f;
}

// The small-machine family: preferred whenever the machine qualifies (mb_set_kernel: 0 auto, 2 forces it; 1 / 3 skip it).
static bool use_small(mb_machine *m) {
  if (g_kernel_choice == 1 || g_kernel_choice == 3) return false;
  if (!small_eligible(m)) return false;
  if (!m->fast) m->fast = new FastState();
  FastState *f = (FastState *)m->fast;
  if (!f->smallTried) {
    f->smallTried = true;
    if (opt_int<MB_SMALL>()) f->smallOk = small_build(m, false, f->smF) && small_build(m, true, f->smB);
  }
  return f->smallOk;
}

// the program of the traceback-byte Viterbi sweep of the tiled family (nullptr: the machine keeps the fp64 matrix)
static MedProgram *medium_tb_program(mb_machine *m, MedGeom **geo) {
  FastState *f = fast_state(m);
  if (!f->mediumOk) return nullptr;
  if (!f->fwdExact.hasSplits) { *geo = &f->geoFE; return medium_tb_eligible(m, f->fwdExact) ? &f->fwdExact : nullptr; }
  if (!f->tbTried) {
    f->tbTried = true;
    f->tbOk = medium_build_unsplit(m, f->G, f->fwdTb, f->geoTb) && medium_tb_eligible(m, f->fwdTb);
  }
  *geo = &f->geoTb;
  return f->tbOk ? &f->fwdTb : nullptr;
}

static bool use_medium(mb_machine *m) {
  if (g_kernel_choice == 1) return false;
  FastState *f = fast_state(m);
  if (g_kernel_choice == 3 && !f->mediumOk) return false;
  return f->mediumOk;
}

// the one-tape family: program of a direction / semiring, (re)built from the current weights when needed
static WideProgram *wide_program(mb_machine *m, int mode) {
  if (g_kernel_choice == 1 || !wide_applicable(m)) return nullptr;
  FastState *f = fast_state(m);
  WideProgram &P = mode == MB_VITERBI ? f->wVit : (mode == MB_BACKWARD ? f->wBwd : f->wFwd);
  if ((!P.ok || P.dirty) && !wide_build(m, mode == MB_BACKWARD, mode == MB_VITERBI, P)) return nullptr;
  return &P;
}

// One-tape machine of moderate size whose max program has no retimed form (762 states: retimed 44 G cells/s, tiles 32; 1268
// states: 73 vs 22): the log-sum-exp sweeps belong to the one-tape family, but its column-by-column Viterbi sweep walks the
// silent levels one record at a time (0.2 us per level), where the run-time specialised tile kernel has them as straight-line
// code (762 states: 32 vs 14.5 G cells/s, 1268 states: 22.8 vs 15.6).  Decided when a Viterbi fill asks, and again after a weight
// update: which edges are -inf decides whether the retimed form exists (they leave the retiming graph), so a machine can gain or
// lose it.  Callers that never run Viterbi build neither program.
static bool onetape_tiled_viterbi(mb_machine *m) {
  if (!wide_applicable(m) || g_kernel_choice == 1 || m->S > opt_int<MB_WIDE_VITERBI_MIN_STATES>()) return false;
  FastState *f = fast_state(m);
  WideProgram *W = wide_program(m, MB_VITERBI);      // (built on first use, rebuilt when the weights changed)
  if (W && W->retOk) return false;
  if (!f->exactTried) {
    f->exactTried = true;
    int G = opt_int<MB_MEDIUM_G>();
    if (!medium_valid_G(G)) G = medium_default_G(m->S);
    f->G = G;
    f->exactOk = medium_build(m, false, 0, G, f->fwdExact, f->geoFE);
  }
  return f->exactOk;
}

// One-tape machines, `--viterbi / --align` with paths: the retimed max sweep keeping ONE traceback code per cell (mb_wide.hip,
// WideProgram::tbCodes) -- nullptr when the machine has no such program (no retimed form, a fan-in beyond 256, more than 2^15
// states or 2^16 transitions, a silent transition i -> j with j <= i -- the self-loop on state 0 is the one the reference lets
// through: a candidate of its traceback but not of the fill --, MB_ONETAPE_TB=0): the fp64 matrix and its walkers take it then.
// Decided at the first call and AGAIN after every weight update (which edges are -inf decides whether a retimed form exists,
// see onetape_tiled_viterbi): a failed build is retried then, not latched; a program without a retimed form or without codes is
// freed at once (its column-by-column twin would never run).
static WideProgram *wide_tb_program(mb_machine *m) {
  if (g_kernel_choice == 1 || !wide_applicable(m) || !opt_int<MB_ONETAPE_TB>()) return nullptr;
  FastState *f = fast_state(m);
  WideProgram &P = f->wVitTb;
  if (!f->wVitTbTried || P.dirty) {
    f->wVitTbTried = true;
    P.dirty = false;      // (this set of weights has been looked at, whatever comes of it)
    for (long long e = 0; e < m->nTrans; ++e)
      if (m->inTok[e] == 0 && m->outTok[e] == 0 && m->dst[e] <= m->src[e]) { if (P.ok) wide_free(P); return nullptr; }
    P.tbCodes = true;
    const bool built = wide_build(m, false, true, P);
    if (!built || !(P.ok && P.retOk && P.tbOk)) { wide_free(P); P.dirty = false; return nullptr; }
  }
  return (P.ok && P.retOk && P.tbOk) ? &P : nullptr;
}

// Fill the matrices of one chunk of pairs (materialised), choosing the kernel family.
static int fill_chunk(mb_machine *m, int mode, const PairDesc *d_desc, const std::vector<PairDesc> &hp, const int *d_in,
                      const int *d_out, double *pool, int startState, const mb_batch *b) {
  const bool env = b && b->hasEnv;   // envelopes: cells outside keep the -inf written here (tiles outside them do not even run)
  if (env) {
    long long cells = 0;
    for (const PairDesc &pd : hp) cells = std::max(cells, pd.cellBase + (long long)(pd.inLen + 1) * (pd.outLen + 1) * m->S);
    if (launch_fill_neg_inf(pool, cells, g_stream)) return 1;
  }
  const bool tiledViterbi = !env && mode == MB_VITERBI && onetape_tiled_viterbi(m);
  if (!env && startState == 0 && wide_applicable(m) && g_kernel_choice != 1 && !tiledViterbi) {
    WideProgram *W = wide_program(m, mode);
    if (!W) return 1;
    const int rcW = wide_fill(m, *W, d_desc, (long long)hp.size(), m->nOut ? d_out : d_in, pool, nullptr, g_stream, false, hp.data(), device_cus());
    g_last_kernel = wide_kernel_name(*W);
    return rcW;
  }
  if ((use_medium(m) && !(env && wide_applicable(m))) || tiledViterbi) {
    FastState *f = fast_state(m);
    const bool exactFwd = mode == MB_VITERBI || (mode == MB_FORWARD && startState != 0);
    MedProgram &P = mode == MB_BACKWARD ? f->bwdSum : (exactFwd ? f->fwdExact : f->fwdSum);
    const MedGeom &geo = mode == MB_BACKWARD ? f->geoBS : (exactFwd ? f->geoFE : f->geoFS);
    const MedEnv me = b ? med_env(b) : MedEnv();
    const int rc = medium_fill_materialised(m, P, geo, mode == MB_VITERBI ? MB_VITERBI : MB_FORWARD,
                                            (mode == MB_FORWARD && startState != 0) ? startState : -1, d_desc, hp, d_in, d_out, pool, g_stream, me);
    if (rc >= 0) {
      g_last_kernel = medium_jit_ready(P, mode == MB_VITERBI ? MB_VITERBI : MB_FORWARD, MED_MAT_FULL) ? "k_medium_jit" : (mode == MB_VITERBI ? "k_medium_tile<1>" : "k_medium_tile<0>");
      return rc;
    }
    // (-1: envelopes need the run-time specialised kernel and it is unavailable: the generic family takes the chunk)
  }
  g_last_kernel = mode == MB_VITERBI ? "k_generic_fill_fwd<1>" : (mode == MB_BACKWARD ? "k_generic_fill_bwd" : "k_generic_fill_fwd<0>");
  return launch_generic_fill(m, mode, d_desc, (long long)hp.size(), d_in, d_out, pool, startState, g_stream,
                             env ? b->d_envStart : nullptr, env ? b->d_envEnd : nullptr);
}

// ---- the small-machine family (mb_small.cpp): placement of its per-pair buffers and chunking -----------------------------
struct SmallPlan {
  std::vector<SmAux> aux;
  long long poolD = 0, tbB = 0, haloD = 0, boundD = 0;
};

// Halo rows and boundary records are laid out for the LARGER of the two sweep directions' needs: a count call runs the
// Backward and the Forward program over the same buffers (and offsets), and the two programs of an asymmetric machine
// keep different numbers of values per halo row / boundary record.
static int small_halo_width(const mb_machine *m) { const FastState *f = (const FastState *)m->fast; return std::max(1, std::max(f->smF.H, f->smB.H)); }
static int small_bound_width(const mb_machine *m) { const FastState *f = (const FastState *)m->fast; return std::max(f->smF.NBD, f->smB.NBD); }

static void small_plan(const mb_machine *m, const SmallProgram &P, const PairDesc *hp, long long n, bool wantPool, bool wantTb, SmallPlan &pl) {
  const int HW = small_halo_width(m), BW = small_bound_width(m);
  pl = SmallPlan();
  pl.aux.resize((size_t)n);
  for (long long k = 0; k < n; ++k) {
    const PairDesc &pd = hp[k];
    SmAux &a = pl.aux[(size_t)k];
    a.pool = pl.poolD; a.tb = pl.tbB; a.halo = pl.haloD; a.bound = pl.boundD;
    if (wantPool) pl.poolD += small_pair_doubles(P.S, pd.inLen, pd.outLen);
    if (wantTb) pl.tbB += (small_pair_tb_bytes(P.S, pd.inLen, pd.outLen) + 15) & ~15ll;
    pl.haloD += (long long)small_strips(pd.inLen) * (pd.outLen + 1) * HW;   // one halo column per strip
    pl.boundD += (long long)small_strips(pd.inLen) * 64 * BW;
  }
}

// Split the batch into chunks whose buffers fit the memory budget (pairs are independent).
static bool small_chunks_plan(const mb_batch *b, const SmallProgram &P, bool wantPool, bool wantTb, std::vector<Chunk> &out) {
  const long long budget = (long long)budget_bytes();
  long long p0 = 0, acc = 0;
  for (long long p = 0; p < b->nPairs; ++p) {
    const PairDesc &pd = b->pairs[p];
    long long c = ((long long)small_strips(pd.inLen) * (pd.outLen + 1) * small_halo_width(b->m) + (long long)small_strips(pd.inLen) * 64 * small_bound_width(b->m)) * 8;
    if (wantPool) c += small_pair_doubles(P.S, pd.inLen, pd.outLen) * 8;
    if (wantTb) c += small_pair_tb_bytes(P.S, pd.inLen, pd.outLen) + 16;
    if (c > budget) { set_error("a single DP matrix (" + std::to_string(c) + " bytes) exceeds the device memory budget"); return false; }
    if (acc + c > budget) { out.push_back({p0, p, acc}); p0 = p; acc = 0; }
    acc += c;
  }
  if (b->nPairs > p0) out.push_back({p0, b->nPairs, acc});
  return true;
}

// One chunk of a small-family call: its pairs, their placement, the aux records (owned, on the device) and the sweep's arguments.
struct SmallChunk { SmallPlan pl; std::vector<PairDesc> hp; SmBuf<SmAux> d_aux; SmSweep sw; };
// aux records uploaded, workspaces sized; fills k.sw
static int small_prepare(mb_batch *b, const Chunk &c, const SmallProgram &P, bool wantPool, bool wantTb, SmallChunk &k, size_t chunkNo = (size_t)-1) {
  SmallPlan &pl = k.pl; std::vector<PairDesc> &hp = k.hp; SmSweep &sw = k.sw;
  hp.assign(b->pairs.begin() + c.p0, b->pairs.begin() + c.p1);
  small_plan(b->m, P, hp.data(), (long long)hp.size(), wantPool, wantTb, pl);
  MB_HIP(k.d_aux.alloc((long long)hp.size()));
  MB_HIP(hipMemcpyAsync(k.d_aux, pl.aux.data(), hp.size() * sizeof(SmAux), hipMemcpyHostToDevice, g_stream));
  sw = SmSweep();
  sw.d_pairs = b->d_pairs + c.p0; sw.pairs = &hp; sw.d_in = b->d_in; sw.d_out = b->d_out; sw.d_aux = k.d_aux;
  if (chunkNo != (size_t)-1) {
    if (b->smTiles.size() <= 2 * chunkNo + 1) b->smTiles.resize(2 * chunkNo + 2);
    for (int bw = 0; bw < 2; ++bw) {
      SmTileCache &tc = b->smTiles[2 * chunkNo + bw];
      if (tc.p0 != c.p0 || tc.p1 != c.p1 || tc.envVersion != b->envVersion) {
        if (tc.d_tiles) (void)hipFree(tc.d_tiles);
        if (tc.d_deps) (void)hipFree(tc.d_deps);
        if (tc.d_flags) (void)hipFree(tc.d_flags);
        tc.d_deps = tc.d_flags = nullptr;
        tc = SmTileCache(); tc.p0 = c.p0; tc.p1 = c.p1; tc.envVersion = b->envVersion;
      }
    }
    sw.tileCacheFwd = &b->smTiles[2 * chunkNo]; sw.tileCacheBwd = &b->smTiles[2 * chunkNo + 1];
  }
  if (b->hasEnv) {   // PairDesc::envBase (-1: full) indexes them
    sw.d_envStart = b->d_envStart; sw.d_envEnd = b->d_envEnd;
    sw.h_envStart = b->h_envStart.data(); sw.h_envEnd = b->h_envEnd.data();
  }
  sw.haloDoubles = pl.haloD;      // (pre-filled by the sweep: -inf for tiles that do not run, the sentinel of the persistent strips)
  if (wantPool && !(sw.d_pool = (double *)ws_get(0, (size_t)std::max<long long>(pl.poolD, 1) * 8))) return 1;
  if (wantTb && !(sw.d_tb = (unsigned char *)ws_get(8, (size_t)std::max<long long>(pl.tbB, 16)))) return 1;
  if (!(sw.d_halo = (double *)ws_get(9, (size_t)std::max<long long>(pl.haloD, 1) * 8))) return 1;
  if (!(sw.d_bound = (double *)ws_get(10, (size_t)std::max<long long>(pl.boundD, 1) * 8))) return 1;
  return 0;
}

// the chunk builder of a small-family call (for_chunks); it numbers the chunks for the tile caches
static auto small_chunk_build(mb_batch *b, const SmallProgram &P, bool wantPool, bool wantTb) {
  return [=, &P, chunkNo = (size_t)0](const Chunk &c, SmallChunk &k) mutable { return small_prepare(b, c, P, wantPool, wantTb, k, chunkNo++); };
}

static int small_forward(mb_batch *b, int flags, double *loglike) {
  FastState *f = (FastState *)b->m->fast;
  const bool mat = !(flags & MB_ROLLING);
  std::vector<Chunk> chunks;
  if (!small_chunks_plan(b, f->smF, mat, false, chunks)) return 1;
  SmBuf<double> d_ll;
  MB_HIP(d_ll.alloc(b->nPairs));
  int rc = for_chunks<SmallChunk>(chunks, small_chunk_build(b, f->smF, mat, false), [&](const Chunk &c, SmallChunk &k, Timer &tm) {
    k.sw.d_loglike = d_ll + c.p0;
    Timed t(tm, 0);
    return small_sweep(f->smF, SM_SUM, mat, k.sw, g_stream);
  });
  g_last_kernel = small_kernel_name(f->smF, SM_SUM, mat);
  if (!rc) rc = fetch_loglike(loglike, d_ll, b->nPairs);
  return rc;
}

// ---- the path tail of the Viterbi calls (small family here, viterbi_chunks below) ------------------------------------------------
// MB_TIMING: the host-side laps of a Viterbi call on stderr
struct Laps {
  const bool on = opt_present<MB_TIMING>();
  double tPrev = now();
  static double now() { return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now().time_since_epoch()).count(); }
  void lap(const char *what) { if (on) { const double t = now(); fprintf(stderr, "[mbhip] viterbi %-28s %7.2f ms\n", what, t - tPrev); tPrev = t; } }
};

// Where the traceback kernel of a chunk writes: each pair's path into a slot of its worst-case length, the lengths beside them
// (cached workspaces 3..5: a hipMalloc/hipFree pair per call costs more than the traceback kernel of a small batch).
struct PathSlots { std::vector<long long> slot; long long *d_slot = nullptr, *d_len = nullptr; uint32_t *d_path = nullptr; };
static int path_slots(const mb_batch *b, const Chunk &c, PathSlots &s) {
  const long long np = c.p1 - c.p0;
  s.slot.assign(np + 1, 0);
  for (long long p = 0; p < np; ++p)
    s.slot[p + 1] = s.slot[p] + mb_viterbi_path_bound(b->m, b->pairs[c.p0 + p].inLen, b->pairs[c.p0 + p].outLen);
  if (!(s.d_slot = (long long *)ws_get(3, (np + 1) * sizeof(long long)))) return 1;
  if (!(s.d_len = (long long *)ws_get(4, np * sizeof(long long)))) return 1;
  if (!(s.d_path = (uint32_t *)ws_get(5, std::max<long long>(s.slot[np], 1) * sizeof(uint32_t)))) return 1;
  return hip_ok(hipMemcpyAsync(s.d_slot, s.slot.data(), (np + 1) * sizeof(long long), hipMemcpyHostToDevice, g_stream), "H2D") ? 0 : 1;
}

// The caller's path arrays of a Viterbi call, and how much of them the chunks so far have used.
struct PathOut { int64_t *off; uint32_t *edges; int64_t cap; long long written = 0; };

// The paths of chunk c from their slots to the caller's arrays: lengths checked (-1: no finite path, an empty one; -2 / any other
// negative: the traceback's two errors, worded by the caller), the chunk's total checked against what is left of pathCap, then
// packed on the device (slots 6/7) and ONE copy of exactly the used entries (the slots are sized for the worst case,
// (inLen+outLen+1) x levels edges per pair: 32 MB for 1024 x 1 kb x 1 kb dnapsw pairs, 15 MB used).
static int pack_paths(PathOut &o, const Chunk &c, const PathSlots &s, const char *overflowText, const char *deadEndText, Laps &laps) {
  const long long np = c.p1 - c.p0;
  std::vector<long long> len(np, 0), off(np, -1);
  if (!hip_ok(hipMemcpy(len.data(), s.d_len, np * sizeof(long long), hipMemcpyDeviceToHost), "D2H path lengths")) return 1;
  long long total = 0;
  for (long long p = 0; p < np; ++p) {
    const long long n = len[p];
    if (n == -1) continue;   // -inf end cell: no path (src/dpmatrix.defs.h:84)
    if (n < 0) { set_error(n == -2 ? overflowText : deadEndText); return 1; }
    off[p] = total; total += n;
  }
  if (o.written + total > o.cap) { set_error("pathCap too small for the Viterbi paths of this batch"); return 1; }
  long long *d_off = (long long *)ws_get(6, np * sizeof(long long));
  uint32_t *d_packed = (uint32_t *)ws_get(7, std::max<long long>(total, 1) * sizeof(uint32_t));
  if (!d_off || !d_packed) return 1;
  if (!hip_ok(hipMemcpyAsync(d_off, off.data(), np * sizeof(long long), hipMemcpyHostToDevice, g_stream), "H2D")) return 1;
  if (const int rc = launch_compact_paths(s.d_path, s.d_slot, s.d_len, d_off, d_packed, np, g_stream)) return rc;
  if (total && d2h_large(o.edges + o.written, d_packed, total * sizeof(uint32_t))) return 1;
  if (!hip_ok(hipStreamSynchronize(g_stream), "path compaction")) return 1;
  laps.lap("pack + D2H paths");
  for (long long p = 0; p < np; ++p) {
    if (len[p] > 0) o.written += len[p];
    o.off[c.p0 + p + 1] = o.written;
  }
  return 0;
}
static const char *const PATH_OVERFLOW = "Viterbi traceback exceeded its path bound", *const PATH_DEAD_END = "Viterbi traceback reached a dead end";

// ViterbiMatrix(eval, sp).logLike() / path(): one traceback byte per cell, walked on the device
static int small_viterbi(mb_batch *b, double *loglike, int64_t *pathOff, uint32_t *pathEdges, int64_t pathCap) {
  FastState *f = (FastState *)b->m->fast;
  const bool wantPaths = pathEdges != nullptr && pathOff != nullptr;
  std::vector<Chunk> chunks;
  if (!small_chunks_plan(b, f->smF, false, true, chunks)) return 1;
  PathOut out{pathOff, pathEdges, pathCap};
  Laps laps;
  const int rc = for_chunks<SmallChunk>(chunks, small_chunk_build(b, f->smF, false, true), [&](const Chunk &c, SmallChunk &k, Timer &tm) {
    const long long np = c.p1 - c.p0;
    SmBuf<double> d_ll;
    if (!hip_ok(d_ll.alloc(np), "hipMalloc")) return 1;
    k.sw.d_loglike = d_ll;
    laps.lap("chunk set-up");
    PathSlots ps;
    {
      Timed t(tm, 0);
      if (const int r = small_sweep(f->smF, SM_TB, false, k.sw, g_stream)) return r;
      laps.lap("fill (traceback bytes)");
      if (wantPaths) {
        if (path_slots(b, c, ps)) return 1;
        if (const int r = launch_small_traceback(f->smF, k.sw.d_pairs, np, b->d_in, b->d_out, k.sw.d_tb, k.d_aux, d_ll, ps.d_slot, ps.d_path, ps.d_len, g_stream)) return r;
      }
    }
    laps.lap("traceback kernel");
    if (fetch_loglike(loglike + c.p0, d_ll, np)) return 1;
    return wantPaths ? pack_paths(out, c, ps, PATH_OVERFLOW, PATH_OVERFLOW, laps) : 0;      // (this family's walker reports every failure as the bound's)
  });
  g_last_kernel = "k_small_tb";
  return rc;
}

// MachineCounts(eval, seqPairList): Backward matrices written once (tile-major), then a Forward sweep that reads them and
// keeps the posterior usage sums on chip -- the Forward matrix itself never reaches HBM.
static const int SMALL_COUNT_REPLICAS = 64;
static int small_counts(mb_batch *b, double *counts, double *loglikeSum, double *loglike) {
  FastState *f = (FastState *)b->m->fast;
  const long long nT = b->m->nTrans, nRep = std::max<long long>(nT, 1) * SMALL_COUNT_REPLICAS;
  std::vector<Chunk> chunks;
  if (!small_chunks_plan(b, f->smB, true, false, chunks)) return 1;
  g_last_kernel = "k_small_count";
  SmBuf<double> d_rep, d_ll, d_bll;
  if (!hip_ok(d_rep.alloc(nRep), "hipMalloc") || !hip_ok(d_ll.alloc(b->nPairs), "hipMalloc") || !hip_ok(d_bll.alloc(b->nPairs), "hipMalloc")) return 1;
  if (!hip_ok(hipMemsetAsync(d_rep, 0, nRep * sizeof(double), g_stream), "memset")) return 1;
  const int rc = for_chunks<SmallChunk>(chunks, small_chunk_build(b, f->smB, true, false), [&](const Chunk &c, SmallChunk &k, Timer &tm) {
    Timed t(tm, 0);
    k.sw.d_loglike = d_bll + c.p0;
    if (const int r = small_sweep(f->smB, SM_SUM, true, k.sw, g_stream)) return r;      // BackwardMatrix::fill, src/backward.cpp:18-46
    k.sw.d_loglike = d_ll + c.p0; k.sw.d_bwdLL = d_bll + c.p0; k.sw.d_counts = d_rep; k.sw.nRep = SMALL_COUNT_REPLICAS;
    return small_sweep(f->smF, SM_COUNT, false, k.sw, g_stream);                          // Forward + getCounts, src/backward.cpp:58-87
  });
  if (rc) return rc;
  std::vector<double> hc((size_t)nT * SMALL_COUNT_REPLICAS), hll(b->nPairs);
  if (nT && !hip_ok(hipMemcpy(hc.data(), d_rep, hc.size() * sizeof(double), hipMemcpyDeviceToHost), "D2H counts")) return 1;
  if (fetch_loglike(hll.data(), d_ll, b->nPairs)) return 1;
  CountSum sum(nT);
  for (long long e = 0; e < nT; ++e) {
    if (g_deterministic) {      // fixed point, 2^-36: the replicas add up as integers, then the sum is decoded
      unsigned long long tot = 0; bool inRange = true;
      for (int r = 0; r < SMALL_COUNT_REPLICAS; ++r) { unsigned long long u; std::memcpy(&u, &hc[(size_t)r * nT + e], 8); inRange = inRange && u < (1ull << 62); tot += u; }
      if (!det_to_double(tot, sum.total[(size_t)e]) || !inRange) { set_error(COUNT_RANGE_ERROR); return 1; }
      continue;
    }
    double s = 0.0;
    for (int r = 0; r < SMALL_COUNT_REPLICAS; ++r) s += hc[(size_t)r * nT + e];
    sum.total[(size_t)e] = s;
  }
  sum.finish(hll, counts, loglikeSum, loglike);   // loglike += forward.logLike(), src/counts.cpp:61-62
  return 0;
}

// one full matrix in the reference's layout (mb_fill): sweep tile-major, convert on the device, copy out
static int small_fill(mb_batch *b, int mode, double *cellsOut) {
  FastState *f = (FastState *)b->m->fast;
  SmallProgram &P = mode == MB_BACKWARD ? f->smB : f->smF;
  const PairDesc &pd = b->pairs[0];
  const long long n = (long long)(pd.inLen + 1) * (pd.outLen + 1) * b->m->S;
  const int smMode = mode == MB_VITERBI ? SM_MAX : SM_SUM;
  const int rc = [&]() {
    if ((size_t)(small_pair_doubles(P.S, pd.inLen, pd.outLen) + n) * 8 > budget_bytes()) { set_error("matrix exceeds the device memory budget"); return 1; }
    SmallChunk k;
    if (const int r = small_prepare(b, Chunk{0, 1, 0}, P, true, false, k)) return r;
    SmBuf<double> d_ll;
    if (!hip_ok(d_ll.alloc(1), "hipMalloc")) return 1;
    double *d_cells = (double *)ws_get(1, (size_t)std::max<long long>(n, 1) * 8);
    if (!d_cells) return 1;
    k.sw.d_loglike = d_ll;
    if (const int r = small_sweep(P, smMode, true, k.sw, g_stream)) return r;
    if (const int r = launch_fill_neg_inf(d_cells, n, g_stream)) return r;
    if (const int r = launch_small_unpack(k.sw.d_pool, P.S, pd.inLen, pd.outLen, mode == MB_BACKWARD, d_cells,
                                          b->hasEnv && pd.envBase >= 0 ? b->d_envStart + pd.envBase : nullptr,
                                          b->hasEnv && pd.envBase >= 0 ? b->d_envEnd + pd.envBase : nullptr, g_stream)) return r;
    if (!hip_ok(hipStreamSynchronize(g_stream), "fill kernel")) return 1;
    return hip_ok(hipMemcpy(cellsOut, d_cells, n * sizeof(double), hipMemcpyDeviceToHost), "D2H matrix") ? 0 : 1;
  }();
  g_last_kernel = small_kernel_name(P, smMode, true);
  return rc;
}

}  // namespace mb

using namespace mb;

extern "C" {

int mb_device_count(void) {
  int n = 0;
  if (hipGetDeviceCount(&n) != hipSuccess) return 0;
  return n;
}

int mb_set_device(int device) {
  ApiGuard guard;
  if (g_init && device != g_device) {   // the stream, the workspaces and every compiled program are bound to the first device
    set_error("mb_set_device: the library is already initialised on device " + std::to_string(g_device) + " (one process drives one GPU)");
    return 1;
  }
  MB_HIP(hipSetDevice(device));
  return 0;
}

int mb_synchronize(void) {
  ApiGuard guard;
  if (!g_init) return 0;      // nothing was ever queued
  MB_HIP(hipDeviceSynchronize());
  return 0;
}

const char *mb_last_error(void) { return g_err.c_str(); }
double mb_last_device_ms(void) { return g_last_ms; }
const char *mb_last_kernel_name(void) { return g_last_kernel; }
int64_t mb_last_launch_count(void) { return g_last_launches; }

int mb_set_kernel(int which) {
  if (which < 0 || which > 3) { set_error("mb_set_kernel: unknown kernel family"); return 1; }
  g_kernel_choice = which;
  return 0;
}

int mb_set_memory_budget(size_t bytes) { g_mem_budget = bytes; return 0; }

size_t mb_memory_budget(void) {
  ApiLock lock;
  if (ensure_init()) return 0;
  return budget_bytes();
}

int mb_release_workspace(void) {
  ApiGuard guard;
  ws_release();
  return 0;
}

int mb_alloc_stats(int64_t *poolAllocs, int64_t *poolFrees, int64_t *evictions, uint64_t *bytesAllocated, double *ms) {
  ApiLock lock;
  if (poolAllocs) *poolAllocs = g_alloc.allocs;
  if (poolFrees) *poolFrees = g_alloc.frees;
  if (evictions) *evictions = g_alloc.evictions;
  if (bytesAllocated) *bytesAllocated = g_alloc.bytes;
  if (ms) *ms = g_alloc.ms;
  return 0;
}

int mb_jit_stats(double *compileMs, int64_t *compiles, int64_t *cacheHits) {
  if (compileMs) *compileMs = jit_compile_ms();
  if (compiles) *compiles = jit_compiles();
  if (cacheHits) *cacheHits = jit_cache_hits();
  return 0;
}

int mb_machine_sweep_ops(mb_machine *m, double *expPerCell, double *logPerCell, const char **family) {
  ApiGuard guard;
  if (!m) { set_error("null argument"); return 1; }
  double ne = 0.0, nl = 0.0; const char *fam = "generic";
  if (use_small(m)) {
    // per supercell and lane: two candidates -> exp + log of the pair; three or more -> one exp each + one log
    const SmallProgram &P = ((FastState *)m->fast)->smF;
    for (int d = 0; d < P.S; ++d) { const size_t n = P.cand[d].size(); if (n == 2) { ne += 1; nl += 1; } else if (n > 2) { ne += (double)n; nl += 1; } }
    ne /= m->S; nl /= m->S; fam = "small";
  } else if (wide_applicable(m) && g_kernel_choice != 1) {
    WideProgram *W = wide_program(m, MB_FORWARD);
    if (!W) return 1;
    ne = (double)W->slotsPerColumn * W->W / m->S; nl = (double)W->rounds.size() * W->W / m->S; fam = "one-tape";   // one exp per slot and lane (+ the group reduction), one log per round
  } else if (use_medium(m)) {
    const MedProgram &P = fast_state(m)->fwdSum;
    double slots = 0.0, logs = 0.0;   // a round with one candidate slot is a plain add: no exp, no log
    for (const MedRoundInfo &ri : P.roundInfo) if (ri.slots.size() > 1) { slots += (double)ri.slots.size(); logs += 1.0; }
    ne = slots * P.LPG / m->S; nl = logs * P.LPG / m->S; fam = "tiled";
  } else {
    ne = (double)m->nTrans / m->S; nl = ne;   // generic family: log1p(exp()) per candidate, token-filtered at run time (upper bound)
  }
  if (expPerCell) *expPerCell = ne;
  if (logPerCell) *logPerCell = nl;
  if (family) *family = fam;
  return 0;
}

// Tuning knobs are read from the environment when a machine's programs / kernels are built (mb_options.h lists them, DESIGN.md
// section 4.7 the ones for a host); this is the same switchboard for a host that prefers calls to environment variables.
int mb_set_option(const char *name, const char *value) {
  ApiLock lock;
  const int id = opt_find(name);
  if (id < 0) { set_error(std::string("mb_set_option: unknown option ") + (name ? name : "(null)")); return 1; }
  if (OPT_TABLE[id].cls == OptClass::info) { set_error(std::string("mb_set_option: ") + name + " is read-only"); return 1; }
  opt_override((Opt)id, value);      // (the library's table: the process environment is the host's, not ours to write)
  return 0;
}

const char *mb_get_option(const char *name) {
  ApiLock lock;
  if (!name) return opt_list();
  const int id = opt_find(name);
  if (id < 0) return nullptr;
  if (id == MB_INFO_INPLACE_RING_KERNELS) {      // (read-only: kernel kinds that took the in-place ring so far, for tests)
    static thread_local std::string v;
    v = std::to_string(medium_inplace_kernels());
    return v.c_str();
  }
  return opt_raw((Opt)id);
}

mb_machine *mb_machine_create(int32_t nStates, int32_t nInTok, int32_t nOutTok, int64_t nTrans, const uint32_t *src,
                              const uint32_t *dst, const uint16_t *inTok, const uint16_t *outTok, const double *logWeight) {
  ApiGuard guard;
  if (nStates <= 0) { set_error("EvaluatedMachine has no states"); return nullptr; }
  if (nInTok < 0 || nOutTok < 0 || nTrans < 0) { set_error("mb_machine_create: negative size"); return nullptr; }
  if (ensure_init()) return nullptr;
  mb_machine *m = new mb_machine();
  m->S = nStates; m->nIn = nInTok; m->nOut = nOutTok; m->nTrans = nTrans;
  m->src.assign(src, src + nTrans); m->dst.assign(dst, dst + nTrans);
  m->inTok.assign(inTok, inTok + nTrans); m->outTok.assign(outTok, outTok + nTrans);
  m->logW.assign(logWeight, logWeight + nTrans);
  std::string err;
  if (!compile_machine(m, &err)) { set_error(err); delete m; return nullptr; }
  if (!upload_machine(m)) { free_machine_device(m); delete m; return nullptr; }
  return m;
}

int mb_machine_set_weights(mb_machine *m, const double *logWeight) {
  ApiGuard guard;
  if (!m) { set_error("null machine"); return 1; }
  m->logW.assign(logWeight, logWeight + m->nTrans);
  if (!upload_weights(m)) return 1;
  if (m->fast) {
    FastState *f = (FastState *)m->fast;
    if (f->mediumOk && !(medium_refresh_weights(m, f->fwdExact) && medium_refresh_weights(m, f->fwdSum) && medium_refresh_weights(m, f->bwdSum))) return 1;
    if (!f->mediumOk && f->exactOk && !medium_refresh_weights(m, f->fwdExact)) return 1;
    if (f->countOk && !medium_refresh_weights(m, f->fwdCnt)) return 1;
    if (f->tbOk && !medium_refresh_weights(m, f->fwdTb)) return 1;
    if (f->smallOk && !(small_refresh_weights(m, f->smF) && small_refresh_weights(m, f->smB))) return 1;
    f->wFwd.dirty = f->wBwd.dirty = f->wVit.dirty = f->wVitTb.dirty = true;
    usage_free(f->usage);      // (its records carry the weights, and which transitions are -inf: rebuilt by the next count call)
  }
  return 0;
}

void mb_machine_destroy(mb_machine *m) {
  ApiGuard guard;
  if (!m) return;
  if (m->fast) {
    FastState *f = (FastState *)m->fast;
    medium_free(f->fwdExact); medium_free(f->fwdSum); medium_free(f->bwdSum); medium_free(f->fwdCnt); medium_free(f->fwdTb);
    wide_free(f->wFwd); wide_free(f->wBwd); wide_free(f->wVit); wide_free(f->wVitTb); wide_counts_free(f->wCnt); wide_traceback_free(f->wTb);
    small_free(f->smF); small_free(f->smB);
    usage_free(f->usage);
    delete f;
  }
  free_machine_device(m);
  delete m;
}

int32_t mb_machine_n_states(const mb_machine *m) { return m ? m->S : 0; }
int64_t mb_machine_n_trans(const mb_machine *m) { return m ? m->nTrans : 0; }
int32_t mb_machine_n_levels(const mb_machine *m) { return m ? m->nLevF : 0; }

int mb_machine_edge_order(const mb_machine *m, int which, uint32_t *out) {
  if (!m) { set_error("null machine"); return 1; }
  const std::vector<uint32_t> &p = which ? m->outPerm : m->inPerm;
  std::memcpy(out, p.data(), p.size() * sizeof(uint32_t));
  return 0;
}

mb_batch *mb_batch_create(mb_machine *m, int64_t nPairs, const int32_t *inTok, const int64_t *inOff, const int32_t *outTok,
                          const int64_t *outOff) {
  ApiGuard guard;
  if (!m) { set_error("null machine"); return nullptr; }
  if (nPairs < 0) { set_error("negative pair count"); return nullptr; }
  mb_batch *b = new mb_batch();
  b->m = m; b->nPairs = nPairs;
  b->pairs.resize(nPairs);
  long long base = 0;
  for (long long p = 0; p < nPairs; ++p) {
    PairDesc &pd = b->pairs[p];
    const long long il = inOff[p + 1] - inOff[p], ol = outOff[p + 1] - outOff[p];
    if (il < 0 || ol < 0 || il > 0x3fffffff || ol > 0x3fffffff) { set_error("bad sequence offsets"); delete b; return nullptr; }
    pd.inBase = inOff[p] - inOff[0]; pd.outBase = outOff[p] - outOff[0];
    pd.inLen = (int)il; pd.outLen = (int)ol; pd.cellBase = base; pd.envBase = -1;
    const long long c = (il + 1) * (ol + 1) * m->S;
    base += c;
    b->maxPairCells = std::max(b->maxPairCells, c);
  }
  b->totalCells = base;
  b->nInTokTotal = nPairs ? inOff[nPairs] - inOff[0] : 0;
  b->nOutTokTotal = nPairs ? outOff[nPairs] - outOff[0] : 0;
  const int32_t *in0 = inTok + (nPairs ? inOff[0] : 0), *out0 = outTok + (nPairs ? outOff[0] : 0);
  // Tokenizer::tokenize throws on symbols outside the alphabet (src/eval.h:33-37); token 0 (epsilon) is not a symbol
  for (long long k = 0; k < b->nInTokTotal; ++k)
    if (in0[k] < 1 || in0[k] > m->nIn) { set_error("Can't tokenize symbol: input token outside the machine's alphabet"); delete b; return nullptr; }
  for (long long k = 0; k < b->nOutTokTotal; ++k)
    if (out0[k] < 1 || out0[k] > m->nOut) { set_error("Can't tokenize symbol: output token outside the machine's alphabet"); delete b; return nullptr; }
  auto fail = [&]() { mb_batch_destroy(b); return (mb_batch *)nullptr; };
  if (!hip_ok(hipMalloc((void **)&b->d_in, std::max<long long>(b->nInTokTotal, 1) * sizeof(int)), "hipMalloc(tokens)")) return fail();
  if (!hip_ok(hipMalloc((void **)&b->d_out, std::max<long long>(b->nOutTokTotal, 1) * sizeof(int)), "hipMalloc(tokens)")) return fail();
  if (!hip_ok(hipMalloc((void **)&b->d_pairs, std::max<long long>(nPairs, 1) * sizeof(PairDesc)), "hipMalloc(pairs)")) return fail();
  if (b->nInTokTotal && !hip_ok(hipMemcpy(b->d_in, in0, b->nInTokTotal * sizeof(int), hipMemcpyHostToDevice), "H2D tokens")) return fail();
  if (b->nOutTokTotal && !hip_ok(hipMemcpy(b->d_out, out0, b->nOutTokTotal * sizeof(int), hipMemcpyHostToDevice), "H2D tokens")) return fail();
  if (nPairs && !hip_ok(hipMemcpy(b->d_pairs, b->pairs.data(), nPairs * sizeof(PairDesc), hipMemcpyHostToDevice), "H2D pairs")) return fail();
  return b;
}

void mb_batch_destroy(mb_batch *b) {
  ApiGuard guard;
  if (!b) return;
  if (b->d_in) (void)hipFree(b->d_in);
  if (b->d_out) (void)hipFree(b->d_out);
  if (b->d_pairs) (void)hipFree(b->d_pairs);
  if (b->d_envStart) (void)hipFree(b->d_envStart);
  if (b->d_envEnd) (void)hipFree(b->d_envEnd);
  for (mb::SmTileCache &tc : b->smTiles) { if (tc.d_tiles) (void)hipFree(tc.d_tiles); if (tc.d_deps) (void)hipFree(tc.d_deps); if (tc.d_flags) (void)hipFree(tc.d_flags); }
  delete b;
}

int64_t mb_batch_cells(const mb_batch *b) { return b ? b->totalCells : 0; }

// Envelope::fits / connected as DPMatrix::alloc asserts them (src/dpmatrix.defs.h:31-32, src/seqpair.cpp:184-193)

int mb_batch_set_envelopes(mb_batch *b, const int64_t *envOff, const int32_t *inStart, const int32_t *inEnd) {
  ApiGuard guard;
  if (!b || !envOff) { set_error("null argument"); return 1; }
  if (b->d_envStart) { (void)hipFree(b->d_envStart); b->d_envStart = nullptr; }
  if (b->d_envEnd) { (void)hipFree(b->d_envEnd); b->d_envEnd = nullptr; }
  b->hasEnv = false;
  ++b->envVersion;
  const long long total = envOff[b->nPairs] - envOff[0];
  auto fail = [&](const char *msg) {   // a rejected call leaves the batch with full envelopes, not with half of the new ones
    for (PairDesc &pd : b->pairs) pd.envBase = -1;
    b->hasEnv = false;
    if (b->nPairs) (void)hipMemcpy(b->d_pairs, b->pairs.data(), b->nPairs * sizeof(PairDesc), hipMemcpyHostToDevice);
    set_error(msg);
    return 1;
  };
  for (PairDesc &pd : b->pairs) pd.envBase = -1;
  for (long long p = 0; p < b->nPairs; ++p) {
    PairDesc &pd = b->pairs[p];
    const long long rows = envOff[p + 1] - envOff[p];
    if (rows == 0) continue;   // full envelope
    if (!inStart || !inEnd) return fail("null argument");
    if (rows != (long long)pd.outLen + 1) return fail("Envelope/sequence mismatch");
    const int32_t *st = inStart + envOff[p], *en = inEnd + envOff[p];
    for (long long y = 0; y < rows; ++y)
      if (st[y] < 0 || en[y] > pd.inLen + 1 || st[y] > en[y]) return fail("Envelope/sequence mismatch");
    bool conn = env_overlapping(st[0], en[0], 0, 1);
    for (long long y = 1; conn && y < rows; ++y) conn = env_overlapping(st[y - 1], (long long)en[y - 1] + 1, st[y], en[y]);
    conn = conn && env_overlapping(st[rows - 1], en[rows - 1], pd.inLen, (long long)pd.inLen + 1);
    if (!conn) return fail("Envelope is not connected");
    pd.envBase = envOff[p] - envOff[0];
    b->hasEnv = true;
  }
  if (b->hasEnv) {
    MB_HIP(hipMalloc((void **)&b->d_envStart, std::max<long long>(total, 1) * sizeof(int)));
    MB_HIP(hipMalloc((void **)&b->d_envEnd, std::max<long long>(total, 1) * sizeof(int)));
    MB_HIP(hipMemcpy(b->d_envStart, inStart + envOff[0], total * sizeof(int), hipMemcpyHostToDevice));
    MB_HIP(hipMemcpy(b->d_envEnd, inEnd + envOff[0], total * sizeof(int), hipMemcpyHostToDevice));
    b->h_envStart.assign(inStart + envOff[0], inStart + envOff[0] + total);
    b->h_envEnd.assign(inEnd + envOff[0], inEnd + envOff[0] + total);
  }
  if (b->nPairs) MB_HIP(hipMemcpy(b->d_pairs, b->pairs.data(), b->nPairs * sizeof(PairDesc), hipMemcpyHostToDevice));
  return 0;
}

// ---- two one-tape fills side by side ------------------------------------------------------------------------------------------
// g_stream and the second stream forked: the second stream starts after what g_stream has queued so far (descriptors), join()
// makes g_stream wait for what the second one ran since.  The events go on every path.
struct StreamFork {
  hipStream_t s2 = second_stream();
  hipEvent_t evStart = nullptr, evDone = nullptr;
  bool ok;
  StreamFork() {
    ok = s2 && hipEventCreateWithFlags(&evStart, hipEventDisableTiming) == hipSuccess && hipEventCreateWithFlags(&evDone, hipEventDisableTiming) == hipSuccess &&
         hipEventRecord(evStart, g_stream) == hipSuccess && hipStreamWaitEvent(s2, evStart, 0) == hipSuccess;
  }
  bool join() { return ok && hipEventRecord(evDone, s2) == hipSuccess && hipStreamWaitEvent(g_stream, evDone, 0) == hipSuccess; }
  ~StreamFork() { if (evStart) (void)hipEventDestroy(evStart); if (evDone) (void)hipEventDestroy(evDone); }
};

// A Forward-direction fill (program WF over descriptors d_f / h_f into dstF) and a Backward-direction one (WB, d_b / h_b, dstB) of
// the same n sequences of a one-tape machine, which are independent: both in ONE launch when the programs share a kernel variant,
// else two launches on two streams, joined before this returns.  keepColumns: only the last column of each sequence is kept (the
// split Forward) instead of the matrix.  With CUs to spare each fill runs k workgroups per sequence on half the chip; a machine whose
// ring lives in L2 and whose parts fit the LDS only when a sweep has the whole chip runs one fill after the other on all of it.
// Returns 0, an error, or -1 when nothing ran: the programs share no kernel and there is no second stream (a caller that asked for
// the stream up front never sees that).  forkError / joinError: the texts of the two stream failures.
static int onetape_fill_pair(mb_machine *m, WideProgram &WF, WideProgram &WB, const PairDesc *d_f, const PairDesc *d_b, const PairDesc *h_f,
                             const PairDesc *h_b, long long n, const int *tape, double *dstF, double *dstB, bool keepColumns,
                             const char *forkError, const char *joinError) {
  hipStream_t s2 = second_stream();
  const int cus = device_cus();
  bool parts = s2 && wide_parts_for(m, WF, n, cus / 2, h_f) > 1 && wide_parts_for(m, WB, n, cus / 2, h_b) > 1;
  const bool oneByOne = s2 && !parts && (WF.retGv || WB.retGv) && wide_parts_for(m, WF, n, cus, h_f) > 1 && wide_parts_for(m, WB, n, cus, h_b) > 1;
  parts = parts || oneByOne;
  const int share = oneByOne ? 1 : 2;
  const int fused = parts ? -1 : wide_fill2(m, WF, WB, d_f, d_b, n, n, tape, dstF, dstB, g_stream, keepColumns);   // both sweeps in ONE launch
  if (fused >= 0 || !s2) return fused;
  // (programs of different kernel variants: two launches on two streams)
  StreamFork fork;
  if (!fork.ok) { set_error(forkError); return 1; }
  int rc = wide_fill(m, WF, d_f, n, tape, dstF, nullptr, oneByOne ? g_stream : s2, keepColumns, parts ? h_f : nullptr, cus / share);
  if (!rc) rc = wide_fill(m, WB, d_b, n, tape, dstB, nullptr, g_stream, keepColumns, parts ? h_b : nullptr, cus / share);
  if (!fork.join()) { set_error(joinError); rc = 1; }
  return rc;
}

// ---- Forward ------------------------------------------------------------------------------------------------
// Each route below leaves the log-likelihoods of the batch in d_ll (device, nPairs entries); run_fill_loglike chooses.

// One-tape machine, fewer sequences than half the CUs (one workgroup per sequence): every sequence is CUT IN TWO -- Forward over
// the prefix and Backward over the suffix behind the cut run side by side, k_onetape_join sums over the emitting transitions that
// cross the cut.  Same likelihood (a different summation order: ~1e-12 relative), half the sweep length.
static int forward_onetape_split(mb_batch *b, WideProgram &W, double *d_ll) {
  mb_machine *m = b->m;
  WideProgram *WB = wide_program(m, MB_BACKWARD);
  const long long n = b->nPairs, S = m->S;
  std::vector<PairDesc> pre, suf;
  auto cutAt = [&](double frac) {
    pre = b->pairs; suf = b->pairs;
    for (long long p = 0; p < n; ++p) {
      const int L = m->nOut ? b->pairs[p].outLen : b->pairs[p].inLen, mid = std::min(L - 1, std::max(0, (int)(L * frac)));
      pre[p].cellBase = suf[p].cellBase = p * S;
      if (m->nOut) { pre[p].outLen = mid; suf[p].outBase += mid + 1; suf[p].outLen = L - mid - 1; }
      else { pre[p].inLen = mid; suf[p].inBase += mid + 1; suf[p].inLen = L - mid - 1; }
    }
  };
  cutAt(0.5);
  // k workgroups per sequence: the two programs' parts are not equally fast (the Backward program of the 5 063-state machine takes 136 ms
  // where the Forward one takes 120): the cut goes where both halves end together under the planner's model
  if (WB) {
    const double cF = wide_parts_cost(m, W, n, device_cus() / 2, pre.data()), cB = wide_parts_cost(m, *WB, n, device_cus() / 2, suf.data());
    if (cF > 0.0 && cB > 0.0 && opt_int<MB_ONETAPE_SPLIT_BALANCE>()) cutAt(std::min(0.65, std::max(0.35, cB / (cF + cB))));
  }
  if (!WB) return 1;
  SmBuf<PairDesc> d_pre, d_suf;
  if (!hip_ok(d_pre.alloc(n), "hipMalloc") || !hip_ok(d_suf.alloc(n), "hipMalloc")) return 1;
  double *vec = (double *)ws_get(2, (size_t)(2 * n * S) * sizeof(double));
  if (!vec) return 1;
  if (!hip_ok(hipMemcpyAsync(d_pre, pre.data(), n * sizeof(PairDesc), hipMemcpyHostToDevice, g_stream), "H2D") ||
      !hip_ok(hipMemcpyAsync(d_suf, suf.data(), n * sizeof(PairDesc), hipMemcpyHostToDevice, g_stream), "H2D") ||
      !hip_ok(hipStreamSynchronize(g_stream), "H2D")) { quiesce_streams(); return 1; }   // (pre / suf are pageable host vectors)
  int rc = timed([&] {
    if (onetape_fill_pair(m, W, *WB, d_pre, d_suf, pre.data(), suf.data(), n, tape_of(b), vec, vec + n * S, true,
                          "one-tape split: stream set-up failed", "one-tape split: stream synchronisation failed")) return 1;
    return wide_join(m, d_pre, n, tape_of(b), vec, vec + n * S, d_ll, g_stream);
  });
  if (!rc) { static thread_local std::string nm; nm = std::string(wide_kernel_name(W)) + " x2 + k_onetape_join"; g_last_kernel = nm.c_str(); }
  if (!rc && !hip_ok(hipStreamSynchronize(g_stream), "one-tape forward kernels")) rc = 1;
  if (!rc && wide_parts_failed()) rc = 1;
  if (rc) quiesce_streams();      // (the halves may still read the descriptors freed on return)
  return rc;
}

// one-tape machine, log-likelihood only: the two live columns of every sequence stay in LDS, nothing goes to HBM
static int forward_onetape(mb_batch *b, double *d_ll) {
  mb_machine *m = b->m;
  WideProgram *W = wide_program(m, MB_FORWARD);
  if (!W) return 1;
  int minLen = 1 << 30;
  for (const PairDesc &pd : b->pairs) minLen = std::min(minLen, m->nOut ? pd.outLen : pd.inLen);
  if (opt_int<MB_ONETAPE_SPLIT>() && 2 * b->nPairs <= device_cus() && minLen >= opt_int<MB_ONETAPE_SPLIT_MIN_LEN>() && second_stream())
    return forward_onetape_split(b, *W, d_ll);
  int rc = timed([&] { return wide_fill(m, *W, b->d_pairs, b->nPairs, tape_of(b), nullptr, d_ll, g_stream, false, b->pairs.data(), device_cus()); });
  g_last_kernel = wide_kernel_name(*W);
  if (!rc && !hip_ok(hipStreamSynchronize(g_stream), "one-tape forward kernel")) rc = 1;
  if (!rc && wide_parts_failed()) rc = 1;
  return rc;
}

// tiled family, log-likelihoods only, few pairs or envelopes: the tile pipeline WITHOUT a matrix (halo columns + boundary records).
// Returns -1 when its kernel is unavailable: nothing was written, another route takes the call.
static int forward_rolltiles(mb_batch *b, double *d_ll) {
  FastState *f = fast_state(b->m);
  std::vector<PairDesc> hp(b->pairs);
  int rc = launch_fill_neg_inf(d_ll, b->nPairs, g_stream);
  if (!rc) rc = timed([&] { return medium_forward_rolltiles(b->m, f->fwdSum, f->geoFS, b->d_pairs, hp, b->d_in, b->d_out, d_ll, g_stream, med_env(b)); });
  if (rc < 0) return -1;
  g_last_kernel = "k_medium_jit";
  if (!rc && !hip_ok(hipStreamSynchronize(g_stream), "rolling forward kernels")) rc = 1;
  return rc;
}

// tiled family, RollingOutputForwardMatrix: no matrix in HBM, only two halo columns per pair.  It runs ONE workgroup per pair: with
// fewer pairs than CUs the tile pipeline (which cuts every pair into hundreds of tiles and recycles matrix slots) fills the chip
// better, and only the log-likelihoods are kept either way (psw2dna, 64 pairs: 229 vs 517 G cells/s) -- see fewPairs in the selector.
static int forward_rolling_halo(mb_batch *b, double *d_ll) {
  mb_machine *m = b->m;
  FastState *f = fast_state(m);
  std::vector<long long> hb(b->nPairs);
  long long tot = 0;
  for (long long p = 0; p < b->nPairs; ++p) { hb[p] = tot; tot += 2ll * (b->pairs[p].outLen + 1) * m->S; }
  double *d_halo = (double *)ws_get(2, std::max<long long>(tot, 1) * sizeof(double));
  if (!d_halo) return 1;
  SmBuf<long long> d_hb;
  if (!hip_ok(d_hb.alloc(b->nPairs), "hipMalloc")) return 1;
  if (!hip_ok(hipMemcpyAsync(d_hb, hb.data(), b->nPairs * sizeof(long long), hipMemcpyHostToDevice, g_stream), "H2D")) return 1;
  int rc = timed([&] { return medium_forward_rolling(m, f->fwdSum, f->geoFS, b->d_pairs, b->pairs, b->d_in, b->d_out, d_halo, d_hb, d_ll, g_stream); });
  g_last_kernel = (medium_jit_ready(f->fwdSum, MB_FORWARD, MED_MAT_NONE) || medium_jit_ready(f->fwdSum, MB_FORWARD, MED_MAT_ROLL)) ? "k_medium_jit" : "k_medium_tile<0>";
  if (!rc && !hip_ok(hipStreamSynchronize(g_stream), "rolling forward kernel")) rc = 1;
  return rc;
}

// tiled family, the matrices of the batch do not fit the device-memory budget together: ForwardMatrix semantics with only logLike()
// kept -- a continuous pipeline over recycled matrix slots
static int forward_pipelined(mb_batch *b, double *d_ll) {
  mb_machine *m = b->m;
  FastState *f = fast_state(m);
  const size_t budget = budget_bytes();
  const long long want = std::min<long long>(b->totalCells, (long long)(budget / 8));
  double *pool = (double *)ws_get(0, (size_t)std::max<long long>(want, b->maxPairCells) * sizeof(double));
  if (!pool) return 1;
  const long long poolCells = (long long)(ws_bytes(0) / 8);
  if (poolCells < b->maxPairCells) { set_error("a single DP matrix exceeds the device memory budget"); return 1; }
  Timer tm;
  Timed t(tm, 0);
  int rc = medium_forward_pipelined(m, f->fwdSum, f->geoFS, b->pairs, b->d_in, b->d_out, pool, poolCells, d_ll, g_stream, !m->mediumPersistOff);
  if (rc == 2) {      // a persistent strip waited longer than MB_MEDIUM_PERSIST_TIMEOUT_S: latched off for this machine, the call runs again launch by launch
    m->mediumPersistOff = true;
    fprintf(stderr, "[mbhip] WARNING: a persistent strip of the pipelined Forward waited longer than MB_MEDIUM_PERSIST_TIMEOUT_S for another strip (is the device shared?): the call is run again launch by launch, and so are this machine's later calls\n");
    rc = medium_forward_pipelined(m, f->fwdSum, f->geoFS, b->pairs, b->d_in, b->d_out, pool, poolCells, d_ll, g_stream, false);
  }
  g_last_kernel = (medium_jit_ready(f->fwdSum, MB_FORWARD, MED_MAT_FULL) || medium_jit_ready(f->fwdSum, MB_FORWARD, MED_MAT_PERSIST)) ? "k_medium_jit" : "k_medium_tile<0>";
  return rc;
}

// every other case: the matrices of a chunk materialised by fill_chunk, the end cells gathered
static int forward_chunked(mb_batch *b, int mode, double *d_ll) {
  std::vector<Chunk> chunks;
  if (!plan_chunks(b, 1, chunks)) return 1;
  return for_chunks<DescPlan>(chunks, desc_build(b), [&](const Chunk &c, DescPlan &pl, Timer &tm) {
    double *pool = (double *)ws_get(0, std::max<long long>(c.cells, 1) * sizeof(double));
    if (!pool) return 1;
    {
      Timed t(tm, 0);
      if (const int rc = fill_chunk(b->m, mode, pl.d, pl.hp, b->d_in, b->d_out, pool, 0, b)) return rc;
      if (const int rc = launch_gather_loglike(pl.d, c.p1 - c.p0, pool, b->m->S, 0, d_ll + c.p0, g_stream)) return rc;
    }
    if (!hip_ok(hipStreamSynchronize(g_stream), "fill kernel")) return 1;
    return wide_parts_failed() ? 1 : 0;
  });
}

static int run_fill_loglike(mb_batch *b, int mode, int flags, double *loglike) {
  reset_last();
  if (b->nPairs == 0) return 0;
  mb_machine *m = b->m;
  const bool fwd = mode == MB_FORWARD, rolling = (flags & MB_ROLLING) != 0;
  if (fwd && use_small(m) && small_can_run(((FastState *)m->fast)->smF, SM_SUM, !rolling, b->hasEnv)) return small_forward(b, flags, loglike);
  SmBuf<double> d_ll;
  MB_HIP(d_ll.alloc(b->nPairs));
  const bool belowMinPairs = b->nPairs < opt_int<MB_ROLLING_MIN_PAIRS>();
  const bool fewPairs = belowMinPairs && (size_t)b->maxPairCells * 8 * 2 <= budget_bytes();
  int rc = -1;      // (-1: no route has taken the call yet)
  if (fwd && !b->hasEnv && wide_applicable(m) && g_kernel_choice != 1 && (rolling || (size_t)b->totalCells * 8 > budget_bytes()))
    rc = forward_onetape(b, d_ll);
  else if (fwd && rolling && use_medium(m) && !wide_applicable(m) && opt_int<MB_MEDIUM_ROLLTILES>() && (belowMinPairs || b->hasEnv))
    rc = forward_rolltiles(b, d_ll);      // -1: its kernel is unavailable -- the routes below take the call, from a clean slate
  if (rc < 0) {
    reset_last();
    if (fwd && rolling && !fewPairs && !b->hasEnv && use_medium(m)) rc = forward_rolling_halo(b, d_ll);
    else if (fwd && !b->hasEnv && use_medium(m) && opt_int<MB_MEDIUM_PIPELINE>() && (size_t)b->totalCells * 8 > budget_bytes()) rc = forward_pipelined(b, d_ll);
    else rc = forward_chunked(b, mode, d_ll);
  }
  if (!rc) rc = fetch_loglike(loglike, d_ll, b->nPairs);
  return rc;
}

// A one-tape sweep with k workgroups per sequence whose exchange timed out (the device is shared, a CU mask is set: the parts were
// not co-resident) has latched its programs to one workgroup per sequence: the call is run once more instead of failing.
static int with_parts_retry(const std::function<int()> &run) {
  int rc = run();
  if (rc > 0 && wide_parts_retry()) {
    (void)hipStreamSynchronize(g_stream);
    rc = run();
  }
  if (rc) wide_parts_reset();
  return rc;
}

int mb_batch_forward(mb_batch *b, int flags, double *loglike) {
  ApiGuard guard;
  if (!b || !loglike) { set_error("null argument"); return 1; }
  return with_parts_retry([&] { return run_fill_loglike(b, MB_FORWARD, flags, loglike); });
}

// ---- Viterbi ------------------------------------------------------------------------------------------------
int64_t mb_viterbi_path_bound(const mb_machine *m, int64_t inLen, int64_t outLen) {
  if (!m) return 0;
  // between two emitting steps the traceback follows silent edges to strictly lower states through at most
  // nLevF-1 levels; one more run may precede the first emission.
  return (inLen + outLen + 1) * (int64_t)m->nLevF + 1;
}

// ViterbiMatrix over a batch on the tiled / generic / one-tape families.
// tb: 0 = fp64 Viterbi matrices, 1 = the tiled family's traceback bytes (ONE byte per cell, run-time specialised kernel), 2 = the
// one-tape family's traceback codes.  tb 1 / 2 return -1 before anything was written when their kernel is unavailable.
static int viterbi_chunks(mb_batch *b, double *loglike, int64_t *pathOff, uint32_t *pathEdges, int64_t pathCap, int tb) {
  mb_machine *m = b->m;
  const bool wantPaths = pathEdges != nullptr && pathOff != nullptr;
  const int Sb = tb == 2 ? wide_tb_stride(m->S) : medium_tb_stride(m->S);
  std::vector<Chunk> chunks;
  if (!plan_chunks(b, 1, chunks, tb ? (double)Sb / m->S + 0.01 : 0.0)) return 1;
  PathOut out{pathOff, pathEdges, pathCap};
  Laps laps;
  return for_chunks<DescPlan>(chunks, desc_build(b, tb ? Sb : 0), [&](const Chunk &c, DescPlan &pl, Timer &tm) {
    const long long np = c.p1 - c.p0;
    const std::vector<PairDesc> &hp = pl.hp;
    const PairDesc *d_desc = pl.d;
    double *pool = (double *)ws_get(0, tb ? (size_t)std::max<long long>(c.cells / m->S * Sb, 16) : std::max<long long>(c.cells, 1) * sizeof(double));
    if (!pool) return 1;
    const unsigned char *bytes = (const unsigned char *)pool;      // (tb: the pool holds traceback bytes / codes)
    SmBuf<double> d_ll;
    if (!hip_ok(d_ll.alloc(np), "hipMalloc")) return 1;
    laps.lap("chunk set-up");
    PathSlots ps;
    {
      Timed t(tm, 0);
      if (tb == 2) {
        WideProgram *W = wide_tb_program(m);
        if (!W && c.p0 == 0) return -1;
        if (!W) { set_error("one-tape traceback-code program became unavailable mid-batch"); return 1; }
        if (const int rc = wide_fill_tb(m, *W, d_desc, np, tape_of(b), (unsigned char *)pool, d_ll, g_stream, hp.data(), device_cus())) return rc;
        g_last_kernel = wide_kernel_name(*W);      // (the generated kernel or the interpreter, one workgroup or k: asked after the launch)
      } else if (tb) {
        if (const int rc = launch_fill_neg_inf(d_ll, np, g_stream)) return rc;   // (a pair whose end cell lies in a tile that does not run)
        MedGeom *tbGeo = nullptr;
        MedProgram *tbP = medium_tb_program(m, &tbGeo);
        int rc = tbP ? medium_viterbi_tb(m, *tbP, *tbGeo, d_desc, hp, b->d_in, b->d_out, (unsigned char *)pool, d_ll, g_stream, med_env(b)) : -1;
        if (rc < 0 && c.p0 > 0) { set_error("traceback-byte Viterbi kernel became unavailable mid-batch"); rc = 1; }
        if (rc) return rc;
        g_last_kernel = "k_medium_jit";
      } else {
        if (const int rc = fill_chunk(m, MB_VITERBI, d_desc, hp, b->d_in, b->d_out, pool, 0, b)) return rc;
        if (const int rc = launch_gather_loglike(d_desc, np, pool, m->S, 0, d_ll, g_stream)) return rc;
      }
      if (wantPaths) {
        if (path_slots(b, c, ps)) return 1;
        int rc;
        if (tb == 2) rc = wide_traceback_codes(m, *wide_tb_program(m), d_desc, np, bytes, d_ll, ps.d_slot, ps.d_path, ps.d_len, g_stream);
        else if (tb) rc = launch_traceback_bytes(m, d_desc, np, b->d_in, b->d_out, bytes, Sb, d_ll, ps.d_slot, ps.d_path, ps.d_len, g_stream);
        else {
          // one-tape machines beyond the LDS edge tables of the generic walkers: columns in LDS, one trip to memory per step
          WideTbPlan *T = nullptr;
          if (wide_applicable(m) && g_kernel_choice != 1 && m->nTrans > opt_int<MB_ONETAPE_TRACEBACK_MIN_TRANS>() && !b->hasEnv) {
            FastState *f = fast_state(m);
            if (!f->wTb.tried) (void)wide_traceback_build(m, f->wTb);
            if (f->wTb.ok) T = &f->wTb;
          }
          rc = T ? wide_traceback(m, *T, d_desc, np, tape_of(b), pool, ps.d_slot, ps.d_path, ps.d_len, g_stream)
                 : launch_traceback(m, d_desc, np, b->d_in, b->d_out, pool, ps.d_slot, ps.d_path, ps.d_len, g_stream);
        }
        if (rc) return rc;
      }
      laps.lap("launches (host side)");
    }
    if (!hip_ok(hipStreamSynchronize(g_stream), "viterbi kernels")) return 1;
    if (wide_parts_failed()) return 1;
    laps.lap("kernels");
    if (fetch_loglike(loglike + c.p0, d_ll, np)) return 1;
    return wantPaths ? pack_paths(out, c, ps, PATH_OVERFLOW, PATH_DEAD_END, laps) : 0;
  });
}

static int batch_viterbi(mb_batch *b, double *loglike, int64_t *pathOff, uint32_t *pathEdges, int64_t pathCap);
int mb_batch_viterbi(mb_batch *b, double *loglike, int64_t *pathOff, uint32_t *pathEdges, int64_t pathCap) {
  ApiGuard guard;
  if (!b || !loglike) { set_error("null argument"); return 1; }
  return with_parts_retry([&] { return batch_viterbi(b, loglike, pathOff, pathEdges, pathCap); });
}
static int batch_viterbi(mb_batch *b, double *loglike, int64_t *pathOff, uint32_t *pathEdges, int64_t pathCap) {
  reset_last();
  if (pathOff) pathOff[0] = 0;
  if (b->nPairs == 0) return 0;
  if (use_small(b->m) && small_can_run(((FastState *)b->m->fast)->smF, SM_TB, false, b->hasEnv)) return small_viterbi(b, loglike, pathOff, pathEdges, pathCap);
  // tiled family: one traceback byte per cell when the machine's exact program allows it
  MedGeom *tbGeo = nullptr;
  if (!wide_applicable(b->m) && use_medium(b->m) && opt_int<MB_MEDIUM_TB>() && medium_tb_program(b->m, &tbGeo) &&
      traceback_bytes_lds(b->m, medium_tb_stride(b->m->S))) {
    const int rc = viterbi_chunks(b, loglike, pathOff, pathEdges, pathCap, 1);
    if (rc >= 0) return rc;
    reset_last();
    if (pathOff) pathOff[0] = 0;
  }
  // one-tape family: one traceback code per cell when paths are wanted (a fill without paths keeps the leaner fp64 sweep).
  // MB_ONETAPE_TB=0 forbids it (the walker then re-evaluates candidates on the fp64 Viterbi matrix).  The code sweep costs 13 % over
  // the plain max sweep (a compare and a select per candidate, a second butterfly over the places), its walker half of the fp64
  // walker, and it moves an eighth of the bytes: 64 x 50 kb on the 5 063-state machine 315 vs 346 ms with 16 instead of 130 GB,
  // 256 x 4 kb 28 vs 42 ms, 64 x 2 kb 13.3 vs 14.2, the whole fn3 composite (L2-resident ring) 158 vs 171 -- and 557 GB of fp64 for
  // that machine at 64 x 50 kb could not be resident at all.  (Until the reduction was split into two butterflies the sweep cost
  // 29 % and the route was taken only when memory asked for it.)
  const bool tbWanted = opt_int<MB_ONETAPE_TB>() != 0;
  if (pathEdges && pathOff && !b->hasEnv && tbWanted && wide_tb_program(b->m)) {
    const int rc = viterbi_chunks(b, loglike, pathOff, pathEdges, pathCap, 2);
    if (rc >= 0) return rc;
    reset_last();
    pathOff[0] = 0;
  }
  return viterbi_chunks(b, loglike, pathOff, pathEdges, pathCap, 0);
}

// ---- Forward-Backward counts --------------------------------------------------------------------------------
// One-tape E-step over LONG sequences: the fills carry their log-sum-exp correction term in fp64 (mb_wide.hip, wide_exp64): the
// fp32 term's per-column error repeats in stationary states and grows linearly with the length (7.6e-5 per transition at 50 000
// columns).  MB_ONETAPE_COUNT_FP64: 1 always, 0 never, default: sequences of >= MB_ONETAPE_COUNT_FP64_MIN_LEN (10 000) symbols.
struct AccurateFills { bool on; explicit AccurateFills(bool o) : on(o) { if (on) wide_set_accurate(true); } ~AccurateFills() { if (on) wide_set_accurate(false); } };
static bool accurate_fills_wanted(const mb_machine *m, const std::vector<PairDesc> &hp) {
  int longest = 0;
  for (const PairDesc &pd : hp) longest = std::max(longest, std::max(pd.inLen, pd.outLen));
  const int accMode = opt_int<MB_ONETAPE_COUNT_FP64>();
  return wide_applicable(m) && (accMode == 1 || (accMode != 0 && longest >= opt_int<MB_ONETAPE_COUNT_FP64_MIN_LEN>()));
}

// roll: the tiled family's count sweep WITHOUT a Forward matrix (medium_counts_rolling) -- one matrix per pair instead of two,
// so twice the pairs per chunk; returns -1 before anything was accumulated when that kernel is unavailable
// usage3: both matrices materialised by the plain fills, then the dependency-free usage pass of mb_usage.hip (tiled family)
static int counts_chunks(mb_batch *b, double *counts, double *loglikeSum, double *loglike, bool roll, bool usage3 = false) {
  mb_machine *m = b->m;
  const long long nT = m->nTrans;
  std::vector<Chunk> chunks;
  if (!plan_chunks(b, roll ? 1 : 2, chunks)) return 1;
  SmBuf<double> d_counts, d_ll;
  if (!hip_ok(d_counts.alloc(nT), "hipMalloc(counts)")) return 1;
  if (!hip_ok(d_ll.alloc(b->nPairs), "hipMalloc(loglike)") ||
      !hip_ok(hipMemsetAsync(d_counts, 0, std::max<long long>(nT, 1) * sizeof(double), g_stream), "memset(counts)")) return 1;
  const int rc = for_chunks<DescPlan>(chunks, desc_build(b), [&](const Chunk &c, DescPlan &pl, Timer &tm) {
    const long long np = c.p1 - c.p0;
    const std::vector<PairDesc> &hp = pl.hp;
    const PairDesc *d_desc = pl.d;
    double *fwd = nullptr, *bwd = nullptr;
    { const size_t need = (size_t)std::max<long long>(c.cells, 1) * sizeof(double); const int sl[2] = {1, 0}; const size_t nb[2] = {need, need}; ws_plan(roll ? 1 : 2, sl, nb); }
    if (!roll && !(fwd = (double *)ws_get(0, std::max<long long>(c.cells, 1) * sizeof(double)))) return 1;
    if (!(bwd = (double *)ws_get(1, std::max<long long>(c.cells, 1) * sizeof(double)))) return 1;
    long long maxc = 0;
    for (long long p = c.p0; p < c.p1; ++p)
      maxc = std::max(maxc, (long long)(b->pairs[p].inLen + 1) * (b->pairs[p].outLen + 1) * m->S);
    {
      Timed t(tm, 0);
      const AccurateFills accurateFills(accurate_fills_wanted(m, hp));
      // One-tape machine (one workgroup per sequence): the Backward and the Forward fill are independent and a batch of fewer
      // sequences than CUs leaves most of the chip idle, so the two run side by side (64 sequences: 64 + 64 CUs); the count kernel
      // waits for both.  Without a second stream, programs that share no kernel are filled one after the other below.
      bool fwdDone = false;
      if (!roll && !b->hasEnv && wide_applicable(m) && g_kernel_choice != 1 && opt_int<MB_ONETAPE_CONCURRENT_FILLS>()) {
        WideProgram *WB = wide_program(m, MB_BACKWARD), *WF = wide_program(m, MB_FORWARD);
        if (!WB || !WF) return 1;
        const int rc = onetape_fill_pair(m, *WF, *WB, d_desc, d_desc, hp.data(), hp.data(), np, tape_of(b), fwd, bwd, false,
                                         "one-tape counts: stream synchronisation failed", "one-tape counts: stream synchronisation failed");
        if (rc > 0) return rc;
        if (rc == 0) { fwdDone = true; g_last_kernel = wide_kernel_name(*WF); }
      }
      if (!fwdDone) if (const int rc = fill_chunk(m, MB_BACKWARD, d_desc, hp, b->d_in, b->d_out, bwd, 0, b)) return rc;
      // fused path: the Forward sweep accumulates the counts while its anti-diagonals are still in LDS
      int fused = -1;
      if (roll) {
        FastState *f = fast_state(m);
        if (const int rc = launch_fill_neg_inf(d_ll + c.p0, np, g_stream)) return rc;   // (a pair whose end cell lies in a tile that does not run)
        fused = medium_counts_rolling(m, f->fwdCnt, f->geoCnt, d_desc, hp, b->d_in, b->d_out, bwd, d_counts, d_ll + c.p0, g_stream, med_env(b));
        if (fused < 0 && c.p0 == 0) return -1;      // kernel unavailable: the caller runs the two-matrix path
        if (fused) { if (fused < 0) set_error("count sweep kernel became unavailable mid-batch"); return 1; }
        g_last_kernel = "k_medium_jit";
      } else if (usage3) {
        // (fused stays -1: Forward fill, log-likelihoods, then the usage pass below)
      } else if (use_medium(m) && fast_state(m)->countOk && !(b->hasEnv && wide_applicable(m))) {
        FastState *f = fast_state(m);
        if (b->hasEnv) if (const int rc = launch_fill_neg_inf(fwd, c.cells, g_stream)) return rc;      // tiles outside the envelopes do not run
        fused = medium_counts_materialised(m, f->fwdCnt, f->geoCnt, d_desc, hp, b->d_in, b->d_out, fwd, bwd, d_counts, d_ll + c.p0, g_stream, med_env(b));
        if (fused > 0) return 1;
        if (fused == 0) g_last_kernel = "k_medium_jit";
      }
      if (fused < 0) {
        if (!fwdDone) if (const int rc = fill_chunk(m, MB_FORWARD, d_desc, hp, b->d_in, b->d_out, fwd, 0, b)) return rc;
        if (const int rc = launch_gather_loglike(d_desc, np, fwd, m->S, 0, d_ll + c.p0, g_stream)) return rc;
        // one-tape machines: a lane owns a transition and walks the columns (mb_wide.hip); two tapes: one thread per cell
        const bool oneTape = ((m->nIn != 0) != (m->nOut != 0)) && g_kernel_choice != 1 && opt_int<MB_ONETAPE_COUNTS>();
        int rc;
        if (usage3) {
          rc = usage_launch(m, fast_state(m)->usage, d_desc, hp, b->d_in, b->d_out, fwd, bwd, d_counts, g_stream);
          if (!rc) g_last_kernel = "k_medium_jit (two fills) + k_medium_usage";
        } else if (oneTape) {
          FastState *f = fast_state(m);
          if (!f->wCnt.ok && !wide_counts_build(m, f->wCnt)) return 1;
          rc = wide_counts(m, f->wCnt, d_desc, hp, tape_of(b), fwd, bwd, d_counts, g_stream);
          if (!rc) g_last_kernel = "k_onetape_counts";
        } else rc = launch_generic_counts(m, d_desc, np, maxc, b->d_in, b->d_out, fwd, bwd, d_counts, g_stream);
        if (rc) return rc;
      }
    }
    if (!hip_ok(hipStreamSynchronize(g_stream), "counts kernels")) return 1;
    return wide_parts_failed() ? 1 : 0;
  });
  if (rc) return rc;
  CountSum sum(nT);
  std::vector<double> hll((size_t)b->nPairs);
  if (sum.add(d_counts, g_deterministic) || fetch_loglike(hll.data(), d_ll, b->nPairs)) return 1;
  sum.finish(hll, counts, loglikeSum, loglike);      // loglike += forward.logLike()
  return 0;
}

static int batch_counts(mb_batch *b, double *counts, double *loglikeSum, double *loglike);
int mb_batch_counts(mb_batch *b, double *counts, double *loglikeSum, double *loglike) {
  ApiGuard guard;
  if (!b || !counts) { set_error("null argument"); return 1; }
  return with_parts_retry([&] { return batch_counts(b, counts, loglikeSum, loglike); });      // (the counts reach the caller's array after the last chunk only: a second run adds nothing twice)
}
static int batch_counts(mb_batch *b, double *counts, double *loglikeSum, double *loglike) {
  reset_last();
  latch_deterministic();
  if (b->nPairs == 0) return 0;
  if (use_small(b->m) && small_count_fits(((FastState *)b->m->fast)->smF, b->hasEnv) && small_can_run(((FastState *)b->m->fast)->smB, SM_SUM, true, b->hasEnv))
    return small_counts(b, counts, loglikeSum, loglike);
  // Tiled family, two ways: the FUSED sweep (Backward fill, then a Forward sweep that weighs the transitions while its cells are in LDS:
  // 16 B per lattice cell, one matrix per pair) or THREE passes (both fills materialised, then the dependency-free usage pass of
  // mb_usage.hip).  Measured on the 482-state composition at 24 x 487 aa x 10 kb: fused 593 ms; three passes 946 ms -- the usage pass
  // itself 286 ms, but two matrices per pair leave 6 pairs per chunk and the two fills of such a chunk cannot fill the chip (660 ms
  // where 256 pairs through the pipeline would take 280).  So the fused sweep is the default; MB_MEDIUM_COUNT_PASSES=3 asks for the three
  // passes (a host with few long pairs and memory to spare; the parity tests).
  if (!wide_applicable(b->m) && use_medium(b->m) && !b->hasEnv) {
    const int passes = opt_int<MB_MEDIUM_COUNT_PASSES>();
    FastState *f = fast_state(b->m);
    if (f->mediumOk && passes == 3 && (size_t)b->maxPairCells * 16 <= budget_bytes()) {
      if (!f->usage.tried) usage_build(b->m, f->usage);
      if (f->usage.ok) return counts_chunks(b, counts, loglikeSum, loglike, false, true);
    }
  }
  if (!wide_applicable(b->m) && use_medium(b->m) && fast_state(b->m)->countOk && opt_int<MB_MEDIUM_COUNTS_ROLL>()) {
    const int rc = counts_chunks(b, counts, loglikeSum, loglike, true);
    if (rc >= 0) return rc;
    reset_last();
  }
  return counts_chunks(b, counts, loglikeSum, loglike, false);
}

// ---- single full matrix -------------------------------------------------------------------------------------
int mb_fill_env(mb_machine *m, int mode, const int32_t *in, int64_t inLen, const int32_t *out, int64_t outLen,
                int32_t startState, const int32_t *envStart, const int32_t *envEnd, double *cellsOut) {
  ApiGuard guard;
  if (!m || !cellsOut) { set_error("null argument"); return 1; }
  if (mode < MB_FORWARD || mode > MB_BACKWARD) { set_error("mb_fill: unknown mode"); return 1; }
  if (startState < 0 || startState >= m->S) { set_error("mb_fill: start state out of range"); return 1; }
  const int64_t inOff[2] = {0, inLen}, outOff[2] = {0, outLen};
  mb_batch *b = mb_batch_create(m, 1, in, inOff, out, outOff);
  if (!b) return 1;
  if (envStart && envEnd) {
    const int64_t envOff[2] = {0, outLen + 1};
    if (mb_batch_set_envelopes(b, envOff, envStart, envEnd)) { mb_batch_destroy(b); return 1; }
  }
  if (startState == 0 && use_small(m) &&
      small_can_run(mode == MB_BACKWARD ? ((FastState *)m->fast)->smB : ((FastState *)m->fast)->smF, mode == MB_VITERBI ? SM_MAX : SM_SUM, true, b->hasEnv)) {
    const int rcs = small_fill(b, mode, cellsOut);
    mb_batch_destroy(b);
    return rcs;
  }
  const long long n = b->totalCells;
  double *pool = nullptr;
  int rc = 0;
  if (n * 8ull > budget_bytes()) { set_error("matrix exceeds the device memory budget"); rc = 1; }
  if (!rc && !(pool = (double *)ws_get(0, n * sizeof(double)))) rc = 1;
  if (!rc && opt_int<MB_DEBUG_POISON>()) (void)hipMemsetAsync(pool, 0xFF, n * sizeof(double), g_stream);
  for (int attempt = 0; attempt < 2 && !rc; ++attempt) {      // (a second time when the exchange between the parts of a one-tape sweep timed out: see with_parts_retry)
    rc = fill_chunk(m, mode, b->d_pairs, b->pairs, b->d_in, b->d_out, pool, mode == MB_FORWARD ? startState : 0, b);
    if (!rc && !hip_ok(hipStreamSynchronize(g_stream), "fill kernel")) rc = 1;
    if (!rc && wide_parts_failed()) { if (attempt == 0 && wide_parts_retry()) continue; rc = 1; }
    break;
  }
  if (rc) wide_parts_reset();
  if (!rc && !hip_ok(hipMemcpy(cellsOut, pool, n * sizeof(double), hipMemcpyDeviceToHost), "D2H matrix")) rc = 1;
  mb_batch_destroy(b);
  return rc;
}

int mb_fill(mb_machine *m, int mode, const int32_t *in, int64_t inLen, const int32_t *out, int64_t outLen,
            int32_t startState, double *cellsOut) {
  return mb_fill_env(m, mode, in, inLen, out, outLen, startState, nullptr, nullptr, cellsOut);
}

// ---- introspection: the persistent-strip plan of a batch (host only): tickets (pair, strip) and per pair (slot, strips to wait for) ----
int64_t mb_debug_persist_plan(int64_t nPairs, const int32_t *inLen, const int32_t *outLen, int32_t C, int64_t nSlots, int32_t *tickets, int64_t maxTickets, int32_t *wait) {
  ApiLock lock;
  if (nPairs < 0 || C < 1 || nSlots < 1 || (nPairs > 0 && (!inLen || !outLen || !wait))) { set_error("mb_debug_persist_plan: bad argument"); return -1; }
  std::vector<PairDesc> pairs((size_t)nPairs);
  for (int64_t p = 0; p < nPairs; ++p) { pairs[p].inLen = inLen[p]; pairs[p].outLen = outLen[p]; }
  std::vector<int2> tk, w;
  medium_persist_plan(pairs, C, nSlots, tk, w);
  if ((int64_t)tk.size() > maxTickets || (!tickets && !tk.empty())) { set_error("mb_debug_persist_plan: ticket buffer too small"); return -1; }
  for (size_t k = 0; k < tk.size(); ++k) { tickets[2 * k] = tk[k].x; tickets[2 * k + 1] = tk[k].y; }
  for (size_t p = 0; p < w.size(); ++p) { wait[2 * p] = w[p].x; wait[2 * p + 1] = w[p].y; }
  return (int64_t)tk.size();
}

// ---- host-buffer convenience wrappers -------------------------------------------------------------------------
int mb_forward_batch(mb_machine *m, int64_t nPairs, const int32_t *inTok, const int64_t *inOff, const int32_t *outTok,
                     const int64_t *outOff, int flags, double *loglike) {
  mb_batch *b = mb_batch_create(m, nPairs, inTok, inOff, outTok, outOff);
  if (!b) return 1;
  const int rc = mb_batch_forward(b, flags, loglike);
  mb_batch_destroy(b);
  return rc;
}

int mb_viterbi_batch(mb_machine *m, int64_t nPairs, const int32_t *inTok, const int64_t *inOff, const int32_t *outTok,
                     const int64_t *outOff, double *loglike, int64_t *pathOff, uint32_t *pathEdges, int64_t pathCap) {
  mb_batch *b = mb_batch_create(m, nPairs, inTok, inOff, outTok, outOff);
  if (!b) return 1;
  const int rc = mb_batch_viterbi(b, loglike, pathOff, pathEdges, pathCap);
  mb_batch_destroy(b);
  return rc;
}

int mb_counts_batch(mb_machine *m, int64_t nPairs, const int32_t *inTok, const int64_t *inOff, const int32_t *outTok,
                    const int64_t *outOff, double *counts, double *loglikeSum, double *loglike) {
  mb_batch *b = mb_batch_create(m, nPairs, inTok, inOff, outTok, outOff);
  if (!b) return 1;
  const int rc = mb_batch_counts(b, counts, loglikeSum, loglike);
  mb_batch_destroy(b);
  return rc;
}

// ---- prefix search: node fills on the device, the tree on the host (mb_prefix.hip, docs/decoding.md) --------------------------
static const int WS_PREFIX_POOL = 15;

static void prefix_free(mb_prefix *p) {
  sm_free(p->d_out); sm_free(p->d_logP); sm_free(p->d_colTok); sm_free(p->d_rOff); sm_free(p->d_rIdx); sm_free(p->d_rVal);   // (cached by size class: steady cycles allocate nothing)
  if (p->pool) {
    if (p->poolIsWorkspace) g_ws[WS_PREFIX_POOL].held = false;      // the memory stays cached for the next search
    else { (void)hipFree(p->pool); ++g_alloc.frees; }
  }
  delete p;
}

// The searches of one object decode either token strings (outTok) or profiles (profile = true: logP, rows of nOutTok + 1 log
// weights, outOff counting rows) or CTC-merged profiles (nCols > 0: rows of nCols + 1 log weights, nCols + 1 planes per slot,
// mb_prefix_merge.hip); everything else -- R, the pool, the free list -- is the same.
static mb_prefix *prefix_create(mb_machine *m, int64_t nSeq, bool profile, const int32_t *outTok, const double *logP, const int64_t *outOff,
                                const double *logSumInTrans, int64_t maxNodes, int32_t nCols = 0, const int32_t *colTok = nullptr) {
  if (!m || nSeq < 1 || !outOff || !logSumInTrans || maxNodes < 1) { set_error("null argument"); return nullptr; }
  if (ensure_init()) return nullptr;
  if (m->S > PREFIX_MAX_STATES) { set_error("prefix search: more than " + std::to_string(PREFIX_MAX_STATES) + " states"); return nullptr; }
  mb_prefix *p = new mb_prefix();
  p->m = m; p->nSeq = nSeq; p->maxNodes = maxNodes;
  p->outOff.resize(nSeq + 1);
  for (int64_t k = 0; k <= nSeq; ++k) p->outOff[k] = outOff[k] - outOff[0];
  for (int64_t k = 0; k < nSeq; ++k) {
    const long long len = p->outOff[k + 1] - p->outOff[k];
    if (len < 0 || len > 0x3fffffff) { set_error("bad output offsets"); delete p; return nullptr; }
    p->maxOutLen = std::max(p->maxOutLen, len);
  }
  const long long nTok = profile ? 0 : p->outOff[nSeq];
  const int32_t *tok = outTok ? outTok + outOff[0] : nullptr;
  if (nTok && !tok) { set_error("null argument"); delete p; return nullptr; }
  for (long long k = 0; k < nTok; ++k)
    if (tok[k] < 1 || tok[k] > m->nOut) { set_error("output token " + std::to_string(tok[k]) + " outside the alphabet"); delete p; return nullptr; }
  const long long width = nCols ? nCols + 1 : m->nOut + 1;      // doubles of a profile row
  const long long nVal = profile ? p->outOff[nSeq] * width : 0;
  const double *val = logP ? logP + outOff[0] * width : nullptr;
  if (nVal && !val) { set_error("null argument"); delete p; return nullptr; }
  if (!profile_values_ok(val, nVal)) { delete p; return nullptr; }
  p->profile = profile;
  p->nCols = nCols;
  // R by column, -inf entries dropped; NaN or +inf is a caller's error
  const int S = m->S;
  std::vector<long long> rOff(S + 1, 0);
  std::vector<int> rIdx; std::vector<double> rVal;
  for (int s = 0; s < S; ++s) {
    for (int q = 0; q < S; ++q) {
      const double v = logSumInTrans[(size_t)q * S + s];
      if (std::isnan(v) || v == INFINITY) { set_error("logSumInTrans holds NaN or +infinity"); delete p; return nullptr; }
      if (v > -INFINITY) { rIdx.push_back(q); rVal.push_back(v); }
    }
    rOff[s + 1] = (long long)rIdx.size();
  }
  p->slotDoubles = nCols ? merged_prefix_slot_doubles(S, nCols, p->maxOutLen) : prefix_slot_doubles(S, p->maxOutLen);
  if (nCols && !merged_prefix_lds_fits(S, nCols)) {
    set_error("prefix search against merged profiles: ((6 nCols + 5) x states + nCols + 1) doubles exceed the LDS of a workgroup (160 KiB; " +
              std::to_string(S) + " states, " + std::to_string(nCols) + " columns)");
    delete p; return nullptr;
  }
  const double poolBytes = (double)maxNodes * (double)p->slotDoubles * 8.0;
  const double rBytes = 12.0 * (double)rIdx.size() + 8.0 * (S + 1) + 4.0 * (double)nTok + 8.0 * (double)nVal;   // R by column and the tokens (profile rows) count too
  if (poolBytes + rBytes > (double)budget_bytes()) {
    set_error("prefix search: " + std::to_string(maxNodes) + " node lattices of " + std::to_string(p->slotDoubles * 8) + " bytes and " +
              std::to_string((long long)rBytes) + " bytes of tables exceed the device memory budget (" + std::to_string(budget_bytes()) +
              " bytes): ask for fewer nodes (--decode-nodes)");
    delete p; return nullptr;
  }
  bool ok = hip_ok(sm_alloc((void **)&p->d_out, (size_t)std::max<long long>(nTok, 1) * sizeof(int)), "hipMalloc(prefix tokens)") &&
            hip_ok(sm_alloc((void **)&p->d_rOff, rOff.size() * sizeof(long long)), "hipMalloc(prefix R)") &&
            hip_ok(sm_alloc((void **)&p->d_rIdx, std::max<size_t>(rIdx.size(), 1) * sizeof(int)), "hipMalloc(prefix R)") &&
            hip_ok(sm_alloc((void **)&p->d_rVal, std::max<size_t>(rVal.size(), 1) * sizeof(double)), "hipMalloc(prefix R)");
  ok = ok && (!profile || hip_ok(sm_alloc((void **)&p->d_logP, (size_t)std::max<long long>(nVal, 1) * sizeof(double)), "hipMalloc(prefix profiles)"));
  ok = ok && (!nCols || (hip_ok(sm_alloc((void **)&p->d_colTok, (size_t)nCols * sizeof(int)), "hipMalloc(prefix columns)") &&
                         hip_ok(hipMemcpy(p->d_colTok, colTok, (size_t)nCols * sizeof(int), hipMemcpyHostToDevice), "H2D prefix columns")));
  ok = ok && (!nVal || (!h2d_large(p->d_logP, val, (size_t)nVal * sizeof(double)) && hip_ok(hipStreamSynchronize(g_stream), "H2D prefix profiles")));
  ok = ok && (!nTok || hip_ok(hipMemcpy(p->d_out, tok, (size_t)nTok * sizeof(int), hipMemcpyHostToDevice), "H2D prefix tokens")) &&
       hip_ok(hipMemcpy(p->d_rOff, rOff.data(), rOff.size() * sizeof(long long), hipMemcpyHostToDevice), "H2D prefix R") &&
       (rIdx.empty() || (hip_ok(hipMemcpy(p->d_rIdx, rIdx.data(), rIdx.size() * sizeof(int), hipMemcpyHostToDevice), "H2D prefix R") &&
                         hip_ok(hipMemcpy(p->d_rVal, rVal.data(), rVal.size() * sizeof(double), hipMemcpyHostToDevice), "H2D prefix R")));
  if (ok) {
    // the node pool: the library's cached workspace when no other live search holds it (steady create / destroy cycles allocate
    // nothing), else an allocation of this object
    Workspace &w = g_ws[WS_PREFIX_POOL];
    if (!w.held) {
      p->pool = (double *)ws_get(WS_PREFIX_POOL, (size_t)poolBytes);
      if (p->pool) { w.held = true; p->poolIsWorkspace = true; }
      ok = p->pool != nullptr;
    } else {
      ok = hip_ok(hipMalloc((void **)&p->pool, std::max<size_t>((size_t)poolBytes, 256)), "hipMalloc(prefix node pool)");
      if (ok) { ++g_alloc.allocs; g_alloc.bytes += (size_t)poolBytes; } else p->pool = nullptr;
    }
  }
  if (!ok) { prefix_free(p); return nullptr; }
  p->slotSeq.assign((size_t)maxNodes, -1);
  p->freeSlots.resize((size_t)maxNodes);
  for (int64_t k = 0; k < maxNodes; ++k) p->freeSlots[(size_t)k] = maxNodes - 1 - k;   // slot 0 goes out first
  return p;
}

mb_prefix *mb_prefix_create(mb_machine *m, int64_t nSeq, const int32_t *outTok, const int64_t *outOff, const double *logSumInTrans,
                            int64_t maxNodes) {
  ApiGuard guard;
  return prefix_create(m, nSeq, false, outTok, nullptr, outOff, logSumInTrans, maxNodes);
}

mb_prefix *mb_prefix_create_profiles(mb_machine *m, int64_t nProfiles, const double *logP, const int64_t *rowOff, const double *logSumInTrans,
                                     int64_t maxNodes) {
  ApiGuard guard;
  return prefix_create(m, nProfiles, true, nullptr, logP, rowOff, logSumInTrans, maxNodes);
}

mb_prefix *mb_prefix_create_merged(mb_machine *m, int64_t nProfiles, const double *logP, const int64_t *rowOff, int32_t nCols,
                                   const int32_t *colTok, const double *logSumInTrans, int64_t maxNodes) {
  ApiGuard guard;
  if (!merge_map_ok(m, nCols, colTok)) return nullptr;
  return prefix_create(m, nProfiles, true, nullptr, logP, rowOff, logSumInTrans, maxNodes, nCols, colTok);
}

void mb_prefix_destroy(mb_prefix *p) {
  if (!p) return;
  ApiGuard guard;
  quiesce_streams();
  prefix_free(p);
}

// One launch for n fills.  parent[i] < 0: entry i is the root of search seq[i] (inTok ignored).
static int prefix_fill(mb_prefix *p, int64_t n, const int64_t *seq, const int64_t *parent, const int32_t *inTok, int64_t *childOut,
                       double *logSeqProb, double *logPrefixProb) {
  if (n == 0) return 0;
  if (n > 0x7fffffff) { set_error("too many fills in one call"); return 1; }
  const mb_machine *m = p->m;
  for (int64_t i = 0; i < n; ++i) {
    if (seq[i] < 0 || seq[i] >= p->nSeq) { set_error("prefix fill " + std::to_string(i) + ": no such search"); return 1; }
    if (parent[i] >= 0) {
      if (parent[i] >= p->maxNodes || p->slotSeq[(size_t)parent[i]] != seq[i]) { set_error("prefix fill " + std::to_string(i) + ": parent is not a live node of that search"); return 1; }
      if (inTok[i] < 1 || inTok[i] > m->nIn) { set_error("prefix fill " + std::to_string(i) + ": input token outside the alphabet"); return 1; }
    }
  }
  if ((int64_t)p->freeSlots.size() < n) {
    set_error("prefix node pool is full (" + std::to_string(p->maxNodes) + " nodes, " + std::to_string(p->freeSlots.size()) + " free, " + std::to_string(n) + " wanted)");
    return 1;
  }
  std::vector<PrefixDesc> h((size_t)n);
  for (int64_t i = 0; i < n; ++i) {
    const long long slot = p->freeSlots[p->freeSlots.size() - 1 - (size_t)i];
    childOut[i] = slot;
    PrefixDesc &d = h[(size_t)i];
    d.parentBase = parent[i] >= 0 ? parent[i] * p->slotDoubles : -1;
    d.childBase = slot * p->slotDoubles;
    d.outBase = p->outOff[(size_t)seq[i]];
    d.outLen = (int)(p->outOff[(size_t)seq[i] + 1] - p->outOff[(size_t)seq[i]]);
    d.inTok = parent[i] >= 0 ? inTok[i] : 0;
  }
  SmBuf<PrefixDesc> d_desc; SmBuf<double> d_res;
  MB_HIP(d_desc.alloc((long long)h.size()));
  if (!hip_ok(d_res.alloc(n * 2), "hipMalloc(prefix results)")) return 1;
  std::vector<double> res((size_t)n * 2);
  int rc = hip_ok(hipMemcpyAsync(d_desc, h.data(), h.size() * sizeof(PrefixDesc), hipMemcpyHostToDevice, g_stream), "H2D prefix descriptors") ? 0 : 1;
  if (!rc) {
    Timer tm;
    tm.start();
    const PrefixR R{p->d_rOff, p->d_rIdx, p->d_rVal};
    rc = p->nCols    ? launch_prefix_fill_merged(m, R, p->nCols, p->d_colTok, d_desc, (int)n, p->d_logP, p->pool, d_res, g_stream)
         : p->profile ? launch_prefix_fill_profile(m, R, d_desc, (int)n, p->d_logP, p->pool, d_res, g_stream)
                      : launch_prefix_fill(m, R, d_desc, (int)n, p->d_out, p->pool, d_res, g_stream);
    g_last_ms += tm.stop();
    g_last_launches = 1;
  }
  if (!rc && !hip_ok(hipMemcpyAsync(res.data(), d_res, res.size() * sizeof(double), hipMemcpyDeviceToHost, g_stream), "D2H prefix results")) rc = 1;
  const char *kernel = p->nCols ? "k_prefix_fill_merged" : p->profile ? "k_prefix_fill_profile" : "k_prefix_fill";
  if (!rc && !hip_ok(hipStreamSynchronize(g_stream), kernel)) rc = 1;
  g_last_kernel = kernel;
  if (rc) { quiesce_streams(); return rc; }      // (before the descriptors go)
  for (int64_t i = 0; i < n; ++i) {
    p->slotSeq[(size_t)childOut[i]] = seq[i];
    logSeqProb[i] = res[2 * (size_t)i]; logPrefixProb[i] = res[2 * (size_t)i + 1];
  }
  p->freeSlots.resize(p->freeSlots.size() - (size_t)n);
  return 0;
}

int mb_prefix_root(mb_prefix *p, int64_t seq, int64_t *nodeOut, double *logSeqProb, double *logPrefixProb) {
  ApiGuard guard;
  if (!p || !nodeOut || !logSeqProb || !logPrefixProb) { set_error("null argument"); return 1; }
  reset_last();
  const int64_t none = -1;
  return prefix_fill(p, 1, &seq, &none, nullptr, nodeOut, logSeqProb, logPrefixProb);
}

int mb_prefix_extend(mb_prefix *p, int64_t n, const int64_t *seq, const int64_t *parent, const int32_t *inTok, int64_t *childOut,
                     double *logSeqProb, double *logPrefixProb) {
  ApiGuard guard;
  if (!p || n < 0 || (n && (!seq || !parent || !inTok || !childOut || !logSeqProb || !logPrefixProb))) { set_error("null argument"); return 1; }
  reset_last();
  for (int64_t i = 0; i < n; ++i)
    if (parent[i] < 0) { set_error("prefix fill " + std::to_string(i) + ": parent is not a live node of that search"); return 1; }
  return prefix_fill(p, n, seq, parent, inTok, childOut, logSeqProb, logPrefixProb);
}

int mb_prefix_release(mb_prefix *p, int64_t n, const int64_t *node) {
  ApiGuard guard;
  if (!p || n < 0 || (n && !node)) { set_error("null argument"); return 1; }
  for (int64_t i = 0; i < n; ++i) {
    if (node[i] < 0 || node[i] >= p->maxNodes || p->slotSeq[(size_t)node[i]] < 0) { set_error("prefix release: node " + std::to_string(node[i]) + " is not live"); return 1; }
    for (int64_t k = 0; k < i; ++k) if (node[k] == node[i]) { set_error("prefix release: node " + std::to_string(node[i]) + " is listed twice"); return 1; }
  }
  for (int64_t i = 0; i < n; ++i) { p->slotSeq[(size_t)node[i]] = -1; p->freeSlots.push_back(node[i]); }
  return 0;
}

int64_t mb_prefix_free_nodes(const mb_prefix *p) { return p ? (int64_t)p->freeSlots.size() : 0; }

int mb_prefix_node_cells(mb_prefix *p, int64_t node, double *cellsOut) {
  ApiGuard guard;
  if (!p || !cellsOut) { set_error("null argument"); return 1; }
  if (node < 0 || node >= p->maxNodes || p->slotSeq[(size_t)node] < 0) { set_error("prefix node " + std::to_string(node) + " is not live"); return 1; }
  const long long k = p->slotSeq[(size_t)node];
  const long long cells = prefix_slot_doubles(p->m->S, p->outOff[(size_t)k + 1] - p->outOff[(size_t)k]) * (p->nCols ? p->nCols + 1 : 1);
  return d2h_large(cellsOut, p->pool + node * p->slotDoubles, (size_t)cells * sizeof(double));
}

}  // extern "C"
