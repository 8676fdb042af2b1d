// mb_profile_api.hip -- the C-ABI of the profile tapes (include/mbhip.h, docs/profile_tapes.md): one-tape profiles (mb_profiles, plain
// and CTC-merged), sequence-against-profile pairs (mb_profile_pairs, plain, merged and under envelopes) and two-profile pairs
// (mb_profile_twos, plain, merged and under envelopes).
//
// Host orchestration only, like mb_api.hip.  Each family has Forward, Viterbi, counts, row posteriors, set_rows and a single-lattice
// fill; what those calls share with the token batch calls -- the chunk loop, the call-scoped device buffers, the count tail -- is in
// mb_api_internal.h, what they share among themselves -- the chunk planner, the path copier, the posterior tail -- is written once at
// the top, the per-family parts (descriptors, launches, kernel names) follow.
#include <algorithm>
#include <cmath>
#include <cstring>
#include <functional>
#include <string>
#include <vector>

#include "mb_api_internal.h"
#include "mb_profile.h"
#include "mb_profile_merge.h"
#include "mb_profile_pair.h"
#include "mb_profile_pair_env.h"
#include "mb_profile_pair_merge.h"
#include "mb_profile_post.h"
#include "mb_profile_two.h"
#include "mb_profile_two_env.h"
#include "mb_profile_two_merge.h"

namespace mb {

bool profile_values_ok(const double *v, long long n) {
  for (long long k = 0; k < n; ++k)
    if (std::isnan(v[k]) || v[k] == INFINITY) { set_error("profile weight " + std::to_string(k) + " is NaN or +infinity (log weights: -inf allowed)"); return false; }
  return true;
}

bool merge_map_ok(const mb_machine *m, int32_t nCols, const int32_t *colTok) {
  if (!m) { set_error("null argument"); return false; }
  if (nCols < 1 || nCols > 0xffff) { set_error("merged profiles need 1..65535 columns"); return false; }
  if (!colTok) { set_error("null argument"); return false; }
  for (int c = 0; c < nCols; ++c)
    if (colTok[c] < 1 || colTok[c] > m->nOut) { set_error("column " + std::to_string(c + 1) + ": token " + std::to_string(colTok[c]) + " is outside 1..nOutTok"); return false; }
  return true;
}

// ---- what the three families share ---------------------------------------------------------------------------------------------
// Split n items (noun: "profile" or "pair", for the error) into chunks whose device memory (bytesPer(item k)) fits the budget;
// even-sized like plan_chunks.
static bool lattice_chunks(long long n, const char *noun, const std::function<double(long long)> &bytesPer, std::vector<Chunk> &out) {
  const double budget = (double)budget_bytes();
  double total = 0.0;
  for (long long k = 0; k < n; ++k) {
    const double b = bytesPer(k);
    if (b > budget) { set_error("one " + std::string(noun) + "'s DP lattice (" + std::to_string((long long)b) + " bytes) exceeds the device memory budget"); return false; }
    total += b;
  }
  const double nChunks = std::max(1.0, std::ceil(total / budget));
  const double share = std::min(budget, total / nChunks * 1.05);
  long long p0 = 0;
  double acc = 0.0;
  for (long long k = 0; k < n; ++k) {
    const double b = bytesPer(k);
    if (k > p0 && (acc + b > budget || (acc >= share && acc + b > share) || k - p0 >= (1 << 30))) { out.push_back({p0, k, 0}); p0 = k; acc = 0.0; }
    acc += b;
  }
  if (n > p0) out.push_back({p0, n, 0});
  return true;
}

// Where the per-pair device results of mb_profile_pairs landed (PairProfPlan::slot, below): each chunk in the order of its plan's
// slots, at[k] = the entry of pair k.
struct PairWhere { std::vector<long long> at; bool permuted = false; };

// per-item log-likelihoods of a pair batch into dst[0..n): permuted when the batch has envelopes
static int fetch_loglike(double *dst, const double *d_ll, long long n, const PairWhere *where) {
  if (n <= 0 || !where->permuted) return fetch_loglike(dst, d_ll, n);
  std::vector<double> tmp((size_t)n);
  if (fetch_loglike(tmp.data(), d_ll, n)) return 1;
  for (long long k = 0; k < n; ++k) dst[k] = tmp[(size_t)where->at[(size_t)k]];
  return 0;
}

// The caller's path arrays of a Viterbi call and the host staging of one chunk.  noun: "profile" or "pair", for the traceback's
// errors; bound(k): the traceback slots of item k, which is how far apart the chunk's paths lie on the device.
struct PathSink {
  int64_t *off; uint32_t *edges; int32_t *row, *inRow;
  long long cap;
  const char *noun;
  std::function<long long(long long)> bound;
  long long written = 0;
  std::vector<long long> len;
  std::vector<uint32_t> he;
  std::vector<int32_t> hr, hi;
};

// The paths of chunk items [k0, k0 + np) from the device (paths: the chunk's traceback slots; slot: where each item's length landed,
// nullptr = in order; d_i: the third array of the two-profile pairs) to the caller's arrays, packed.  A path that does not fit under
// the caller's cap ends the call with the earlier items' paths and offsets written.
static int unpack_paths(PathSink &o, long long k0, long long np, long long paths, const std::vector<long long> *slot, const long long *d_len,
                        const uint32_t *d_e, const int32_t *d_r, const int32_t *d_i = nullptr) {
  o.len.resize((size_t)np); o.he.resize((size_t)std::max<long long>(paths, 1)); o.hr.resize(o.he.size()); o.hi.resize(d_i ? o.he.size() : 0);
  if (!hip_ok(hipMemcpy(o.len.data(), d_len, np * sizeof(long long), hipMemcpyDeviceToHost), "D2H path lengths")) return 1;
  if (paths && (d2h_large(o.he.data(), d_e, paths * sizeof(uint32_t)) || (o.row && d2h_large(o.hr.data(), d_r, paths * sizeof(int32_t))) ||
                (o.inRow && d2h_large(o.hi.data(), d_i, paths * sizeof(int32_t))))) return 1;
  long long base = 0;
  for (long long k = 0; k < np; ++k) {
    long long n = o.len[(size_t)(slot ? (*slot)[(size_t)k] : k)];
    if (n == -1) n = 0;   // no finite path: an empty one (the reference refuses to trace it)
    else if (n < 0) { set_error(std::string(o.noun) + (n == -2 ? " traceback overflowed its bound" : " traceback found no matching candidate")); return 1; }
    if (o.written + n > o.cap) { set_error("pathCap too small for the Viterbi paths"); return 1; }
    std::memcpy(o.edges + o.written, o.he.data() + base, (size_t)n * sizeof(uint32_t));
    if (o.row) std::memcpy(o.row + o.written, o.hr.data() + base, (size_t)n * sizeof(int32_t));
    if (o.inRow) std::memcpy(o.inRow + o.written, o.hi.data() + base, (size_t)n * sizeof(int32_t));
    o.written += n;
    o.off[k0 + k + 1] = o.written;
    base += o.bound(k0 + k);
  }
  return 0;
}

// The caller's arrays of a sample call (nS samples per item) and the host staging of one chunk; inRow: the third array of the
// two-profile pairs.
struct SampleSink {
  int64_t *off; uint32_t *edges; int32_t *row, *inRow; double *logProb;
  long long nS;
  std::function<long long(long long)> bound;
  long long written = 0;
  std::vector<long long> len;
  std::vector<double> lq;
  std::vector<uint32_t> he;
  std::vector<int32_t> hr, hi;
};

// The sampled paths of chunk items [k0, k0 + np) from the device to the caller's arrays, packed: path (k0 + k) * nS + j is sample j
// of item k.  Lengths and log probabilities lie where the item's lanes were (slot: in which place of the chunk each item ran,
// nullptr = in order); the path slots (entries: all of the chunk's) are packed in item order, bound(k) entries per sample.
static int unpack_samples(SampleSink &o, long long k0, long long np, long long entries, const std::vector<long long> *slot, const long long *d_len, const double *d_lq,
                          const uint32_t *d_e, const int32_t *d_r, const int32_t *d_i = nullptr) {
  const long long lanes = np * o.nS;
  o.len.resize((size_t)std::max<long long>(lanes, 1)); o.lq.resize(o.len.size());
  o.he.resize((size_t)std::max<long long>(entries, 1)); o.hr.resize(o.row ? o.he.size() : 0); o.hi.resize(o.inRow ? o.he.size() : 0);
  if (lanes && (d2h_large(o.len.data(), d_len, (size_t)lanes * sizeof(long long)) || d2h_large(o.lq.data(), d_lq, (size_t)lanes * sizeof(double)))) return 1;
  if (!lanes && !hip_ok(hipStreamSynchronize(g_stream), "sample launch")) return 1;
  if (entries && (d2h_large(o.he.data(), d_e, (size_t)entries * sizeof(uint32_t)) || (o.row && d2h_large(o.hr.data(), d_r, (size_t)entries * sizeof(int32_t))) ||
                  (o.inRow && d2h_large(o.hi.data(), d_i, (size_t)entries * sizeof(int32_t))))) return 1;
  long long base = 0;
  for (long long k = 0; k < np; ++k) {
    const long long bound = o.bound(k0 + k), at = (slot ? (*slot)[(size_t)k] : k) * o.nS;
    for (long long j = 0; j < o.nS; ++j, base += bound) {
      long long n = o.len[(size_t)(at + j)];
      if (n == -1) n = 0;      // a dead pair: empty paths, logq = -inf
      else if (n < 0) { set_error(n == -2 ? "pair sample overflowed its bound" : "pair sample found no candidate with a positive probability"); return 1; }
      std::memcpy(o.edges + o.written, o.he.data() + base, (size_t)n * sizeof(uint32_t));
      if (o.row) std::memcpy(o.row + o.written, o.hr.data() + base, (size_t)n * sizeof(int32_t));
      if (o.inRow) std::memcpy(o.inRow + o.written, o.hi.data() + base, (size_t)n * sizeof(int32_t));
      o.written += n;
      o.off[(k0 + k) * o.nS + j + 1] = o.written;
      if (o.logProb) o.logProb[(k0 + k) * o.nS + j] = o.lq[(size_t)(at + j)];
    }
  }
  return 0;
}

// the workgroups per item of the count kernels of the pairs and the two-profile pairs: one per 2 048 cells of the largest lattice, 256 at the most
template <class Cells> static int count_groups(long long p0, long long p1, Cells cells) {
  long long maxCells = 0;
  for (long long k = p0; k < p1; ++k) maxCells = std::max<long long>(maxCells, cells(k));
  return (int)std::min<long long>(256, std::max<long long>(1, (maxCells + 2047) / 2048));
}

// the LDS table of the row-posterior kernels in doubles; MB_ROWPOST_TABLE makes it smaller (the rows-per-block and wide-row paths at small shapes)
static int rowpost_table() { return std::max(1, std::min(opt_int<MB_ROWPOST_TABLE>(ROWPOST_LDS_MAX), ROWPOST_LDS_MAX)); }
// the line blocks of the item of [p0, p1) that has most, 1 024 at the most (a group past an item's last block has nothing to do);
// lines(k): the rows of item k on the axis, blockRows(k): how many of them one block takes
template <class Lines, class BlockRows> static long long rowpost_groups(long long p0, long long p1, Lines lines, BlockRows blockRows) {
  long long groups = 1;
  for (long long k = p0; k < p1; ++k) {
    const long long L = lines(k), R = blockRows(k);
    groups = std::max(groups, (L + R - 1) / R);
  }
  return std::min<long long>(groups, 1024);
}
// the bins of a row-posterior call to the host (fixed point under MB_DETERMINISTIC: 2^-36, a posterior is at most 1, far inside the range)
static int fetch_posteriors(double *post, const double *d_post, long long nv) {
  if (nv && d2h_large(post, d_post, (size_t)nv * sizeof(double))) return 1;
  return g_deterministic ? decode_fixed_point(post, nv, "MB_DETERMINISTIC: a row posterior left the fixed-point range") : 0;
}

// One materialised lattice to the host (the mb_*_fill calls): `cells` doubles of slot 0, `ring` doubles of scratch in slot 1 (0: none),
// launch(pool, scratch, d_ll) as the call's one launch, the lattice into out.
template <class Launch> static int fill_one(long long cells, long long ring, double *out, Launch launch) {
  SmBuf<double> d_ll;
  if (!hip_ok(d_ll.alloc(1), "hipMalloc(loglike)")) return 1;
  double *pool = (double *)ws_get(0, (size_t)cells * sizeof(double));
  double *scratch = pool && ring ? (double *)ws_get(1, (size_t)ring * sizeof(double)) : nullptr;
  int rc = !pool || (ring && !scratch);
  if (!rc) {
    Timer tm;
    Timed t(tm, 1);
    rc = launch(pool, scratch, d_ll.p);
  }
  if (!rc) rc = d2h_large(out, pool, (size_t)cells * sizeof(double));
  if (rc) quiesce_streams();
  return rc;
}
static bool fill_mode_ok(int mode) {
  if (mode == MB_FORWARD || mode == MB_VITERBI || mode == MB_BACKWARD) return true;
  set_error("unknown fill mode");
  return false;
}

// ---- one-tape profiles (mb_profile.hip, mb_profile_merge.hip) ---------------------------------------------------------------------
// Plain and CTC-merged profiles (p->nCols > 0, mb_profile_merge.hip) share the entry points below: the merged lattice has nCols + 1
// planes of the plain one, its own kernels and its own rolling state.
static long long pf_rows(const mb_profiles *p, long long k) { return p->rowOff[k + 1] - p->rowOff[k]; }
static long long pf_planes(const mb_profiles *p) { return p->nCols ? p->nCols + 1 : 1; }
static long long pf_width(const mb_profiles *p) { return p->nCols ? p->nCols + 1 : p->m->nOut + 1; }   // doubles of a row
static long long pf_cells(const mb_profiles *p, long long nRows) { return profile_cells(p->m->S, nRows) * pf_planes(p); }
static long long pf_path_bound(const mb_profiles *p, long long k) { return profile_path_bound(p->m->nLevF, pf_rows(p, k)); }
static MergeMap pf_map(const mb_profiles *p) { return MergeMap{p->nCols, p->d_colTok}; }
// doubles of global scratch a workgroup of the Forward / Viterbi (mat: materialised) or of the rolling Backward sweep needs (0: LDS)
static long long pf_fwd_scratch(const mb_profiles *p, bool mat) {
  const int S = p->m->S;
  if (!p->nCols) return mat || profile_lds_bytes(S) ? 0 : 3LL * S;
  return profile_merge_fwd_lds(S, p->nCols, mat) ? 0 : profile_merge_ring(S, p->nCols);
}
static long long pf_bwd_scratch(const mb_profiles *p) {
  const int S = p->m->S;
  if (!p->nCols) return profile_lds_bytes(S) ? 0 : 3LL * S;
  return profile_merge_bwd_lds(S, p->nCols) ? 0 : profile_merge_ring(S, p->nCols);
}
static int pf_fwd(const mb_profiles *p, int mode, bool mat, const ProfDesc *d, int n, double *pool, double *scratch, double *loglike) {
  return p->nCols ? launch_profile_merge_fwd(p->m, pf_map(p), mode, mat, d, n, p->d_logP, pool, scratch, loglike, g_stream)
                  : launch_profile_fwd(p->m, mode, mat, d, n, p->d_logP, pool, scratch, loglike, g_stream);
}
static int pf_bwd(const mb_profiles *p, bool mat, const ProfDesc *d, int n, double *pool, const double *fwdPool, double *scratch,
                  double *loglike, double *part, long long nTrans) {
  return p->nCols ? launch_profile_merge_bwd(p->m, pf_map(p), mat, d, n, p->d_logP, pool, fwdPool, scratch, loglike, part, nTrans, g_stream)
                  : launch_profile_bwd(p->m, mat, d, n, p->d_logP, pool, fwdPool, scratch, loglike, part, nTrans, g_stream);
}
static int pf_traceback(const mb_profiles *p, const ProfDesc *d, int n, const double *pool, uint32_t *edges, int32_t *rows, long long *len) {
  return p->nCols ? launch_profile_merge_traceback(p->m, pf_map(p), d, n, p->d_logP, pool, edges, rows, len, g_stream)
                  : launch_profile_traceback(p->m, d, n, p->d_logP, pool, edges, rows, len, g_stream);
}
static const char *pf_name(const mb_profiles *p, const char *plain, const char *merged) { return p->nCols ? merged : plain; }
static const char *pf_fwd_name(const mb_profiles *p, int mode, bool mat) {
  return mode == MB_VITERBI ? (mat ? pf_name(p, "k_profile_fwd<max,mat>", "k_profile_merge_fwd<max,mat>") : pf_name(p, "k_profile_fwd<max,rolling>", "k_profile_merge_fwd<max,rolling>"))
                            : (mat ? pf_name(p, "k_profile_fwd<sum,mat>", "k_profile_merge_fwd<sum,mat>") : pf_name(p, "k_profile_fwd<sum,rolling>", "k_profile_merge_fwd<sum,rolling>"));
}

// descriptors of profiles [p0, p1): lattices and traceback slots packed from 0, with the pool doubles and path entries they take
struct ProfPlan { SmBuf<ProfDesc> d; long long cells = 0, paths = 0; };
static int profile_descs(const mb_profiles *p, long long p0, long long p1, ProfPlan &pl) {
  std::vector<ProfDesc> h((size_t)(p1 - p0));
  for (long long k = p0; k < p1; ++k) {
    ProfDesc &d = h[(size_t)(k - p0)];
    d.rowBase = p->rowOff[k]; d.nRows = (int)pf_rows(p, k); d.cellBase = pl.cells; d.pathBase = pl.paths; d.pad = 0;
    pl.cells += pf_cells(p, d.nRows);
    pl.paths += pf_path_bound(p, k);
  }
  MB_HIP(pl.d.alloc((long long)h.size()));
  if (!h.empty() && (!hip_ok(hipMemcpyAsync(pl.d, h.data(), h.size() * sizeof(ProfDesc), hipMemcpyHostToDevice, g_stream), "H2D profile descriptors") ||
                     !hip_ok(hipStreamSynchronize(g_stream), "H2D profile descriptors"))) return 1;
  return 0;
}
static auto pf_build(const mb_profiles *p) { return [p](const Chunk &c, ProfPlan &pl) { return profile_descs(p, c.p0, c.p1, pl); }; }

static int profile_scratch(long long perGroup, long long n, double **scratch) {
  *scratch = nullptr;
  if (!perGroup || n == 0) return 0;
  *scratch = (double *)ws_get(1, (size_t)n * perGroup * sizeof(double));
  return *scratch ? 0 : 1;
}

// Forward (MB_FORWARD) or Viterbi scores without paths (MB_VITERBI); mat: through the materialised lattice
static int profiles_scores(mb_profiles *p, int mode, bool mat, double *loglike) {
  const long long fScratch = pf_fwd_scratch(p, mat);
  const double rollBytes = 8.0 * fScratch;
  std::vector<Chunk> chunks;
  if (!lattice_chunks(p->n, "profile", [&](long long k) { return (mat ? 8.0 * pf_cells(p, pf_rows(p, k)) : 0.0) + rollBytes; }, chunks)) return 1;
  SmBuf<double> d_ll;
  MB_HIP(d_ll.alloc(p->n));
  int rc = for_chunks<ProfPlan>(chunks, pf_build(p), [&](const Chunk &c, ProfPlan &pl, Timer &tm) {
    const long long np = c.p1 - c.p0;
    double *pool = nullptr, *scratch = nullptr;
    if (mat && !(pool = ws_array<double>(0, pl.cells))) return 1;
    if (profile_scratch(fScratch, np, &scratch)) return 1;
    Timed t(tm, 1);
    return pf_fwd(p, mode, mat, pl.d, (int)np, pool, scratch, d_ll + c.p0);
  });
  if (!rc) rc = fetch_loglike(loglike, d_ll, p->n);
  g_last_kernel = pf_fwd_name(p, mode, mat);
  return rc;
}

// nCols = 0: plain profiles, rows of nOutTok + 1 doubles; nCols > 0: merged, rows of nCols + 1 doubles and the column map colTok
static mb_profiles *profiles_create(mb_machine *m, int64_t nProfiles, const double *logP, const int64_t *rowOff, int nCols, const int32_t *colTok) {
  if (!m || nProfiles < 0 || (nProfiles > 0 && !rowOff)) { set_error("null argument"); return nullptr; }
  if (ensure_init()) return nullptr;
  mb_profiles *p = new mb_profiles();
  p->m = m; p->n = nProfiles; p->nCols = nCols;
  p->rowOff.assign((size_t)nProfiles + 1, 0);
  for (long long k = 0; k < nProfiles; ++k) {
    const long long len = rowOff[k + 1] - rowOff[k];
    if (len < 0 || len > 0x3fffffff) { set_error("bad profile row offsets"); delete p; return nullptr; }
    p->rowOff[(size_t)k + 1] = p->rowOff[(size_t)k] + len;
  }
  p->totalRows = p->rowOff.back();
  const long long C = nCols ? nCols + 1 : m->nOut + 1, nv = p->totalRows * C;
  const double *v0 = logP ? logP + (nProfiles ? rowOff[0] * C : 0) : nullptr;
  if (nv && !v0) { set_error("null argument"); delete p; return nullptr; }
  if (!profile_values_ok(v0, nv)) { delete p; return nullptr; }
  if (!hip_ok(hipMalloc((void **)&p->d_logP, (size_t)std::max<long long>(nv, 1) * sizeof(double)), "hipMalloc(profiles)")) { delete p; return nullptr; }
  if (nCols && (!hip_ok(hipMalloc((void **)&p->d_colTok, (size_t)nCols * sizeof(int)), "hipMalloc(profile columns)") ||
                !hip_ok(hipMemcpyAsync(p->d_colTok, colTok, (size_t)nCols * sizeof(int), hipMemcpyHostToDevice, g_stream), "H2D profile columns"))) { mb_profiles_destroy(p); return nullptr; }
  if (nv && h2d_large(p->d_logP, v0, (size_t)nv * sizeof(double))) { mb_profiles_destroy(p); return nullptr; }
  if (!hip_ok(hipStreamSynchronize(g_stream), "H2D profiles")) { mb_profiles_destroy(p); return nullptr; }
  return p;
}

static int profile_fill(mb_machine *m, int mode, const double *logP, int64_t nRows, int nCols, const int32_t *colTok, double *cellsOut) {
  if (!m || !cellsOut || nRows < 0 || (nRows && !logP)) { set_error("null argument"); return 1; }
  if (!fill_mode_ok(mode)) return 1;
  if (ensure_init()) return 1;
  g_last_ms = 0.0; g_last_launches = 0;
  const int64_t off[2] = {0, nRows};
  mb_profiles *p = profiles_create(m, 1, logP, off, nCols, colTok);
  if (!p) return 1;
  int rc;
  {
    ProfPlan pl;
    rc = profile_descs(p, 0, 1, pl);
    if (!rc) rc = fill_one(pl.cells, mode == MB_BACKWARD ? 0 : pf_fwd_scratch(p, true), cellsOut, [&](double *pool, double *scratch, double *d_ll) {
      return mode == MB_BACKWARD ? pf_bwd(p, true, pl.d, 1, pool, nullptr, nullptr, d_ll, nullptr, 0) : pf_fwd(p, mode, true, pl.d, 1, pool, scratch, d_ll);
    });
  }
  g_last_kernel = mode == MB_BACKWARD ? pf_name(p, "k_profile_bwd<mat>", "k_profile_merge_bwd<mat>") : pf_fwd_name(p, mode, true);
  mb_profiles_destroy(p);
  return rc;
}

}  // namespace mb

using namespace mb;

extern "C" {

mb_profiles *mb_profiles_create(mb_machine *m, int64_t nProfiles, const double *logP, const int64_t *rowOff) {
  ApiGuard guard;
  return profiles_create(m, nProfiles, logP, rowOff, 0, nullptr);
}

mb_profiles *mb_profiles_create_merged(mb_machine *m, int64_t nProfiles, const double *logP, const int64_t *rowOff, int32_t nCols, const int32_t *colTok) {
  ApiGuard guard;
  if (!merge_map_ok(m, nCols, colTok)) return nullptr;
  return profiles_create(m, nProfiles, logP, rowOff, nCols, colTok);
}

void mb_profiles_destroy(mb_profiles *p) {
  ApiGuard guard;
  if (!p) return;
  if (p->d_logP) (void)hipFree(p->d_logP);
  if (p->d_colTok) (void)hipFree(p->d_colTok);
  delete p;
}

int mb_profiles_forward(mb_profiles *p, int flags, double *loglike) {
  ApiGuard guard;
  if (!p || (!loglike && p->n)) { set_error("null argument"); return 1; }
  if (flags != MB_ROLLING && flags != MB_MATERIALISE) { set_error("unknown flags"); return 1; }
  g_last_ms = 0.0; g_last_launches = 0;
  return profiles_scores(p, MB_FORWARD, flags == MB_MATERIALISE, loglike);
}

int64_t mb_profile_path_bound(const mb_machine *m, int64_t nRows) {
  if (!m || nRows < 0) return 0;
  return profile_path_bound(m->nLevF, nRows);
}

// (no pathCap check up front, unlike the pair calls: the cap only has to hold the paths themselves, not their bounds)
int mb_profiles_viterbi(mb_profiles *p, double *loglike, int64_t *pathOff, uint32_t *pathEdges, int32_t *pathRow, int64_t pathCap) {
  ApiGuard guard;
  if (!p || (!loglike && p->n)) { set_error("null argument"); return 1; }
  g_last_ms = 0.0; g_last_launches = 0;
  if (!pathEdges || !pathOff) return profiles_scores(p, MB_VITERBI, false, loglike);
  std::vector<Chunk> chunks;
  const long long vScratch = pf_fwd_scratch(p, true);
  auto bytes = [&](long long k) { return 8.0 * pf_cells(p, pf_rows(p, k)) + 8.0 * pf_path_bound(p, k) + 8.0 * vScratch; };
  if (!lattice_chunks(p->n, "profile", bytes, chunks)) return 1;
  SmBuf<double> d_ll;
  SmBuf<long long> d_len;
  MB_HIP(d_ll.alloc(p->n));
  if (!hip_ok(d_len.alloc(p->n), "hipMalloc(path lengths)")) return 1;
  PathSink out{pathOff, pathEdges, pathRow, nullptr, pathCap, "profile", [&](long long k) { return pf_path_bound(p, k); }};
  pathOff[0] = 0;
  int rc = for_chunks<ProfPlan>(chunks, pf_build(p), [&](const Chunk &c, ProfPlan &pl, Timer &tm) {
    const long long np = c.p1 - c.p0;
    double *pool = ws_array<double>(0, pl.cells);
    uint32_t *d_e = ws_array<uint32_t>(3, pl.paths);
    int32_t *d_r = ws_array<int32_t>(4, pl.paths);
    double *scratch = nullptr;
    if (!pool || !d_e || !d_r || profile_scratch(vScratch, np, &scratch)) return 1;
    {
      Timed t(tm, 1);
      if (pf_fwd(p, MB_VITERBI, true, pl.d, (int)np, pool, scratch, d_ll + c.p0) || pf_traceback(p, pl.d, (int)np, pool, d_e, d_r, d_len + c.p0)) return 1;
    }
    return unpack_paths(out, c.p0, np, pl.paths, nullptr, d_len + c.p0, d_e, d_r);
  });
  if (!rc) rc = fetch_loglike(loglike, d_ll, p->n);
  g_last_kernel = pf_fwd_name(p, MB_VITERBI, true);
  return rc;
}

// (no MB_DETERMINISTIC here: the counts are sums of per-profile partials, which have no fixed-point mode)
int mb_profiles_counts(mb_profiles *p, double *counts, double *loglikeSum, double *loglike) {
  ApiGuard guard;
  if (!p || !counts) { set_error("null argument"); return 1; }
  g_last_ms = 0.0; g_last_launches = 0;
  const long long nT = p->m->nTrans;
  const long long PL = pf_planes(p), cScratch = std::max(pf_fwd_scratch(p, true), pf_bwd_scratch(p));   // one buffer serves both sweeps
  std::vector<Chunk> chunks;
  auto bytes = [&](long long k) { return 8.0 * pf_cells(p, pf_rows(p, k)) + 8.0 * nT * PL + 8.0 * cScratch; };
  if (!lattice_chunks(p->n, "profile", bytes, chunks)) return 1;
  SmBuf<double> d_ll, d_bll, d_cc;
  MB_HIP(d_ll.alloc(p->n));
  if (!hip_ok(d_bll.alloc(p->n), "hipMalloc(loglike)") || !hip_ok(d_cc.alloc(nT), "hipMalloc(counts)")) return 1;
  CountSum sum(nT);
  int rc = for_chunks<ProfPlan>(chunks, pf_build(p), [&](const Chunk &c, ProfPlan &pl, Timer &tm) {
    const long long np = c.p1 - c.p0;
    double *pool = ws_array<double>(0, pl.cells);
    double *part = ws_array<double>(2, np * PL * nT);
    double *scratch = nullptr;
    if (!pool || !part || profile_scratch(cScratch, np, &scratch)) return 1;
    if (np * PL > 0x7fffffff) { set_error("too many profile planes in one chunk"); return 1; }
    {
      Timed t(tm, 1);
      if (pf_fwd(p, MB_FORWARD, true, pl.d, (int)np, pool, scratch, d_ll + c.p0)) return 1;
      if (nT && !hip_ok(hipMemsetAsync(part, 0, (size_t)np * PL * nT * sizeof(double), g_stream), "memset(counts)")) return 1;
      if (pf_bwd(p, false, pl.d, (int)np, nullptr, pool, scratch, d_bll + c.p0, part, nT)) return 1;
      if (launch_profile_sum_counts(part, (int)(np * PL), nT, d_cc, g_stream)) return 1;   // merged: over profiles, then planes
    }
    return sum.add(d_cc, false);
  });
  std::vector<double> hll((size_t)p->n);
  if (!rc) rc = fetch_loglike(hll.data(), d_ll, p->n);
  g_last_kernel = pf_name(p, "k_profile_bwd<counts>", "k_profile_merge_bwd<counts>");
  if (rc) return rc;
  sum.finish(hll, counts, loglikeSum, loglike);
  return 0;
}

// Row posteriors of plain and merged profiles: the materialised Forward, the materialised Backward and the flat k_profile_rowpost
// over both lattices (mb_profile_post.hip).  The lattices take slots 0 and 1, the Forward's scratch slot 2.
int mb_profiles_row_posteriors(mb_profiles *p, double *post, double *loglike) {
  ApiGuard guard;
  if (!p || (!post && p->totalRows)) { set_error("null argument"); return 1; }
  g_last_ms = 0.0; g_last_launches = 0;
  latch_deterministic();
  const mb_machine *m = p->m;
  const long long PL = pf_planes(p), C = pf_width(p), nv = p->totalRows * C, fScratch = pf_fwd_scratch(p, true);
  const int tabMax = rowpost_table();
  std::vector<Chunk> chunks;
  auto rowsOf = [&](long long k) { return pf_rows(p, k); };
  auto bytes = [&](long long k) { return 2.0 * 8.0 * pf_cells(p, rowsOf(k)) + 8.0 * (double)(rowsOf(k) * C) + 8.0 * fScratch; };   // both lattices, the bins, the sweeps' scratch
  if (!lattice_chunks(p->n, "profile", bytes, chunks)) return 1;
  SmBuf<double> d_ll, d_bll, d_post;
  MB_HIP(d_ll.alloc(p->n));
  if (!hip_ok(d_bll.alloc(p->n), "hipMalloc(loglike)") || !hip_ok(d_post.alloc(nv), "hipMalloc(row posteriors)")) return 1;
  int rc = for_chunks<ProfPlan>(chunks, pf_build(p), [&](const Chunk &c, ProfPlan &pl, Timer &tm) {
    const long long np = c.p1 - c.p0;
    double *fwd = ws_array<double>(0, pl.cells);
    double *bwd = ws_array<double>(1, pl.cells);
    double *scratch = fScratch && np ? (double *)ws_get(2, (size_t)(np * fScratch) * sizeof(double)) : nullptr;
    if (!fwd || !bwd || (fScratch && np && !scratch)) return 1;
    const long long groups = rowpost_groups(c.p0, c.p1, rowsOf, [&](long long k) { return profile_rowpost_rows(m->S, (int)PL, rowsOf(k), (int)C, tabMax); });
    if (np * groups > 0x7fffffff) { set_error("too many profiles in one chunk"); return 1; }
    {
      Timed t(tm, 1);
      if (pf_fwd(p, MB_FORWARD, true, pl.d, (int)np, fwd, scratch, d_ll + c.p0) || pf_bwd(p, true, pl.d, (int)np, bwd, nullptr, nullptr, d_bll + c.p0, nullptr, 0) ||
          launch_profile_rowpost(m, pf_map(p), pl.d, (int)np, (int)groups, tabMax, p->d_logP, fwd, bwd, d_ll + c.p0, d_post, g_stream)) return 1;
    }
    return hip_ok(hipStreamSynchronize(g_stream), "row posteriors") ? 0 : 1;      // (the next chunk takes the lattices over)
  });
  if (!rc) rc = fetch_posteriors(post, d_post, nv);
  if (!rc && loglike) rc = fetch_loglike(loglike, d_ll, p->n);
  g_last_kernel = pf_name(p, "k_profile_rowpost", "k_profile_merge_rowpost");
  return rc;
}

int mb_profiles_set_rows(mb_profiles *p, const double *logP) {
  ApiGuard guard;
  if (!p) { set_error("null argument"); return 1; }
  const long long nv = p->totalRows * pf_width(p);
  if (nv && !logP) { set_error("null argument"); return 1; }
  if (!profile_values_ok(logP, nv)) return 1;
  if (nv && h2d_large(p->d_logP, logP, (size_t)nv * sizeof(double))) return 1;
  return hip_ok(hipStreamSynchronize(g_stream), "H2D profiles") ? 0 : 1;
}

int mb_profile_fill(mb_machine *m, int mode, const double *logP, int64_t nRows, double *cellsOut) {
  ApiGuard guard;
  return profile_fill(m, mode, logP, nRows, 0, nullptr, cellsOut);
}

int mb_profile_fill_merged(mb_machine *m, int mode, const double *logP, int64_t nRows, int32_t nCols, const int32_t *colTok, double *cellsOut) {
  ApiGuard guard;
  if (!merge_map_ok(m, nCols, colTok)) return 1;
  return profile_fill(m, mode, logP, nRows, nCols, colTok, cellsOut);
}

}  // extern "C"

// ---- two-tape profile sweeps: an input sequence against a profile (mb_profile_pair.hip, docs/profile_tapes.md "Pairs") ----------
namespace mb {

static long long pp_in(const mb_profile_pairs *p, long long k) { return p->inOff[k + 1] - p->inOff[k]; }
static long long pp_rows(const mb_profile_pairs *p, long long k) { return p->rowOff[k + 1] - p->rowOff[k]; }
static bool pp_env(const mb_profile_pairs *p, long long k) { return p->hasEnv && p->envBase[(size_t)k] >= 0; }
// doubles of pair k's materialised lattice: the rectangle, or the compact lattice of its envelope
static long long pp_cells(const mb_profile_pairs *p, long long k) {
  if (pp_env(p, k)) return p->envCells[(size_t)k] * 2 * (long long)p->m->S * (p->nCols + 1);
  return profile_pair_cells(p->m->S, pp_in(p, k), pp_rows(p, k)) * (p->nCols + 1);
}
static double pp_cell_bytes(const mb_profile_pairs *p, long long k) { return 8.0 * (double)pp_cells(p, k); }
static long long pp_path_bound(const mb_profile_pairs *p, long long k) { return profile_pair_path_bound(p->m->nLevF, pp_in(p, k), pp_rows(p, k)); }
// The ring of pair k's sweep and its dynamic LDS (0: a slice of the global scratch buffer).  Plain profiles: the rolling sweep alone
// has one.  Merged: the materialised sweeps keep their exclusion vectors in one too (mb_profile_pair_merge.h).
static long long pp_ring(const mb_profile_pairs *p, long long k, bool rolling) {
  if (p->nCols && pp_env(p, k)) return profile_pair_merge_env_ring(p->m->S, p->nCols, p->envM[(size_t)k], !rolling);
  if (p->nCols) return profile_pair_merge_ring(p->m->S, p->nCols, pp_in(p, k), pp_rows(p, k), !rolling);
  if (pp_env(p, k)) return rolling ? profile_pair_env_ring(p->m->S, p->envM[(size_t)k]) : 0;
  return rolling ? profile_pair_ring(p->m->S, pp_in(p, k), pp_rows(p, k)) : 0;
}
static size_t pp_ring_lds(const mb_profile_pairs *p, long long k, bool rolling) {
  if (p->nCols && pp_env(p, k)) return profile_pair_merge_env_lds_bytes(p->m->S, p->nCols, p->envM[(size_t)k], !rolling);
  if (p->nCols) return profile_pair_merge_lds_bytes(p->m->S, p->nCols, pp_in(p, k), pp_rows(p, k), !rolling);
  if (pp_env(p, k)) return rolling ? profile_pair_env_lds_bytes(p->m->S, p->envM[(size_t)k]) : 0;
  return rolling ? profile_pair_lds_bytes(p->m->S, pp_in(p, k), pp_rows(p, k)) : 0;
}
// bytes of global scratch the sweep of pair k needs (0: its ring is in LDS, or it has none)
static double pp_ring_bytes(const mb_profile_pairs *p, long long k, bool rolling) {
  return pp_ring_lds(p, k, rolling) ? 0.0 : 8.0 * (double)pp_ring(p, k, rolling);
}
static MergeMap pp_map(const mb_profile_pairs *p) { return MergeMap{p->nCols, p->d_colTok}; }

// Pairs with an envelope go to the kernels' envelope geometry in a launch of their own: a chunk's pairs without one come
// first in its per-pair outputs (log-likelihoods, path lengths), then the pairs with one; slot[k - p0] is where pair k landed.
struct PairProfPlan {
  SmBuf<PairProfDesc> d; SmBuf<PairEnvDesc> e;
  long long cells = 0, paths = 0, ring = 0, maxItems = 0, maxItemsEnv = 0, nPlain = 0, nEnv = 0;
  size_t lds = 0, ldsEnv = 0;
  std::vector<long long> slot;
  int launches() const { return nEnv && nPlain ? 2 : 1; }      // one per kind of pair the chunk holds
};

// descriptors of pairs [p0, p1): lattices, traceback slots and scratch rings packed from 0; where: the call's record of the slots
static int pair_profile_descs(const mb_profile_pairs *p, long long p0, long long p1, bool rolling, PairProfPlan &pl, PairWhere *where = nullptr) {
  std::vector<PairProfDesc> h;
  std::vector<PairEnvDesc> he;
  std::vector<long long> envPairs;
  const int S = p->m->S;
  pl.slot.assign((size_t)(p1 - p0), 0);
  for (long long k = p0; k < p1; ++k) {
    const long long I = pp_in(p, k), L = pp_rows(p, k);
    long long ringBase = -1;
    if (pp_ring(p, k, rolling)) {
      const size_t lds = pp_ring_lds(p, k, rolling);
      if (lds) { if (pp_env(p, k)) pl.ldsEnv = std::max(pl.ldsEnv, lds); else pl.lds = std::max(pl.lds, lds); }
      else { ringBase = pl.ring; pl.ring += pp_ring(p, k, rolling); }
    }
    PairEnvDesc d;      // (a full pair keeps its PairProfDesc part)
    d.inBase = p->inOff[k]; d.rowBase = p->rowOff[k]; d.nIn = (int)I; d.nRows = (int)L;
    d.cellBase = pl.cells; d.pathBase = pl.paths; d.ringBase = ringBase;
    if (pp_env(p, k)) {
      d.envBase = p->envBase[(size_t)k]; d.diagBase = p->diagBase[(size_t)k]; d.nCells = p->envCells[(size_t)k]; d.M = p->envM[(size_t)k];
      pl.maxItemsEnv = std::max(pl.maxItemsEnv, (long long)d.M * S * (p->nCols + 1));
      he.push_back(d); envPairs.push_back(k);
    } else {
      pl.maxItems = std::max(pl.maxItems, (std::min(I, L) + 1) * S * (p->nCols + 1));
      pl.slot[(size_t)(k - p0)] = (long long)h.size();
      h.push_back(d);
    }
    pl.cells += pp_cells(p, k);
    pl.paths += pp_path_bound(p, k);
  }
  pl.nPlain = (long long)h.size(); pl.nEnv = (long long)he.size();
  for (size_t j = 0; j < envPairs.size(); ++j) pl.slot[(size_t)(envPairs[j] - p0)] = pl.nPlain + (long long)j;
  MB_HIP(pl.d.alloc(pl.nPlain));
  if (!hip_ok(pl.e.alloc(pl.nEnv), "hipMalloc(pair descriptors)")) return 1;
  if ((!h.empty() && !hip_ok(hipMemcpyAsync(pl.d, h.data(), h.size() * sizeof(PairProfDesc), hipMemcpyHostToDevice, g_stream), "H2D pair descriptors")) ||
      (!he.empty() && !hip_ok(hipMemcpyAsync(pl.e, he.data(), he.size() * sizeof(PairEnvDesc), hipMemcpyHostToDevice, g_stream), "H2D pair descriptors")) ||
      !hip_ok(hipStreamSynchronize(g_stream), "H2D pair descriptors")) return 1;
  if (where) {
    for (long long s : pl.slot) where->at.push_back(p0 + s);
    where->permuted = where->permuted || pl.nEnv;
  }
  return 0;
}
static auto pp_build(const mb_profile_pairs *p, bool rolling, PairWhere &where) {
  return [p, rolling, &where](const Chunk &c, PairProfPlan &pl) { return pair_profile_descs(p, c.p0, c.p1, rolling, pl, &where); };
}
static PairEnvTables pp_env_tables(const mb_profile_pairs *p) { return PairEnvTables{p->d_envStart, p->d_envEnd, p->d_envOff, p->d_diagLo, p->d_diagCnt}; }

// The one place where the plain and the merged kernels part: the launches of a chunk and the names they report.  The plain kernels
// and the merged ones alike take the chunk's full pairs, then its pairs under an envelope, through the two overloads of one launcher;
// the second launch's per-pair outputs (ll, len) follow the first's, at + nPlain.
static int pp_launch_fwd(const mb_profile_pairs *p, int mode, bool mat, const PairProfPlan &pl, double *pool, double *scratch, double *ll) {
  if (p->nCols) {
    if (launch_profile_pair_merge_fwd(p->m, pp_map(p), mode, mat, pl.d.p, (int)pl.nPlain, pl.lds, pl.maxItems, p->d_in, p->d_logP, pool, scratch, ll, g_stream)) return 1;
    return launch_profile_pair_merge_fwd(p->m, pp_map(p), mode, mat, pl.e.p, pp_env_tables(p), (int)pl.nEnv, pl.ldsEnv, pl.maxItemsEnv, p->d_in, p->d_logP, pool, scratch,
                                         ll + pl.nPlain, g_stream);
  }
  if (launch_profile_pair_fwd(p->m, mode, mat, pl.d.p, (int)pl.nPlain, mat ? 0 : pl.lds, pl.maxItems, p->d_in, p->d_logP, pool, mat ? nullptr : scratch, ll, g_stream)) return 1;
  return launch_profile_pair_fwd(p->m, mode, mat, pl.e.p, pp_env_tables(p), (int)pl.nEnv, mat ? 0 : pl.ldsEnv, pl.maxItemsEnv, p->d_in, p->d_logP, pool,
                                 mat ? nullptr : scratch, ll + pl.nPlain, g_stream);
}
static int pp_launch_bwd(const mb_profile_pairs *p, const PairProfPlan &pl, double *pool, double *scratch, double *ll) {
  if (p->nCols) {
    if (launch_profile_pair_merge_bwd(p->m, pp_map(p), pl.d.p, (int)pl.nPlain, pl.lds, pl.maxItems, p->d_in, p->d_logP, pool, scratch, ll, g_stream)) return 1;
    return launch_profile_pair_merge_bwd(p->m, pp_map(p), pl.e.p, pp_env_tables(p), (int)pl.nEnv, pl.ldsEnv, pl.maxItemsEnv, p->d_in, p->d_logP, pool, scratch,
                                         ll + pl.nPlain, g_stream);
  }
  if (launch_profile_pair_bwd(p->m, pl.d.p, (int)pl.nPlain, pl.maxItems, p->d_in, p->d_logP, pool, ll, g_stream)) return 1;
  return launch_profile_pair_bwd(p->m, pl.e.p, pp_env_tables(p), (int)pl.nEnv, pl.maxItemsEnv, p->d_in, p->d_logP, pool, ll + pl.nPlain, g_stream);
}
static int pp_launch_traceback(const mb_profile_pairs *p, const PairProfPlan &pl, const double *pool, uint32_t *e, int32_t *r, long long *len) {
  if (p->nCols) {
    if (launch_profile_pair_merge_traceback(p->m, pp_map(p), pl.d.p, (int)pl.nPlain, p->d_in, p->d_logP, pool, e, r, len, g_stream)) return 1;
    return launch_profile_pair_merge_traceback(p->m, pp_map(p), pl.e.p, pp_env_tables(p), (int)pl.nEnv, p->d_in, p->d_logP, pool, e, r, len + pl.nPlain, g_stream);
  }
  if (launch_profile_pair_traceback(p->m, pl.d.p, (int)pl.nPlain, p->d_in, p->d_logP, pool, e, r, len, g_stream)) return 1;
  return launch_profile_pair_traceback(p->m, pl.e.p, pp_env_tables(p), (int)pl.nEnv, p->d_in, p->d_logP, pool, e, r, len + pl.nPlain, g_stream);
}
static int pp_launch_counts(const mb_profile_pairs *p, const PairProfPlan &pl, int groups, const double *fwd, const double *bwd, double *cc) {
  if (p->nCols) {
    if (launch_profile_pair_merge_counts(p->m, pp_map(p), pl.d.p, (int)pl.nPlain, groups, p->d_in, p->d_logP, fwd, bwd, cc, g_stream)) return 1;
    return launch_profile_pair_merge_counts(p->m, pp_map(p), pl.e.p, pp_env_tables(p), (int)pl.nEnv, groups, p->d_in, p->d_logP, fwd, bwd, cc, g_stream);
  }
  if (launch_profile_pair_counts(p->m, pl.d.p, (int)pl.nPlain, groups, p->d_in, p->d_logP, fwd, bwd, cc, g_stream)) return 1;
  return launch_profile_pair_counts(p->m, pl.e.p, pp_env_tables(p), (int)pl.nEnv, groups, p->d_in, p->d_logP, fwd, bwd, cc, g_stream);
}
static int pp_launch_rowpost(const mb_profile_pairs *p, const PairProfPlan &pl, int groups, int tabMax, const double *fwd, const double *bwd, double *post) {
  if (launch_profile_pair_rowpost(p->m, pl.d.p, (int)pl.nPlain, groups, tabMax, p->d_in, p->d_logP, fwd, bwd, post, g_stream)) return 1;
  return launch_profile_pair_rowpost(p->m, pl.e.p, pp_env_tables(p), (int)pl.nEnv, groups, tabMax, p->d_in, p->d_logP, fwd, bwd, post, g_stream);
}
// the merged row posteriors; ll: the chunk's Forward log-likelihoods, in the order of the plan's slots
static int pp_launch_merge_rowpost(const mb_profile_pairs *p, const PairProfPlan &pl, int groups, int tabMax, const double *fwd, const double *bwd, const double *ll, double *post) {
  if (launch_profile_pair_merge_rowpost(p->m, pp_map(p), pl.d.p, (int)pl.nPlain, groups, tabMax, p->d_in, p->d_logP, fwd, bwd, ll, post, g_stream)) return 1;
  return launch_profile_pair_merge_rowpost(p->m, pp_map(p), pl.e.p, pp_env_tables(p), (int)pl.nEnv, groups, tabMax, p->d_in, p->d_logP, fwd, bwd, ll + pl.nPlain, post, g_stream);
}
static const char *pp_fwd_name(const mb_profile_pairs *p, int mode, bool mat) {
  static const char *const names[2][2][2] = {{{"k_profile_pair_fwd<sum,rolling>", "k_profile_pair_fwd<sum,mat>"}, {"k_profile_pair_fwd<max,rolling>", "k_profile_pair_fwd<max,mat>"}},
                                             {{"k_profile_pair_merge_fwd<sum,rolling>", "k_profile_pair_merge_fwd<sum,mat>"}, {"k_profile_pair_merge_fwd<max,rolling>", "k_profile_pair_merge_fwd<max,mat>"}}};
  static const char *const envNames[2][2] = {{"k_profile_pair_env_fwd<sum,rolling>", "k_profile_pair_env_fwd<sum,mat>"}, {"k_profile_pair_env_fwd<max,rolling>", "k_profile_pair_env_fwd<max,mat>"}};
  static const char *const mergeEnvNames[2][2] = {{"k_profile_pair_merge_env_fwd<sum,rolling>", "k_profile_pair_merge_env_fwd<sum,mat>"},
                                                  {"k_profile_pair_merge_env_fwd<max,rolling>", "k_profile_pair_merge_env_fwd<max,mat>"}};
  if (p->hasEnv) return (p->nCols ? mergeEnvNames : envNames)[mode == MB_VITERBI ? 1 : 0][mat ? 1 : 0];      // (a batch that mixes both kinds reports the envelope kernel)
  return names[p->nCols ? 1 : 0][mode == MB_VITERBI ? 1 : 0][mat ? 1 : 0];
}

// Forward (MB_FORWARD) or Viterbi scores without paths (MB_VITERBI); mat: through the materialised lattice
static int pair_profile_scores(mb_profile_pairs *p, int mode, bool mat, double *loglike) {
  std::vector<Chunk> chunks;
  if (!lattice_chunks(p->n, "pair", [&](long long k) { return (mat ? pp_cell_bytes(p, k) : 0.0) + pp_ring_bytes(p, k, !mat); }, chunks)) return 1;
  SmBuf<double> d_ll;
  MB_HIP(d_ll.alloc(p->n));
  PairWhere where;
  int rc = for_chunks<PairProfPlan>(chunks, pp_build(p, !mat, where), [&](const Chunk &c, PairProfPlan &pl, Timer &tm) {
    double *pool = nullptr, *scratch = nullptr;
    if (mat && !(pool = ws_array<double>(0, pl.cells))) return 1;
    if (pl.ring && !(scratch = (double *)ws_get(1, (size_t)pl.ring * sizeof(double)))) return 1;
    Timed t(tm, pl.launches());
    return pp_launch_fwd(p, mode, mat, pl, pool, scratch, d_ll + c.p0);
  });
  if (!rc) rc = fetch_loglike(loglike, d_ll, p->n, &where);
  g_last_kernel = pp_fwd_name(p, mode, mat);
  return rc;
}

// ---- envelopes of the pairs (mb_profile_pair_env.h, docs/profile_tapes.md "Pairs under an envelope") ----
static void pp_env_free(mb_profile_pairs *p) {
  if (p->d_envStart) (void)hipFree(p->d_envStart);
  if (p->d_envEnd) (void)hipFree(p->d_envEnd);
  if (p->d_envOff) (void)hipFree(p->d_envOff);
  if (p->d_diagLo) (void)hipFree(p->d_diagLo);
  if (p->d_diagCnt) (void)hipFree(p->d_diagCnt);
  p->d_envStart = p->d_envEnd = p->d_diagLo = p->d_diagCnt = nullptr; p->d_envOff = nullptr;
  p->hasEnv = false;
  p->envBase.clear(); p->diagBase.clear(); p->envCells.clear(); p->envM.clear(); p->h_envStart.clear(); p->h_envEnd.clear();
}

// EnvHost and env_add, which checks a pair's envelope and builds its tables, are mb_profile_lattice.h's.  A message of env_add: the
// call is rejected with it.
static bool env_rejected(const char *msg) {
  if (msg) set_error(msg);
  return msg != nullptr;
}
static bool env_upload(void **dst, const void *src, size_t bytes) {
  return hip_ok(hipMalloc(dst, std::max<size_t>(bytes, 8)), "hipMalloc(pair envelopes)") && h2d_large(*dst, src, bytes) == 0;
}

// A rejected call leaves the pairs without envelopes.  merged: the call came through the merged pairs' own entry.
static int profile_pairs_set_envelopes(mb_profile_pairs *p, bool merged, const int64_t *envOff, const int32_t *inStart, const int32_t *inEnd) {
  pp_env_free(p);
  if (merged && !p->nCols) { set_error("merged envelopes take merged profiles"); return 1; }
  if (!envOff) return 0;
  const long long total = envOff[p->n] - envOff[0];
  if (total && p->nCols && !merged) { set_error("envelopes take plain profiles"); return 1; }
  if (total && (!inStart || !inEnd)) { set_error("null argument"); return 1; }
  EnvHost h(p->n);
  for (long long k = 0; k < p->n; ++k) {
    const long long rows = envOff[k + 1] - envOff[k];
    if (rows == 0) continue;   // full: the pair keeps the full geometry of mb_profile_pair.hip
    if (env_rejected(env_add(h, k, pp_in(p, k), pp_rows(p, k), rows, inStart + envOff[k], inEnd + envOff[k], false))) return 1;
  }
  if (h.st.empty()) return 0;
  if (ensure_init()) return 1;
  if (!env_upload((void **)&p->d_envStart, h.st.data(), h.st.size() * sizeof(int)) || !env_upload((void **)&p->d_envEnd, h.en.data(), h.en.size() * sizeof(int)) ||
      !env_upload((void **)&p->d_envOff, h.off.data(), h.off.size() * sizeof(long long)) || !env_upload((void **)&p->d_diagLo, h.lo.data(), h.lo.size() * sizeof(int)) ||
      !env_upload((void **)&p->d_diagCnt, h.cnt.data(), h.cnt.size() * sizeof(int)) || !hip_ok(hipStreamSynchronize(g_stream), "H2D pair envelopes")) { pp_env_free(p); return 1; }
  p->envBase.swap(h.envBase); p->diagBase.swap(h.diagBase); p->envCells.swap(h.envCells); p->envM.swap(h.M);
  p->h_envStart.swap(h.st); p->h_envEnd.swap(h.en);
  p->hasEnv = true;
  return 0;
}

// nCols > 0: CTC-merged profiles, rows of nCols + 1 doubles and the column map colTok (checked by the caller)
static mb_profile_pairs *profile_pairs_create(mb_machine *m, int64_t nPairs, const int32_t *inTok, const int64_t *inOff, const double *logP,
                                              const int64_t *rowOff, int32_t nCols, const int32_t *colTok) {
  if (!m || nPairs < 0 || (nPairs > 0 && (!rowOff || !inOff))) { set_error("null argument"); return nullptr; }
  if (ensure_init()) return nullptr;
  mb_profile_pairs *p = new mb_profile_pairs();
  p->m = m; p->n = nPairs; p->nCols = nCols;
  p->rowOff.assign((size_t)nPairs + 1, 0); p->inOff.assign((size_t)nPairs + 1, 0);
  for (long long k = 0; k < nPairs; ++k) {
    const long long L = rowOff[k + 1] - rowOff[k], I = inOff[k + 1] - inOff[k];
    if (L < 0 || L > 0x3fffffff || I < 0 || I > 0x3fffffff) { set_error("bad pair offsets"); delete p; return nullptr; }
    if ((double)(std::min(I, L) + 1) * m->S * (nCols + 1) > 2147483647.0) { set_error("pair " + std::to_string(k) + ": an anti-diagonal of the lattice has more than 2^31 cells"); delete p; return nullptr; }
    p->rowOff[(size_t)k + 1] = p->rowOff[(size_t)k] + L;
    p->inOff[(size_t)k + 1] = p->inOff[(size_t)k] + I;
  }
  p->totalRows = p->rowOff.back(); p->totalIn = p->inOff.back();
  const long long C = nCols ? nCols + 1 : m->nOut + 1, nv = p->totalRows * C;
  const double *v0 = logP ? logP + (nPairs ? rowOff[0] * C : 0) : nullptr;
  const int32_t *x0 = inTok ? inTok + (nPairs ? inOff[0] : 0) : nullptr;
  if ((nv && !v0) || (p->totalIn && !x0)) { set_error("null argument"); delete p; return nullptr; }
  for (long long k = 0; k < p->totalIn; ++k)
    if (x0[k] < 1 || x0[k] > m->nIn) {
      set_error("input token " + std::to_string(x0[k]) + " at position " + std::to_string(k) + " is outside 1..nInTok (" + std::to_string(m->nIn) + ")");
      delete p; return nullptr;
    }
  if (!profile_values_ok(v0, nv)) { delete p; return nullptr; }
  if (!hip_ok(hipMalloc((void **)&p->d_logP, (size_t)std::max<long long>(nv, 1) * sizeof(double)), "hipMalloc(pair profiles)") ||
      !hip_ok(hipMalloc((void **)&p->d_in, (size_t)std::max<long long>(p->totalIn, 1) * sizeof(int)), "hipMalloc(pair inputs)")) { mb_profile_pairs_destroy(p); return nullptr; }
  if (nv && h2d_large(p->d_logP, v0, (size_t)nv * sizeof(double))) { mb_profile_pairs_destroy(p); return nullptr; }
  if (p->totalIn && h2d_large(p->d_in, x0, (size_t)p->totalIn * sizeof(int))) { mb_profile_pairs_destroy(p); return nullptr; }
  if (nCols && (!hip_ok(hipMalloc((void **)&p->d_colTok, (size_t)nCols * sizeof(int)), "hipMalloc(column map)") ||
                !hip_ok(hipMemcpyAsync(p->d_colTok, colTok, (size_t)nCols * sizeof(int), hipMemcpyHostToDevice, g_stream), "H2D column map"))) { mb_profile_pairs_destroy(p); return nullptr; }
  if (!hip_ok(hipStreamSynchronize(g_stream), "H2D pairs")) { mb_profile_pairs_destroy(p); return nullptr; }
  return p;
}

static int profile_pair_fill(mb_machine *m, int mode, const int32_t *inTok, int64_t nIn, const double *logP, int64_t nRows, int32_t nCols,
                             const int32_t *colTok, const int32_t *envStart, const int32_t *envEnd, double *cellsOut) {
  if (!m || !cellsOut || nRows < 0 || nIn < 0 || (nRows && !logP) || (nIn && !inTok)) { set_error("null argument"); return 1; }
  if (!fill_mode_ok(mode)) return 1;
  if (ensure_init()) return 1;
  g_last_ms = 0.0; g_last_launches = 0;
  const int64_t rOff[2] = {0, nRows}, iOff[2] = {0, nIn};
  mb_profile_pairs *p = profile_pairs_create(m, 1, inTok, iOff, logP, rOff, nCols, colTok);
  if (!p) return 1;
  const bool env = envStart && envEnd;
  if (env) {
    const int64_t eOff[2] = {0, nRows + 1};
    if (profile_pairs_set_envelopes(p, nCols > 0, eOff, envStart, envEnd)) { mb_profile_pairs_destroy(p); return 1; }
  }
  std::vector<Chunk> chunks;
  if (!lattice_chunks(p->n, "pair", [&](long long k) { return pp_cell_bytes(p, k) + pp_ring_bytes(p, k, false); }, chunks)) { mb_profile_pairs_destroy(p); return 1; }
  int rc;
  {
    PairProfPlan pl;
    rc = pair_profile_descs(p, 0, 1, false, pl);
    std::vector<double> compact(!rc && env ? (size_t)pl.cells : 0);      // under an envelope the lattice comes back compact
    if (!rc) rc = fill_one(pl.cells, pl.ring, env ? compact.data() : cellsOut, [&](double *pool, double *scratch, double *d_ll) {
      return mode == MB_BACKWARD ? pp_launch_bwd(p, pl, pool, scratch, d_ll) : pp_launch_fwd(p, mode, true, pl, pool, scratch, d_ll);
    });
    if (!rc && env) {      // the compact lattice into the full rectangle, -inf outside the envelope
      const size_t cellD = 2 * (size_t)m->S * (size_t)(nCols + 1);
      std::fill(cellsOut, cellsOut + (size_t)(nIn + 1) * (size_t)(nRows + 1) * cellD, -INFINITY);
      size_t at = 0;
      for (int64_t r = 0; r <= nRows; ++r)
        for (int64_t i = envStart[r]; i < envEnd[r]; ++i, at += cellD)
          std::memcpy(cellsOut + ((size_t)i * (size_t)(nRows + 1) + (size_t)r) * cellD, compact.data() + at, cellD * sizeof(double));
    }
  }
  g_last_kernel = mode == MB_BACKWARD ? (nCols ? (env ? "k_profile_pair_merge_env_bwd" : "k_profile_pair_merge_bwd") : (env ? "k_profile_pair_env_bwd" : "k_profile_pair_bwd"))
                                      : pp_fwd_name(p, mode, true);
  mb_profile_pairs_destroy(p);
  return rc;
}

}  // namespace mb

extern "C" {

mb_profile_pairs *mb_profile_pairs_create(mb_machine *m, int64_t nPairs, const int32_t *inTok, const int64_t *inOff, const double *logP, const int64_t *rowOff) {
  ApiGuard guard;
  return profile_pairs_create(m, nPairs, inTok, inOff, logP, rowOff, 0, nullptr);
}

mb_profile_pairs *mb_profile_pairs_create_merged(mb_machine *m, int64_t nPairs, const int32_t *inTok, const int64_t *inOff, const double *logP,
                                                 const int64_t *rowOff, int32_t nCols, const int32_t *colTok) {
  ApiGuard guard;
  if (!merge_map_ok(m, nCols, colTok)) return nullptr;
  return profile_pairs_create(m, nPairs, inTok, inOff, logP, rowOff, nCols, colTok);
}

void mb_profile_pairs_destroy(mb_profile_pairs *p) {
  ApiGuard guard;
  if (!p) return;
  if (p->d_logP) (void)hipFree(p->d_logP);
  if (p->d_in) (void)hipFree(p->d_in);
  if (p->d_colTok) (void)hipFree(p->d_colTok);
  pp_env_free(p);
  delete p;
}

int mb_profile_pairs_set_envelopes(mb_profile_pairs *p, const int64_t *envOff, const int32_t *inStart, const int32_t *inEnd) {
  ApiGuard guard;
  if (!p) { set_error("null argument"); return 1; }
  return profile_pairs_set_envelopes(p, false, envOff, inStart, inEnd);
}

int mb_profile_pairs_set_envelopes_merged(mb_profile_pairs *p, const int64_t *envOff, const int32_t *inStart, const int32_t *inEnd) {
  ApiGuard guard;
  if (!p) { set_error("null argument"); return 1; }
  return profile_pairs_set_envelopes(p, true, envOff, inStart, inEnd);
}

int64_t mb_profile_pairs_cells(const mb_profile_pairs *p) {
  if (!p) return 0;
  long long c = 0;
  for (long long k = 0; k < p->n; ++k) c += pp_cells(p, k);
  return c;
}

int mb_profile_pairs_forward(mb_profile_pairs *p, int flags, double *loglike) {
  ApiGuard guard;
  if (!p || (!loglike && p->n)) { set_error("null argument"); return 1; }
  if (flags != MB_ROLLING && flags != MB_MATERIALISE) { set_error("unknown flags"); return 1; }
  g_last_ms = 0.0; g_last_launches = 0;
  return pair_profile_scores(p, MB_FORWARD, flags == MB_MATERIALISE, loglike);
}

int64_t mb_profile_pair_path_bound(const mb_machine *m, int64_t nIn, int64_t nRows) {
  if (!m || nIn < 0 || nRows < 0) return 0;
  return profile_pair_path_bound(m->nLevF, nIn, nRows);
}

int mb_profile_pairs_viterbi(mb_profile_pairs *p, double *loglike, int64_t *pathOff, uint32_t *pathEdges, int32_t *pathRow, int64_t pathCap) {
  ApiGuard guard;
  if (!p || (!loglike && p->n)) { set_error("null argument"); return 1; }
  g_last_ms = 0.0; g_last_launches = 0;
  if (!pathEdges || !pathOff) return pair_profile_scores(p, MB_VITERBI, false, loglike);
  long long need = 0;
  for (long long k = 0; k < p->n; ++k) need += pp_path_bound(p, k);
  if (pathCap < need) { set_error("pathCap too small for the Viterbi paths: " + std::to_string((long long)pathCap) + " entries, the path bounds of the pairs sum to " + std::to_string(need)); return 1; }
  std::vector<Chunk> chunks;
  auto bytes = [&](long long k) { return pp_cell_bytes(p, k) + pp_ring_bytes(p, k, false) + 8.0 * pp_path_bound(p, k); };
  if (!lattice_chunks(p->n, "pair", bytes, chunks)) return 1;
  SmBuf<double> d_ll;
  SmBuf<long long> d_len;
  MB_HIP(d_ll.alloc(p->n));
  if (!hip_ok(d_len.alloc(p->n), "hipMalloc(path lengths)")) return 1;
  PathSink out{pathOff, pathEdges, pathRow, nullptr, pathCap, "pair", [&](long long k) { return pp_path_bound(p, k); }};
  pathOff[0] = 0;
  PairWhere where;
  int rc = for_chunks<PairProfPlan>(chunks, pp_build(p, false, where), [&](const Chunk &c, PairProfPlan &pl, Timer &tm) {
    const long long np = c.p1 - c.p0;
    double *pool = ws_array<double>(0, pl.cells);
    uint32_t *d_e = ws_array<uint32_t>(3, pl.paths);
    int32_t *d_r = ws_array<int32_t>(4, pl.paths);
    double *scratch = pl.ring ? (double *)ws_get(1, (size_t)pl.ring * sizeof(double)) : nullptr;
    if (!pool || !d_e || !d_r || (pl.ring && !scratch)) return 1;
    {
      Timed t(tm, pl.launches());
      if (pp_launch_fwd(p, MB_VITERBI, true, pl, pool, scratch, d_ll + c.p0) || pp_launch_traceback(p, pl, pool, d_e, d_r, d_len + c.p0)) return 1;
    }
    return unpack_paths(out, c.p0, np, pl.paths, &pl.slot, d_len + c.p0, d_e, d_r);
  });
  if (!rc) rc = fetch_loglike(loglike, d_ll, p->n, &where);
  g_last_kernel = pp_fwd_name(p, MB_VITERBI, true);
  return rc;
}

// The two sample calls: plain pairs (merged = false, rowCol unused) and pairs against merged profiles, whose lanes also write the
// column every row took.  Lengths and log probabilities arrive in slot order; path slots and rowCol are packed in pair order.
static int pair_profile_sample(mb_profile_pairs *p, bool merged, int64_t nSamples, uint64_t seed, double *loglike, int64_t *pathOff, uint32_t *pathEdges,
                               int32_t *pathRow, int32_t *rowCol, double *pathLogProb, int64_t pathCap) {
  if (!p || !pathOff || !pathEdges) { set_error("null argument"); return 1; }
  g_last_ms = 0.0; g_last_launches = 0;
  if (!merged && p->nCols) { set_error("sampling takes plain profiles"); return 1; }
  if (merged && !p->nCols) { set_error("merged sampling takes merged profiles"); return 1; }
  if (nSamples < 1) { set_error("nSamples must be at least 1"); return 1; }
  double need = 0.0;
  for (long long k = 0; k < p->n; ++k) need += (double)pp_path_bound(p, k);
  need *= (double)nSamples;
  if ((double)pathCap < need) {
    set_error("pathCap too small for the sampled paths: " + std::to_string((long long)pathCap) + " entries, nSamples times the path bounds of the pairs is " +
              std::to_string((long long)need));
    return 1;
  }
  // a pair costs its lattice, and per sample a path slot (an edge and a row per entry), a length and a log probability
  std::vector<Chunk> chunks;
  // (merged: also the ring of the fill's exclusion vectors where it does not fit LDS, and per sample a column for every row)
  auto bytes = [&](long long k) {
    return pp_cell_bytes(p, k) + pp_ring_bytes(p, k, false) + (double)nSamples * (8.0 * (double)pp_path_bound(p, k) + 16.0 + (merged ? 4.0 * (double)pp_rows(p, k) : 0.0));
  };
  if (!lattice_chunks(p->n, "pair", bytes, chunks)) return 1;
  for (const Chunk &c : chunks)
    if ((double)(c.p1 - c.p0) * (double)nSamples > 2147483647.0) { set_error("too many samples in one chunk: pairs times nSamples exceeds 2^31 - 1 lanes"); return 1; }
  SmBuf<double> d_ll;
  MB_HIP(d_ll.alloc(p->n));
  const int nS = (int)nSamples;
  std::vector<long long> hidx;
  SampleSink out{pathOff, pathEdges, pathRow, nullptr, pathLogProb, nSamples, [&](long long k) { return pp_path_bound(p, k); }};
  pathOff[0] = 0;
  PairWhere where;
  int rc = for_chunks<PairProfPlan>(chunks, pp_build(p, false, where), [&](const Chunk &c, PairProfPlan &pl, Timer &tm) {
    const long long np = c.p1 - c.p0, lanes = np * nS, entries = pl.paths * nS;
    const long long row0 = p->rowOff[(size_t)c.p0], colEntries = merged ? (p->rowOff[(size_t)c.p1] - row0) * nS : 0;
    double *pool = ws_array<double>(0, pl.cells);
    double *scratch = pl.ring ? (double *)ws_get(1, (size_t)pl.ring * sizeof(double)) : nullptr;
    int32_t *d_rc = merged ? ws_array<int32_t>(7, colEntries) : nullptr;
    if ((pl.ring && !scratch) || (merged && !d_rc)) return 1;
    uint32_t *d_e = ws_array<uint32_t>(3, entries);
    int32_t *d_r = ws_array<int32_t>(4, entries);
    long long *d_len = ws_array<long long>(5, lanes);
    double *d_lq = ws_array<double>(6, lanes);
    SmBuf<long long> d_idx;
    if (!pool || !d_e || !d_r || !d_len || !d_lq || !hip_ok(d_idx.alloc(np), "hipMalloc(pair indices)")) return 1;
    hidx.assign((size_t)np, 0);
    for (long long k = 0; k < np; ++k) hidx[(size_t)pl.slot[(size_t)k]] = c.p0 + k;      // the kernels see the pairs in slot order
    if (np && (!hip_ok(hipMemcpyAsync(d_idx.p, hidx.data(), (size_t)np * sizeof(long long), hipMemcpyHostToDevice, g_stream), "H2D pair indices") ||
               !hip_ok(hipStreamSynchronize(g_stream), "H2D pair indices"))) return 1;
    {
      Timed t(tm, pl.launches());
      if (pp_launch_fwd(p, MB_FORWARD, true, pl, pool, scratch, d_ll + c.p0)) return 1;
      if (merged) {
        if (launch_profile_pair_merge_sample(p->m, pp_map(p), pl.d.p, (int)pl.nPlain, nS, d_idx.p, seed, p->d_in, p->d_logP, pool, row0, d_e, d_r, d_rc, d_len, d_lq,
                                             g_stream)) return 1;
        if (launch_profile_pair_merge_sample(p->m, pp_map(p), pl.e.p, pp_env_tables(p), (int)pl.nEnv, nS, d_idx.p + pl.nPlain, seed, p->d_in, p->d_logP, pool, row0, d_e,
                                             d_r, d_rc, d_len + pl.nPlain * nS, d_lq + pl.nPlain * nS, g_stream)) return 1;
      } else {
        if (launch_profile_pair_sample(p->m, pl.d.p, (int)pl.nPlain, nS, d_idx.p, seed, p->d_in, p->d_logP, pool, d_e, d_r, d_len, d_lq, g_stream)) return 1;
        if (launch_profile_pair_sample(p->m, pl.e.p, pp_env_tables(p), (int)pl.nEnv, nS, d_idx.p + pl.nPlain, seed, p->d_in, p->d_logP, pool, d_e, d_r,
                                       d_len + pl.nPlain * nS, d_lq + pl.nPlain * nS, g_stream)) return 1;
      }
    }
    // lengths and log probabilities landed in slot order, the path slots are packed in pair order
    if (unpack_samples(out, c.p0, np, entries, &pl.slot, d_len, d_lq, d_e, d_r)) return 1;
    // (the chunk's block of rowCol is already in pair order: rows of the object from row0 on, nSamples lines per pair)
    return rowCol && colEntries && d2h_large(rowCol + (row0 - p->rowOff[0]) * nS, d_rc, (size_t)colEntries * sizeof(int32_t)) ? 1 : 0;
  });
  if (!rc && loglike) rc = fetch_loglike(loglike, d_ll, p->n, &where);
  if (merged) g_last_kernel = p->hasEnv ? "k_profile_pair_merge_env_sample" : "k_profile_pair_merge_sample";
  else g_last_kernel = p->hasEnv ? "k_profile_pair_env_sample" : "k_profile_pair_sample";
  return rc;
}

int mb_profile_pairs_sample(mb_profile_pairs *p, int64_t nSamples, uint64_t seed, double *loglike, int64_t *pathOff, uint32_t *pathEdges, int32_t *pathRow,
                            double *pathLogProb, int64_t pathCap) {
  ApiGuard guard;
  return pair_profile_sample(p, false, nSamples, seed, loglike, pathOff, pathEdges, pathRow, nullptr, pathLogProb, pathCap);
}

int mb_profile_pairs_sample_merged(mb_profile_pairs *p, int64_t nSamples, uint64_t seed, double *loglike, int64_t *pathOff, uint32_t *pathEdges, int32_t *pathRow,
                                   int32_t *rowCol, double *pathLogProb, int64_t pathCap) {
  ApiGuard guard;
  return pair_profile_sample(p, true, nSamples, seed, loglike, pathOff, pathEdges, pathRow, rowCol, pathLogProb, pathCap);
}

int mb_profile_pairs_counts(mb_profile_pairs *p, double *counts, double *loglikeSum, double *loglike) {
  ApiGuard guard;
  if (!p || !counts) { set_error("null argument"); return 1; }
  g_last_ms = 0.0; g_last_launches = 0;
  latch_deterministic();
  const long long nT = p->m->nTrans;
  std::vector<Chunk> chunks;
  if (!lattice_chunks(p->n, "pair", [&](long long k) { return 2.0 * pp_cell_bytes(p, k) + pp_ring_bytes(p, k, false); }, chunks)) return 1;   // the Forward and the Backward lattice
  SmBuf<double> d_ll, d_bll, d_cc;
  MB_HIP(d_ll.alloc(p->n));
  if (!hip_ok(d_bll.alloc(p->n), "hipMalloc(loglike)") || !hip_ok(d_cc.alloc(nT), "hipMalloc(counts)")) return 1;
  CountSum sum(nT);
  PairWhere where;
  int rc = for_chunks<PairProfPlan>(chunks, pp_build(p, false, where), [&](const Chunk &c, PairProfPlan &pl, Timer &tm) {
    const long long np = c.p1 - c.p0;
    double *fwd = ws_array<double>(0, pl.cells);
    double *bwd = ws_array<double>(1, pl.cells);
    double *scratch = pl.ring ? (double *)ws_get(2, (size_t)pl.ring * sizeof(double)) : nullptr;
    if (!fwd || !bwd || (pl.ring && !scratch)) return 1;
    const int groups = count_groups(c.p0, c.p1, [&](long long k) { return pp_cells(p, k) / 2; });
    if (np * groups > 0x7fffffff) { set_error("too many pairs in one chunk"); return 1; }
    {
      Timed t(tm, pl.launches());
      if (pp_launch_fwd(p, MB_FORWARD, true, pl, fwd, scratch, d_ll + c.p0)) return 1;      // (merged: the Backward's ring follows the Forward's on the stream, one scratch buffer serves both)
      if (pp_launch_bwd(p, pl, bwd, scratch, d_bll + c.p0)) return 1;
      if (nT && !hip_ok(hipMemsetAsync(d_cc, 0, (size_t)nT * sizeof(double), g_stream), "memset(counts)")) return 1;
      if (pp_launch_counts(p, pl, groups, fwd, bwd, d_cc)) return 1;
    }
    return sum.add(d_cc, g_deterministic);
  });
  std::vector<double> hll((size_t)p->n);
  if (!rc) rc = fetch_loglike(hll.data(), d_ll, p->n, &where);
  g_last_kernel = p->nCols ? (p->hasEnv ? "k_profile_pair_merge_env_counts" : "k_profile_pair_merge_counts") : (p->hasEnv ? "k_profile_pair_env_counts" : "k_profile_pair_counts");
  if (rc) return rc;
  sum.finish(hll, counts, loglikeSum, loglike);
  return 0;
}

int mb_profile_pairs_row_posteriors(mb_profile_pairs *p, double *post, double *loglike) {
  ApiGuard guard;
  if (!p || (!post && p->totalRows)) { set_error("null argument"); return 1; }
  if (p->nCols) { set_error("row posteriors take plain profiles"); return 1; }
  g_last_ms = 0.0; g_last_launches = 0;
  latch_deterministic();
  const mb_machine *m = p->m;
  const long long C = m->nOut + 1, nv = p->totalRows * C;
  const int tabMax = rowpost_table();
  std::vector<Chunk> chunks;
  auto bytes = [&](long long k) { return 2.0 * pp_cell_bytes(p, k) + pp_ring_bytes(p, k, false) + 8.0 * (double)(pp_rows(p, k) * C); };   // both lattices and the pair's bins
  if (!lattice_chunks(p->n, "pair", bytes, chunks)) return 1;
  SmBuf<double> d_ll, d_bll, d_post;
  MB_HIP(d_ll.alloc(p->n));
  if (!hip_ok(d_bll.alloc(p->n), "hipMalloc(loglike)") || !hip_ok(d_post.alloc(nv), "hipMalloc(row posteriors)")) return 1;
  PairWhere where;
  int rc = for_chunks<PairProfPlan>(chunks, pp_build(p, false, where), [&](const Chunk &c, PairProfPlan &pl, Timer &tm) {
    const long long np = c.p1 - c.p0;
    double *fwd = ws_array<double>(0, pl.cells);
    double *bwd = ws_array<double>(1, pl.cells);
    if (!fwd || !bwd) return 1;
    const long long groups = rowpost_groups(c.p0, c.p1, [&](long long k) { return pp_rows(p, k); }, [&](long long k) {
      return profile_pair_rowpost_rows(pp_cells(p, k) / (2 * (long long)m->S), m->S, (int)pp_rows(p, k), (int)C, tabMax);
    });
    if (np * groups > 0x7fffffff) { set_error("too many pairs in one chunk"); return 1; }
    {
      Timed t(tm, pl.launches());
      if (pp_launch_fwd(p, MB_FORWARD, true, pl, fwd, nullptr, d_ll + c.p0) || pp_launch_bwd(p, pl, bwd, nullptr, d_bll + c.p0) ||
          pp_launch_rowpost(p, pl, (int)groups, tabMax, fwd, bwd, d_post)) return 1;
    }
    return hip_ok(hipStreamSynchronize(g_stream), "row posteriors") ? 0 : 1;      // (the next chunk takes the lattices over)
  });
  if (!rc) rc = fetch_posteriors(post, d_post, nv);
  if (!rc && loglike) rc = fetch_loglike(loglike, d_ll, p->n, &where);
  g_last_kernel = p->hasEnv ? "k_profile_pair_env_rowpost" : "k_profile_pair_rowpost";
  return rc;
}

int mb_profile_pairs_set_rows(mb_profile_pairs *p, const double *logP) {
  ApiGuard guard;
  if (!p) { set_error("null argument"); return 1; }
  if (p->nCols) { set_error("row posteriors take plain profiles"); return 1; }
  const long long nv = p->totalRows * (p->m->nOut + 1);
  if (nv && !logP) { set_error("null argument"); return 1; }
  if (!profile_values_ok(logP, nv)) return 1;
  if (nv && h2d_large(p->d_logP, logP, (size_t)nv * sizeof(double))) return 1;
  return hip_ok(hipStreamSynchronize(g_stream), "H2D pair profiles") ? 0 : 1;
}

// The merged pairs' own entry: mb_profile_pairs_counts on a merged object chunk for chunk -- the materialised merged Forward and
// Backward, whose X / T rings share one scratch buffer -- then the flat k_profile_pair_merge_rowpost over the two lattices.
int mb_profile_pairs_row_posteriors_merged(mb_profile_pairs *p, double *post, double *loglike) {
  ApiGuard guard;
  if (!p || (!post && p->totalRows)) { set_error("null argument"); return 1; }
  if (!p->nCols) { set_error("merged row posteriors take merged profiles"); return 1; }
  g_last_ms = 0.0; g_last_launches = 0;
  latch_deterministic();
  const mb_machine *m = p->m;
  const long long PL = p->nCols + 1, nv = p->totalRows * PL;
  const int tabMax = rowpost_table();
  std::vector<Chunk> chunks;
  auto bytes = [&](long long k) { return 2.0 * pp_cell_bytes(p, k) + pp_ring_bytes(p, k, false) + 8.0 * (double)(pp_rows(p, k) * PL); };   // both lattices, the X / T ring and the pair's bins
  if (!lattice_chunks(p->n, "pair", bytes, chunks)) return 1;
  SmBuf<double> d_ll, d_bll, d_post;
  MB_HIP(d_ll.alloc(p->n));
  if (!hip_ok(d_bll.alloc(p->n), "hipMalloc(loglike)") || !hip_ok(d_post.alloc(nv), "hipMalloc(row posteriors)")) return 1;
  PairWhere where;
  int rc = for_chunks<PairProfPlan>(chunks, pp_build(p, false, where), [&](const Chunk &c, PairProfPlan &pl, Timer &tm) {
    const long long np = c.p1 - c.p0;
    double *fwd = ws_array<double>(0, pl.cells);
    double *bwd = ws_array<double>(1, pl.cells);
    double *scratch = pl.ring ? (double *)ws_get(2, (size_t)pl.ring * sizeof(double)) : nullptr;
    if (!fwd || !bwd || (pl.ring && !scratch)) return 1;
    const long long groups = rowpost_groups(c.p0, c.p1, [&](long long k) { return pp_rows(p, k); }, [&](long long k) {
      return profile_pair_rowpost_rows(pp_cells(p, k) / (2 * (long long)m->S), m->S, (int)pp_rows(p, k), (int)PL, tabMax);
    });
    if (np * groups > 0x7fffffff) { set_error("too many pairs in one chunk"); return 1; }
    {
      Timed t(tm, pl.launches());
      if (pp_launch_fwd(p, MB_FORWARD, true, pl, fwd, scratch, d_ll + c.p0) || pp_launch_bwd(p, pl, bwd, scratch, d_bll + c.p0) ||
          pp_launch_merge_rowpost(p, pl, (int)groups, tabMax, fwd, bwd, d_ll + c.p0, d_post)) return 1;
    }
    return hip_ok(hipStreamSynchronize(g_stream), "row posteriors") ? 0 : 1;      // (the next chunk takes the lattices over)
  });
  if (!rc) rc = fetch_posteriors(post, d_post, nv);
  if (!rc && loglike) rc = fetch_loglike(loglike, d_ll, p->n, &where);
  g_last_kernel = p->hasEnv ? "k_profile_pair_merge_env_rowpost" : "k_profile_pair_merge_rowpost";
  return rc;
}

int mb_profile_pairs_set_rows_merged(mb_profile_pairs *p, const double *logP) {
  ApiGuard guard;
  if (!p) { set_error("null argument"); return 1; }
  if (!p->nCols) { set_error("merged row posteriors take merged profiles"); return 1; }
  const long long nv = p->totalRows * (p->nCols + 1);
  if (nv && !logP) { set_error("null argument"); return 1; }
  if (!profile_values_ok(logP, nv)) return 1;
  if (nv && h2d_large(p->d_logP, logP, (size_t)nv * sizeof(double))) return 1;
  return hip_ok(hipStreamSynchronize(g_stream), "H2D pair profiles") ? 0 : 1;
}

int mb_profile_pair_fill(mb_machine *m, int mode, const int32_t *inTok, int64_t nIn, const double *logP, int64_t nRows, double *cellsOut) {
  ApiGuard guard;
  return profile_pair_fill(m, mode, inTok, nIn, logP, nRows, 0, nullptr, nullptr, nullptr, cellsOut);
}

int mb_profile_pair_fill_env(mb_machine *m, int mode, const int32_t *inTok, int64_t nIn, const double *logP, int64_t nRows,
                             const int32_t *envStart, const int32_t *envEnd, double *cellsOut) {
  ApiGuard guard;
  if ((envStart == nullptr) != (envEnd == nullptr)) { set_error("null argument"); return 1; }
  return profile_pair_fill(m, mode, inTok, nIn, logP, nRows, 0, nullptr, envStart, envEnd, cellsOut);
}

int mb_profile_pair_fill_merged(mb_machine *m, int mode, const int32_t *inTok, int64_t nIn, const double *logP, int64_t nRows, int32_t nCols,
                                const int32_t *colTok, double *cellsOut) {
  ApiGuard guard;
  if (!merge_map_ok(m, nCols, colTok)) return 1;
  return profile_pair_fill(m, mode, inTok, nIn, logP, nRows, nCols, colTok, nullptr, nullptr, cellsOut);
}

int mb_profile_pair_fill_merged_env(mb_machine *m, int mode, const int32_t *inTok, int64_t nIn, const double *logP, int64_t nRows, int32_t nCols,
                                    const int32_t *colTok, const int32_t *envStart, const int32_t *envEnd, double *cellsOut) {
  ApiGuard guard;
  if ((envStart == nullptr) != (envEnd == nullptr)) { set_error("null argument"); return 1; }
  if (!merge_map_ok(m, nCols, colTok)) return 1;
  return profile_pair_fill(m, mode, inTok, nIn, logP, nRows, nCols, colTok, envStart, envEnd, cellsOut);
}

}  // extern "C"

// ---- two-profile sweeps: an input profile against an output profile (mb_profile_two.hip, docs/profile_tapes.md "Pairs of profiles") --
namespace mb {

static long long pt_in(const mb_profile_twos *p, long long k) { return p->inOff[k + 1] - p->inOff[k]; }
static long long pt_rows(const mb_profile_twos *p, long long k) { return p->rowOff[k + 1] - p->rowOff[k]; }
// cells (of three layers of S states) of pair k's materialised lattice: the rectangle, or the compact lattice under the envelopes
static long long pt_ncells(const mb_profile_twos *p, long long k) { return p->hasEnv ? p->envCells[(size_t)k] : (pt_in(p, k) + 1) * (pt_rows(p, k) + 1); }
static long long pt_cells(const mb_profile_twos *p, long long k) { return pt_ncells(p, k) * 3 * (long long)p->m->S * (p->nCols + 1); }
static double pt_cell_bytes(const mb_profile_twos *p, long long k) { return 8.0 * (double)pt_cells(p, k); }
// The ring of pair k's sweep and its dynamic LDS (0: a slice of the global scratch buffer).  Plain profiles: the rolling sweep alone
// has one.  Merged: the materialised sweeps keep their exclusion vectors in one too (mb_profile_two_merge.h).
static long long pt_ring(const mb_profile_twos *p, long long k, bool rolling) {
  if (p->nCols && p->hasEnv) return profile_two_merge_env_ring(p->m->S, p->nCols, p->envM[(size_t)k], !rolling);
  if (p->nCols) return profile_two_merge_ring(p->m->S, p->nCols, pt_in(p, k), pt_rows(p, k), !rolling);
  if (!rolling) return 0;
  return p->hasEnv ? profile_two_env_ring(p->m->S, p->envM[(size_t)k]) : profile_two_ring(p->m->S, pt_in(p, k), pt_rows(p, k));
}
static size_t pt_ring_lds(const mb_profile_twos *p, long long k, bool rolling) {
  if (p->nCols && p->hasEnv) return profile_two_merge_env_lds_bytes(p->m->S, p->nCols, p->envM[(size_t)k], !rolling);
  if (p->nCols) return profile_two_merge_lds_bytes(p->m->S, p->nCols, pt_in(p, k), pt_rows(p, k), !rolling);
  if (!rolling) return 0;
  return p->hasEnv ? profile_two_env_lds_bytes(p->m->S, p->envM[(size_t)k]) : profile_two_lds_bytes(p->m->S, pt_in(p, k), pt_rows(p, k));
}
// bytes of global scratch the sweep of pair k needs (0: its ring is in LDS, or it has none)
static double pt_ring_bytes(const mb_profile_twos *p, long long k, bool rolling) { return pt_ring_lds(p, k, rolling) ? 0.0 : 8.0 * (double)pt_ring(p, k, rolling); }
static long long pt_width(const mb_profile_twos *p) { return p->nCols ? p->nCols + 1 : p->m->nOut + 1; }   // doubles of an output row
static MergeMap pt_map(const mb_profile_twos *p) { return MergeMap{p->nCols, p->d_colTok}; }
static long long pt_path_bound(const mb_profile_twos *p, long long k) { return profile_pair_path_bound(p->m->nLevF, pt_in(p, k), pt_rows(p, k)); }

// No call mixes geometries: without envelopes every pair has a PairProfDesc in d, with them every pair a TwoEnvDesc in e (a pair
// that was given none runs under the full envelope).  One launch per kernel and chunk either way, the pairs in their order.
struct TwoProfPlan {
  SmBuf<PairProfDesc> d; SmBuf<TwoEnvDesc> e;
  long long cells = 0, paths = 0, ring = 0, maxItems = 0;
  size_t lds = 0;
};

// descriptors of pairs [p0, p1): lattices, traceback slots and scratch rings (rolling; merged: the materialised sweeps' too) packed from 0
static int two_profile_descs(const mb_profile_twos *p, long long p0, long long p1, bool rolling, TwoProfPlan &pl) {
  std::vector<PairProfDesc> h;
  std::vector<TwoEnvDesc> he;
  const int S = p->m->S;
  for (long long k = p0; k < p1; ++k) {
    const long long K = pt_in(p, k), L = pt_rows(p, k);
    TwoEnvDesc d;      // (without envelopes its PairProfDesc part alone is kept)
    d.inBase = p->inOff[k]; d.rowBase = p->rowOff[k]; d.nIn = (int)K; d.nRows = (int)L;
    d.cellBase = pl.cells; d.pathBase = pl.paths; d.ringBase = -1;
    if (pt_ring(p, k, rolling)) {
      const size_t lds = pt_ring_lds(p, k, rolling);
      if (lds) pl.lds = std::max(pl.lds, lds);
      else { d.ringBase = pl.ring; pl.ring += pt_ring(p, k, rolling); }
    }
    pl.cells += pt_cells(p, k);
    pl.paths += pt_path_bound(p, k);
    if (p->hasEnv) {
      d.envBase = p->envBase[(size_t)k]; d.diagBase = p->diagBase[(size_t)k]; d.colBase = p->colBase[(size_t)k];
      d.nCells = p->envCells[(size_t)k]; d.M = p->envM[(size_t)k];
      pl.maxItems = std::max(pl.maxItems, (long long)d.M * S * (p->nCols + 1));
      he.push_back(d);
    } else {
      pl.maxItems = std::max(pl.maxItems, (std::min(K, L) + 1) * S * (p->nCols + 1));
      h.push_back(d);
    }
  }
  MB_HIP(pl.d.alloc((long long)h.size()));
  if (!hip_ok(pl.e.alloc((long long)he.size()), "hipMalloc(pair descriptors)")) return 1;
  if ((!h.empty() && !hip_ok(hipMemcpyAsync(pl.d, h.data(), h.size() * sizeof(PairProfDesc), hipMemcpyHostToDevice, g_stream), "H2D pair descriptors")) ||
      (!he.empty() && !hip_ok(hipMemcpyAsync(pl.e, he.data(), he.size() * sizeof(TwoEnvDesc), hipMemcpyHostToDevice, g_stream), "H2D pair descriptors")) ||
      !hip_ok(hipStreamSynchronize(g_stream), "H2D pair descriptors")) return 1;
  return 0;
}
static auto pt_build(const mb_profile_twos *p, bool rolling) {
  return [p, rolling](const Chunk &c, TwoProfPlan &pl) { return two_profile_descs(p, c.p0, c.p1, rolling, pl); };
}
static TwoEnvTables pt_env_tables(const mb_profile_twos *p) {
  TwoEnvTables t;
  t.envStart = p->d_envStart; t.envEnd = p->d_envEnd; t.envOff = p->d_envOff; t.diagLo = p->d_diagLo; t.diagCnt = p->d_diagCnt;
  t.colStart = p->d_colStart; t.colEnd = p->d_colEnd; t.colOff = p->d_colOff;
  return t;
}
// The one place where the two geometries and the merged kernels part: the launches of a chunk of np pairs and the names they
// report.  scratch: the chunk's rings that did not fit LDS (plain: the rolling sweep's alone).
static int pt_fwd(const mb_profile_twos *p, int mode, bool mat, const TwoProfPlan &pl, long long np, double *pool, double *scratch, double *ll) {
  if (p->nCols && p->hasEnv) return launch_profile_two_merge_fwd(p->m, pt_map(p), mode, mat, pl.e.p, pt_env_tables(p), (int)np, pl.lds, pl.maxItems, p->d_logA, p->d_logB, pool, scratch, ll, g_stream);
  if (p->nCols) return launch_profile_two_merge_fwd(p->m, pt_map(p), mode, mat, pl.d.p, (int)np, pl.lds, pl.maxItems, p->d_logA, p->d_logB, pool, scratch, ll, g_stream);
  if (p->hasEnv) return launch_profile_two_fwd(p->m, mode, mat, pl.e.p, pt_env_tables(p), (int)np, mat ? 0 : pl.lds, pl.maxItems, p->d_logA, p->d_logB, pool, mat ? nullptr : scratch, ll, g_stream);
  return launch_profile_two_fwd(p->m, mode, mat, pl.d.p, (int)np, mat ? 0 : pl.lds, pl.maxItems, p->d_logA, p->d_logB, pool, mat ? nullptr : scratch, ll, g_stream);
}
static int pt_fwd_mat(const mb_profile_twos *p, int mode, const TwoProfPlan &pl, long long np, double *pool, double *scratch, double *ll) { return pt_fwd(p, mode, true, pl, np, pool, scratch, ll); }
static int pt_bwd(const mb_profile_twos *p, const TwoProfPlan &pl, long long np, double *pool, double *scratch, double *ll) {
  if (p->nCols && p->hasEnv) return launch_profile_two_merge_bwd(p->m, pt_map(p), pl.e.p, pt_env_tables(p), (int)np, pl.lds, pl.maxItems, p->d_logA, p->d_logB, pool, scratch, ll, g_stream);
  if (p->nCols) return launch_profile_two_merge_bwd(p->m, pt_map(p), pl.d.p, (int)np, pl.lds, pl.maxItems, p->d_logA, p->d_logB, pool, scratch, ll, g_stream);
  if (p->hasEnv) return launch_profile_two_bwd(p->m, pl.e.p, pt_env_tables(p), (int)np, pl.maxItems, p->d_logA, p->d_logB, pool, ll, g_stream);
  return launch_profile_two_bwd(p->m, pl.d.p, (int)np, pl.maxItems, p->d_logA, p->d_logB, pool, ll, g_stream);
}
static int pt_counts(const mb_profile_twos *p, const TwoProfPlan &pl, long long np, int groups, const double *fwd, const double *bwd, double *cc) {
  if (p->nCols && p->hasEnv) return launch_profile_two_merge_counts(p->m, pt_map(p), pl.e.p, pt_env_tables(p), (int)np, groups, p->d_logA, p->d_logB, fwd, bwd, cc, g_stream);
  if (p->nCols) return launch_profile_two_merge_counts(p->m, pt_map(p), pl.d.p, (int)np, groups, p->d_logA, p->d_logB, fwd, bwd, cc, g_stream);
  if (p->hasEnv) return launch_profile_two_counts(p->m, pl.e.p, pt_env_tables(p), (int)np, groups, p->d_logA, p->d_logB, fwd, bwd, cc, g_stream);
  return launch_profile_two_counts(p->m, pl.d.p, (int)np, groups, p->d_logA, p->d_logB, fwd, bwd, cc, g_stream);
}
static int pt_rowpost(const mb_profile_twos *p, int axis, const TwoProfPlan &pl, long long np, int groups, int tabMax, const double *fwd, const double *bwd, double *post) {
  if (p->hasEnv) return launch_profile_two_rowpost(p->m, axis, pl.e.p, pt_env_tables(p), (int)np, groups, tabMax, p->d_logA, p->d_logB, fwd, bwd, post, g_stream);
  return launch_profile_two_rowpost(p->m, axis, pl.d.p, (int)np, groups, tabMax, p->d_logA, p->d_logB, fwd, bwd, post, g_stream);
}
// the merged row posteriors; ll: the chunk's Forward log-likelihoods
static int pt_merge_rowpost(const mb_profile_twos *p, int axis, const TwoProfPlan &pl, long long np, int groups, int tabMax, const double *fwd, const double *bwd, const double *ll, double *post) {
  if (p->hasEnv) return launch_profile_two_merge_rowpost(p->m, pt_map(p), axis, pl.e.p, pt_env_tables(p), (int)np, groups, tabMax, p->d_logA, p->d_logB, fwd, bwd, ll, post, g_stream);
  return launch_profile_two_merge_rowpost(p->m, pt_map(p), axis, pl.d.p, (int)np, groups, tabMax, p->d_logA, p->d_logB, fwd, bwd, ll, post, g_stream);
}
static int pt_traceback(const mb_profile_twos *p, const TwoProfPlan &pl, long long np, const double *pool, uint32_t *e, int32_t *r, int32_t *i, long long *len) {
  if (p->nCols && p->hasEnv) return launch_profile_two_merge_traceback(p->m, pt_map(p), pl.e.p, pt_env_tables(p), (int)np, p->d_logA, p->d_logB, pool, e, r, i, len, g_stream);
  if (p->nCols) return launch_profile_two_merge_traceback(p->m, pt_map(p), pl.d.p, (int)np, p->d_logA, p->d_logB, pool, e, r, i, len, g_stream);
  if (p->hasEnv) return launch_profile_two_traceback(p->m, pl.e.p, pt_env_tables(p), (int)np, p->d_logA, p->d_logB, pool, e, r, i, len, g_stream);
  return launch_profile_two_traceback(p->m, pl.d.p, (int)np, p->d_logA, p->d_logB, pool, e, r, i, len, g_stream);
}

static const char *pt_fwd_name(const mb_profile_twos *p, int mode, bool mat) {
  static const char *const names[2][2][2] = {{{"k_profile_two_fwd<sum,rolling>", "k_profile_two_fwd<sum,mat>"}, {"k_profile_two_fwd<max,rolling>", "k_profile_two_fwd<max,mat>"}},
                                             {{"k_profile_two_env_fwd<sum,rolling>", "k_profile_two_env_fwd<sum,mat>"}, {"k_profile_two_env_fwd<max,rolling>", "k_profile_two_env_fwd<max,mat>"}}};
  static const char *const merged[2][2] = {{"k_profile_two_merge_fwd<sum,rolling>", "k_profile_two_merge_fwd<sum,mat>"}, {"k_profile_two_merge_fwd<max,rolling>", "k_profile_two_merge_fwd<max,mat>"}};
  static const char *const mergedEnv[2][2] = {{"k_profile_two_merge_env_fwd<sum,rolling>", "k_profile_two_merge_env_fwd<sum,mat>"},
                                              {"k_profile_two_merge_env_fwd<max,rolling>", "k_profile_two_merge_env_fwd<max,mat>"}};
  if (p->nCols) return (p->hasEnv ? mergedEnv : merged)[mode == MB_VITERBI ? 1 : 0][mat ? 1 : 0];
  return names[p->hasEnv ? 1 : 0][mode == MB_VITERBI ? 1 : 0][mat ? 1 : 0];
}
static const char *pt_name(const mb_profile_twos *p, const char *plain, const char *env, const char *merged, const char *mergedEnv) {
  return p->nCols ? (p->hasEnv ? mergedEnv : merged) : (p->hasEnv ? env : plain);
}

// ---- envelopes of the two-profile pairs (mb_profile_two_env.h, docs/profile_tapes.md "Pairs of profiles under an envelope") ----
static void pt_env_free(mb_profile_twos *p) {
  for (void *q : {(void *)p->d_envStart, (void *)p->d_envEnd, (void *)p->d_diagLo, (void *)p->d_diagCnt, (void *)p->d_colStart, (void *)p->d_colEnd,
                  (void *)p->d_envOff, (void *)p->d_colOff})
    if (q) (void)hipFree(q);
  p->d_envStart = p->d_envEnd = p->d_diagLo = p->d_diagCnt = p->d_colStart = p->d_colEnd = nullptr; p->d_envOff = p->d_colOff = nullptr;
  p->hasEnv = false;
  p->envBase.clear(); p->diagBase.clear(); p->colBase.clear(); p->envCells.clear(); p->envM.clear();
}

// The checks and the row tables are those of the pairs (env_add), with the transposed envelope (colStart, colEnd, colOff) as well.
// If any pair has an envelope every pair gets one, the full envelope where none was given.  A rejected
// call leaves the pairs without envelopes.  merged: the call came through the merged pairs' own entry; the merged kernels take the
// same tables.
static int profile_twos_set_envelopes(mb_profile_twos *p, bool merged, const int64_t *envOff, const int32_t *inStart, const int32_t *inEnd) {
  pt_env_free(p);
  if (merged && !p->nCols) { set_error("merged envelopes take merged profiles"); return 1; }
  if (!envOff) return 0;
  const long long total = envOff[p->n] - envOff[0];
  if (!total) return 0;
  if (p->nCols && !merged) { set_error("envelopes take plain profiles"); return 1; }
  if (!inStart || !inEnd) { set_error("null argument"); return 1; }
  EnvHost h(p->n);
  std::vector<int> fullSt, fullEn;
  for (long long k = 0; k < p->n; ++k) {
    const long long rows = envOff[k + 1] - envOff[k], K = pt_in(p, k), L = pt_rows(p, k);
    if (rows) {
      if (env_rejected(env_add(h, k, K, L, rows, inStart + envOff[k], inEnd + envOff[k], true))) return 1;
    } else {
      fullSt.assign((size_t)L + 1, 0); fullEn.assign((size_t)L + 1, (int)K + 1);
      if (env_rejected(env_add(h, k, K, L, L + 1, fullSt.data(), fullEn.data(), true))) return 1;
    }
    if ((double)h.M[(size_t)k] * p->m->S * (p->nCols + 1) > 2147483647.0) { set_error("pair " + std::to_string(k) + ": an anti-diagonal of the lattice has more than 2^31 cells"); return 1; }
  }
  if (ensure_init()) return 1;
  if (!env_upload((void **)&p->d_envStart, h.st.data(), h.st.size() * sizeof(int)) || !env_upload((void **)&p->d_envEnd, h.en.data(), h.en.size() * sizeof(int)) ||
      !env_upload((void **)&p->d_envOff, h.off.data(), h.off.size() * sizeof(long long)) || !env_upload((void **)&p->d_diagLo, h.lo.data(), h.lo.size() * sizeof(int)) ||
      !env_upload((void **)&p->d_diagCnt, h.cnt.data(), h.cnt.size() * sizeof(int)) || !env_upload((void **)&p->d_colStart, h.cSt.data(), h.cSt.size() * sizeof(int)) ||
      !env_upload((void **)&p->d_colEnd, h.cEn.data(), h.cEn.size() * sizeof(int)) || !env_upload((void **)&p->d_colOff, h.cOff.data(), h.cOff.size() * sizeof(long long)) ||
      !hip_ok(hipStreamSynchronize(g_stream), "H2D pair envelopes")) { pt_env_free(p); return 1; }
  p->envBase.swap(h.envBase); p->diagBase.swap(h.diagBase); p->colBase.swap(h.colBase); p->envCells.swap(h.envCells); p->envM.swap(h.M);
  p->hasEnv = true;
  return 0;
}

// Forward (MB_FORWARD) or Viterbi scores without paths (MB_VITERBI); mat: through the materialised lattice
static int two_profile_scores(mb_profile_twos *p, int mode, bool mat, double *loglike) {
  std::vector<Chunk> chunks;
  if (!lattice_chunks(p->n, "pair", [&](long long k) { return (mat ? pt_cell_bytes(p, k) : 0.0) + pt_ring_bytes(p, k, !mat); }, chunks)) return 1;
  SmBuf<double> d_ll;
  MB_HIP(d_ll.alloc(p->n));
  int rc = for_chunks<TwoProfPlan>(chunks, pt_build(p, !mat), [&](const Chunk &c, TwoProfPlan &pl, Timer &tm) {
    double *pool = nullptr, *scratch = nullptr;
    if (mat && !(pool = ws_array<double>(0, pl.cells))) return 1;
    if (pl.ring && !(scratch = (double *)ws_get(1, (size_t)pl.ring * sizeof(double)))) return 1;
    Timed t(tm, 1);
    return pt_fwd(p, mode, mat, pl, c.p1 - c.p0, pool, scratch, d_ll + c.p0);
  });
  if (!rc) rc = fetch_loglike(loglike, d_ll, p->n);
  g_last_kernel = pt_fwd_name(p, mode, mat);
  return rc;
}

// the line blocks of k_profile_two_rowpost on one axis of the pair that has most among [p0, p1)
static long long pt_rowpost_groups(const mb_profile_twos *p, long long p0, long long p1, int axis, int tabMax) {
  const long long NC = (axis ? p->m->nIn : p->m->nOut) + 1;
  auto lines = [&](long long k) { return axis ? pt_in(p, k) : pt_rows(p, k); };
  return rowpost_groups(p0, p1, lines, [&](long long k) {
    return profile_pair_rowpost_rows(pt_ncells(p, k), p->m->S, (int)lines(k), (int)NC, tabMax);
  });
}
// the same for k_profile_two_merge_rowpost: lines of (K + 1)(nCols + 1) S items and nCols + 1 bins on axis 0, of (L + 1)(nCols + 1) S
// items and nIn + 1 bins on axis 1
static long long pt_merge_rowpost_groups(const mb_profile_twos *p, long long p0, long long p1, int axis, int tabMax) {
  const long long NC = axis ? p->m->nIn + 1 : p->nCols + 1;
  auto lines = [&](long long k) { return axis ? pt_in(p, k) : pt_rows(p, k); };
  return rowpost_groups(p0, p1, lines, [&](long long k) {
    return profile_pair_rowpost_rows(pt_ncells(p, k) * (p->nCols + 1), p->m->S, (int)lines(k), (int)NC, tabMax);
  });
}

}  // namespace mb

extern "C" {

// nCols > 0: CTC-merged output profiles, rows of nCols + 1 doubles and the column map colTok (checked by the caller)
static mb_profile_twos *profile_twos_create(mb_machine *m, int64_t nPairs, const double *logA, const int64_t *inOff, const double *logB, const int64_t *rowOff,
                                            int32_t nCols, const int32_t *colTok) {
  if (!m || nPairs < 0 || (nPairs > 0 && (!rowOff || !inOff))) { set_error("null argument"); return nullptr; }
  if (!m->nIn) { set_error("two-profile sweeps need a machine with an input alphabet"); return nullptr; }
  if (ensure_init()) return nullptr;
  mb_profile_twos *p = new mb_profile_twos();
  p->m = m; p->n = nPairs; p->nCols = nCols;
  p->rowOff.assign((size_t)nPairs + 1, 0); p->inOff.assign((size_t)nPairs + 1, 0);
  for (long long k = 0; k < nPairs; ++k) {
    const long long L = rowOff[k + 1] - rowOff[k], K = inOff[k + 1] - inOff[k];
    if (L < 0 || L > 0x3fffffff || K < 0 || K > 0x3fffffff) { set_error("bad pair offsets"); delete p; return nullptr; }
    if ((double)(std::min(K, L) + 1) * m->S * (nCols + 1) > 2147483647.0) { set_error("pair " + std::to_string(k) + ": an anti-diagonal of the lattice has more than 2^31 cells"); delete p; return nullptr; }
    p->rowOff[(size_t)k + 1] = p->rowOff[(size_t)k] + L;
    p->inOff[(size_t)k + 1] = p->inOff[(size_t)k] + K;
  }
  p->totalRows = p->rowOff.back(); p->totalIn = p->inOff.back();
  const long long C = pt_width(p), CA = m->nIn + 1, nb = p->totalRows * C, na = p->totalIn * CA;
  const double *b0 = logB ? logB + (nPairs ? rowOff[0] * C : 0) : nullptr;
  const double *a0 = logA ? logA + (nPairs ? inOff[0] * CA : 0) : nullptr;
  if ((nb && !b0) || (na && !a0)) { set_error("null argument"); delete p; return nullptr; }
  if (!profile_values_ok(a0, na) || !profile_values_ok(b0, nb)) { delete p; return nullptr; }
  if (!hip_ok(hipMalloc((void **)&p->d_logB, (size_t)std::max<long long>(nb, 1) * sizeof(double)), "hipMalloc(output profiles)") ||
      !hip_ok(hipMalloc((void **)&p->d_logA, (size_t)std::max<long long>(na, 1) * sizeof(double)), "hipMalloc(input profiles)")) { mb_profile_twos_destroy(p); return nullptr; }
  if (nCols && (!hip_ok(hipMalloc((void **)&p->d_colTok, (size_t)nCols * sizeof(int)), "hipMalloc(column map)") ||
                !hip_ok(hipMemcpyAsync(p->d_colTok, colTok, (size_t)nCols * sizeof(int), hipMemcpyHostToDevice, g_stream), "H2D column map"))) { mb_profile_twos_destroy(p); return nullptr; }
  if ((nb && h2d_large(p->d_logB, b0, (size_t)nb * sizeof(double))) || (na && h2d_large(p->d_logA, a0, (size_t)na * sizeof(double))) ||
      !hip_ok(hipStreamSynchronize(g_stream), "H2D profiles")) { mb_profile_twos_destroy(p); return nullptr; }
  return p;
}

mb_profile_twos *mb_profile_twos_create(mb_machine *m, int64_t nPairs, const double *logA, const int64_t *inOff, const double *logB, const int64_t *rowOff) {
  ApiGuard guard;
  return profile_twos_create(m, nPairs, logA, inOff, logB, rowOff, 0, nullptr);
}

mb_profile_twos *mb_profile_twos_create_merged(mb_machine *m, int64_t nPairs, const double *logA, const int64_t *inOff, const double *logB, const int64_t *rowOff,
                                               int32_t nCols, const int32_t *colTok) {
  ApiGuard guard;
  if (!merge_map_ok(m, nCols, colTok)) return nullptr;
  return profile_twos_create(m, nPairs, logA, inOff, logB, rowOff, nCols, colTok);
}

void mb_profile_twos_destroy(mb_profile_twos *p) {
  ApiGuard guard;
  if (!p) return;
  if (p->d_logA) (void)hipFree(p->d_logA);
  if (p->d_logB) (void)hipFree(p->d_logB);
  if (p->d_colTok) (void)hipFree(p->d_colTok);
  pt_env_free(p);
  delete p;
}

int mb_profile_twos_set_envelopes(mb_profile_twos *p, const int64_t *envOff, const int32_t *inStart, const int32_t *inEnd) {
  ApiGuard guard;
  if (!p) { set_error("null argument"); return 1; }
  return profile_twos_set_envelopes(p, false, envOff, inStart, inEnd);
}

int mb_profile_twos_set_envelopes_merged(mb_profile_twos *p, const int64_t *envOff, const int32_t *inStart, const int32_t *inEnd) {
  ApiGuard guard;
  if (!p) { set_error("null argument"); return 1; }
  return profile_twos_set_envelopes(p, true, envOff, inStart, inEnd);
}

int64_t mb_profile_twos_cells(const mb_profile_twos *p) {
  if (!p) return 0;
  long long c = 0;
  for (long long k = 0; k < p->n; ++k) c += pt_cells(p, k);
  return c;
}

int mb_profile_twos_forward(mb_profile_twos *p, int flags, double *loglike) {
  ApiGuard guard;
  if (!p || (!loglike && p->n)) { set_error("null argument"); return 1; }
  if (flags != MB_ROLLING && flags != MB_MATERIALISE) { set_error("unknown flags"); return 1; }
  g_last_ms = 0.0; g_last_launches = 0;
  return two_profile_scores(p, MB_FORWARD, flags == MB_MATERIALISE, loglike);
}

int mb_profile_twos_viterbi(mb_profile_twos *p, double *loglike, int64_t *pathOff, uint32_t *pathEdges, int32_t *pathRow, int32_t *pathInRow, int64_t pathCap) {
  ApiGuard guard;
  if (!p || (!loglike && p->n)) { set_error("null argument"); return 1; }
  g_last_ms = 0.0; g_last_launches = 0;
  if (!pathEdges || !pathOff) return two_profile_scores(p, MB_VITERBI, false, loglike);
  long long need = 0;
  for (long long k = 0; k < p->n; ++k) need += pt_path_bound(p, k);
  if (pathCap < need) { set_error("pathCap too small for the Viterbi paths: " + std::to_string((long long)pathCap) + " entries, the path bounds of the pairs sum to " + std::to_string(need)); return 1; }
  std::vector<Chunk> chunks;
  if (!lattice_chunks(p->n, "pair", [&](long long k) { return pt_cell_bytes(p, k) + pt_ring_bytes(p, k, false) + 12.0 * pt_path_bound(p, k); }, chunks)) return 1;
  SmBuf<double> d_ll;
  SmBuf<long long> d_len;
  MB_HIP(d_ll.alloc(p->n));
  if (!hip_ok(d_len.alloc(p->n), "hipMalloc(path lengths)")) return 1;
  PathSink out{pathOff, pathEdges, pathRow, pathInRow, pathCap, "pair", [&](long long k) { return pt_path_bound(p, k); }};
  pathOff[0] = 0;
  int rc = for_chunks<TwoProfPlan>(chunks, pt_build(p, false), [&](const Chunk &c, TwoProfPlan &pl, Timer &tm) {
    const long long np = c.p1 - c.p0;
    double *pool = ws_array<double>(0, pl.cells);
    uint32_t *d_e = ws_array<uint32_t>(3, pl.paths);
    int32_t *d_r = ws_array<int32_t>(4, pl.paths);
    int32_t *d_i = ws_array<int32_t>(5, pl.paths);
    double *scratch = pl.ring ? (double *)ws_get(1, (size_t)pl.ring * sizeof(double)) : nullptr;
    if (!pool || !d_e || !d_r || !d_i || (pl.ring && !scratch)) return 1;
    {
      Timed t(tm, 1);
      if (pt_fwd_mat(p, MB_VITERBI, pl, np, pool, scratch, d_ll + c.p0) || pt_traceback(p, pl, np, pool, d_e, d_r, d_i, d_len + c.p0)) return 1;
    }
    return unpack_paths(out, c.p0, np, pl.paths, nullptr, d_len + c.p0, d_e, d_r, d_i);
  });
  if (!rc) rc = fetch_loglike(loglike, d_ll, p->n);
  g_last_kernel = pt_fwd_name(p, MB_VITERBI, true);
  return rc;
}

// Per chunk one materialised Forward launch and one sample launch.  The pairs of a chunk run in their order (TwoProfPlan), so the
// index in the object of the pair a lane serves is c.p0 plus its place in the chunk.
int mb_profile_twos_sample(mb_profile_twos *p, int64_t nSamples, uint64_t seed, double *loglike, int64_t *pathOff, uint32_t *pathEdges, int32_t *pathRow,
                           int32_t *pathInRow, double *pathLogProb, int64_t pathCap) {
  ApiGuard guard;
  g_last_ms = 0.0; g_last_launches = 0;
  if (!p || !pathOff || !pathEdges) { set_error("null argument"); return 1; }
  if (p->nCols) { set_error("sampling takes plain profiles"); return 1; }
  if (nSamples < 1) { set_error("nSamples must be at least 1"); return 1; }
  double need = 0.0;
  for (long long k = 0; k < p->n; ++k) need += (double)pt_path_bound(p, k);
  need *= (double)nSamples;
  if ((double)pathCap < need) {
    set_error("pathCap too small for the sampled paths: " + std::to_string((long long)pathCap) + " entries, nSamples times the path bounds of the pairs is " +
              std::to_string((long long)need));
    return 1;
  }
  // a pair costs its lattice, and per sample a path slot (an edge and both rows per entry), a length and a log probability
  std::vector<Chunk> chunks;
  auto bytes = [&](long long k) { return pt_cell_bytes(p, k) + pt_ring_bytes(p, k, false) + (double)nSamples * (12.0 * (double)pt_path_bound(p, k) + 16.0); };
  if (!lattice_chunks(p->n, "pair", bytes, chunks)) return 1;
  for (const Chunk &c : chunks)
    if ((double)(c.p1 - c.p0) * (double)nSamples > 2147483647.0) { set_error("too many samples in one chunk: pairs times nSamples exceeds 2^31 - 1 lanes"); return 1; }
  SmBuf<double> d_ll;
  MB_HIP(d_ll.alloc(p->n));
  const int nS = (int)nSamples;
  SampleSink out{pathOff, pathEdges, pathRow, pathInRow, pathLogProb, nSamples, [&](long long k) { return pt_path_bound(p, k); }};
  pathOff[0] = 0;
  int rc = for_chunks<TwoProfPlan>(chunks, pt_build(p, false), [&](const Chunk &c, TwoProfPlan &pl, Timer &tm) {
    const long long np = c.p1 - c.p0, lanes = np * nS, entries = pl.paths * nS;
    double *pool = ws_array<double>(0, pl.cells);
    uint32_t *d_e = ws_array<uint32_t>(3, entries);
    int32_t *d_r = ws_array<int32_t>(4, entries);
    int32_t *d_i = ws_array<int32_t>(5, entries);
    long long *d_len = ws_array<long long>(6, lanes);
    double *d_lq = ws_array<double>(7, lanes);
    if (!pool || !d_e || !d_r || !d_i || !d_len || !d_lq) return 1;
    {
      Timed t(tm, 1);
      if (pt_fwd_mat(p, MB_FORWARD, pl, np, pool, nullptr, d_ll + c.p0)) return 1;
      if (p->hasEnv ? launch_profile_two_sample(p->m, pl.e.p, pt_env_tables(p), (int)np, nS, c.p0, seed, p->d_logA, p->d_logB, pool, d_e, d_r, d_i, d_len, d_lq, g_stream)
                    : launch_profile_two_sample(p->m, pl.d.p, (int)np, nS, c.p0, seed, p->d_logA, p->d_logB, pool, d_e, d_r, d_i, d_len, d_lq, g_stream)) return 1;
    }
    return unpack_samples(out, c.p0, np, entries, nullptr, d_len, d_lq, d_e, d_r, d_i);
  });
  if (!rc && loglike) rc = fetch_loglike(loglike, d_ll, p->n);
  g_last_kernel = p->hasEnv ? "k_profile_two_env_sample" : "k_profile_two_sample";
  return rc;
}

int mb_profile_twos_counts(mb_profile_twos *p, double *counts, double *loglikeSum, double *loglike) {
  ApiGuard guard;
  if (!p || !counts) { set_error("null argument"); return 1; }
  g_last_ms = 0.0; g_last_launches = 0;
  latch_deterministic();
  const long long nT = p->m->nTrans;
  std::vector<Chunk> chunks;
  if (!lattice_chunks(p->n, "pair", [&](long long k) { return 2.0 * pt_cell_bytes(p, k) + pt_ring_bytes(p, k, false); }, chunks)) return 1;   // the Forward and the Backward lattice
  SmBuf<double> d_ll, d_bll, d_cc;
  MB_HIP(d_ll.alloc(p->n));
  if (!hip_ok(d_bll.alloc(p->n), "hipMalloc(loglike)") || !hip_ok(d_cc.alloc(nT), "hipMalloc(counts)")) return 1;
  CountSum sum(nT);
  int rc = for_chunks<TwoProfPlan>(chunks, pt_build(p, false), [&](const Chunk &c, TwoProfPlan &pl, Timer &tm) {
    const long long np = c.p1 - c.p0;
    double *fwd = ws_array<double>(0, pl.cells);
    double *bwd = ws_array<double>(1, pl.cells);
    double *scratch = pl.ring ? (double *)ws_get(2, (size_t)pl.ring * sizeof(double)) : nullptr;
    if (!fwd || !bwd || (pl.ring && !scratch)) return 1;
    const int groups = count_groups(c.p0, c.p1, [&](long long k) { return pt_cells(p, k) / 3; });
    if (np * groups > 0x7fffffff) { set_error("too many pairs in one chunk"); return 1; }
    {
      Timed t(tm, 1);
      // (merged: the Backward's ring follows the Forward's on the stream, one scratch buffer serves both)
      if (pt_fwd_mat(p, MB_FORWARD, pl, np, fwd, scratch, d_ll + c.p0) || pt_bwd(p, pl, np, bwd, scratch, d_bll + c.p0)) return 1;
      if (nT && !hip_ok(hipMemsetAsync(d_cc, 0, (size_t)nT * sizeof(double), g_stream), "memset(counts)")) return 1;
      if (pt_counts(p, pl, np, groups, fwd, bwd, d_cc)) return 1;
    }
    return sum.add(d_cc, g_deterministic);
  });
  std::vector<double> hll((size_t)p->n);
  if (!rc) rc = fetch_loglike(hll.data(), d_ll, p->n);
  g_last_kernel = pt_name(p, "k_profile_two_counts", "k_profile_two_env_counts", "k_profile_two_merge_counts", "k_profile_two_merge_env_counts");
  if (rc) return rc;
  sum.finish(hll, counts, loglikeSum, loglike);
  return 0;
}

int mb_profile_twos_row_posteriors(mb_profile_twos *p, double *postA, double *postB, double *loglike) {
  ApiGuard guard;
  if (!p) { set_error("null argument"); return 1; }
  if (p->nCols) { set_error("row posteriors take plain profiles"); return 1; }
  g_last_ms = 0.0; g_last_launches = 0;
  latch_deterministic();
  const mb_machine *m = p->m;
  const long long C = m->nOut + 1, CA = m->nIn + 1, nb = postB ? p->totalRows * C : 0, na = postA ? p->totalIn * CA : 0;
  const int tabMax = rowpost_table();
  std::vector<Chunk> chunks;
  auto bytes = [&](long long k) { return 2.0 * pt_cell_bytes(p, k) + 8.0 * (double)(pt_rows(p, k) * C + pt_in(p, k) * CA); };   // both lattices and the pair's bins of both tables
  if (!lattice_chunks(p->n, "pair", bytes, chunks)) return 1;
  SmBuf<double> d_ll, d_bll, d_pa, d_pb;
  MB_HIP(d_ll.alloc(p->n));
  if (!hip_ok(d_bll.alloc(p->n), "hipMalloc(loglike)") || !hip_ok(d_pa.alloc(na), "hipMalloc(row posteriors)") ||
      !hip_ok(d_pb.alloc(nb), "hipMalloc(row posteriors)")) return 1;
  int rc = for_chunks<TwoProfPlan>(chunks, pt_build(p, false), [&](const Chunk &c, TwoProfPlan &pl, Timer &tm) {
    const long long np = c.p1 - c.p0;
    double *fwd = ws_array<double>(0, pl.cells);
    double *bwd = ws_array<double>(1, pl.cells);
    if (!fwd || !bwd) return 1;
    const long long groupsB = pt_rowpost_groups(p, c.p0, c.p1, 0, tabMax), groupsA = pt_rowpost_groups(p, c.p0, c.p1, 1, tabMax);
    if (np * std::max(groupsA, groupsB) > 0x7fffffff) { set_error("too many pairs in one chunk"); return 1; }
    {
      Timed t(tm, 1);
      if (pt_fwd_mat(p, MB_FORWARD, pl, np, fwd, nullptr, d_ll + c.p0) || pt_bwd(p, pl, np, bwd, nullptr, d_bll + c.p0)) return 1;
      if (postB && pt_rowpost(p, 0, pl, np, (int)groupsB, tabMax, fwd, bwd, d_pb)) return 1;
      if (postA && pt_rowpost(p, 1, pl, np, (int)groupsA, tabMax, fwd, bwd, d_pa)) return 1;
    }
    return hip_ok(hipStreamSynchronize(g_stream), "row posteriors") ? 0 : 1;      // (the next chunk takes the lattices over)
  });
  if (!rc) rc = fetch_posteriors(postA, d_pa, na);
  if (!rc) rc = fetch_posteriors(postB, d_pb, nb);
  if (!rc && loglike) rc = fetch_loglike(loglike, d_ll, p->n);
  g_last_kernel = p->hasEnv ? "k_profile_two_env_rowpost" : "k_profile_two_rowpost";
  return rc;
}

// The merged object's own entry: mb_profile_twos_counts on a merged object chunk for chunk -- the materialised merged Forward and
// Backward, whose X / T rings share one scratch buffer -- then the flat k_profile_two_merge_rowpost over the two lattices, once per
// table that was asked for.
int mb_profile_twos_row_posteriors_merged(mb_profile_twos *p, double *postA, double *postB, double *loglike) {
  ApiGuard guard;
  if (!p) { set_error("null argument"); return 1; }
  if (!p->nCols) { set_error("merged row posteriors take merged profiles"); return 1; }
  g_last_ms = 0.0; g_last_launches = 0;
  latch_deterministic();
  const long long PL = p->nCols + 1, CA = p->m->nIn + 1, nb = postB ? p->totalRows * PL : 0, na = postA ? p->totalIn * CA : 0;
  const int tabMax = rowpost_table();
  std::vector<Chunk> chunks;
  auto bytes = [&](long long k) {      // both lattices, the X / T ring and the pair's bins of both tables
    return 2.0 * pt_cell_bytes(p, k) + pt_ring_bytes(p, k, false) + 8.0 * (double)(pt_rows(p, k) * PL + pt_in(p, k) * CA);
  };
  if (!lattice_chunks(p->n, "pair", bytes, chunks)) return 1;
  SmBuf<double> d_ll, d_bll, d_pa, d_pb;
  MB_HIP(d_ll.alloc(p->n));
  if (!hip_ok(d_bll.alloc(p->n), "hipMalloc(loglike)") || !hip_ok(d_pa.alloc(na), "hipMalloc(row posteriors)") ||
      !hip_ok(d_pb.alloc(nb), "hipMalloc(row posteriors)")) return 1;
  int rc = for_chunks<TwoProfPlan>(chunks, pt_build(p, false), [&](const Chunk &c, TwoProfPlan &pl, Timer &tm) {
    const long long np = c.p1 - c.p0;
    double *fwd = ws_array<double>(0, pl.cells);
    double *bwd = ws_array<double>(1, pl.cells);
    double *scratch = pl.ring ? (double *)ws_get(2, (size_t)pl.ring * sizeof(double)) : nullptr;
    if (!fwd || !bwd || (pl.ring && !scratch)) return 1;
    const long long groupsB = pt_merge_rowpost_groups(p, c.p0, c.p1, 0, tabMax), groupsA = pt_merge_rowpost_groups(p, c.p0, c.p1, 1, tabMax);
    if (np * std::max(groupsA, groupsB) > 0x7fffffff) { set_error("too many pairs in one chunk"); return 1; }
    {
      Timed t(tm, 1);
      if (pt_fwd_mat(p, MB_FORWARD, pl, np, fwd, scratch, d_ll + c.p0) || pt_bwd(p, pl, np, bwd, scratch, d_bll + c.p0)) return 1;
      if (postB && pt_merge_rowpost(p, 0, pl, np, (int)groupsB, tabMax, fwd, bwd, d_ll + c.p0, d_pb)) return 1;
      if (postA && pt_merge_rowpost(p, 1, pl, np, (int)groupsA, tabMax, fwd, bwd, d_ll + c.p0, d_pa)) return 1;
    }
    return hip_ok(hipStreamSynchronize(g_stream), "row posteriors") ? 0 : 1;      // (the next chunk takes the lattices over)
  });
  if (!rc) rc = fetch_posteriors(postA, d_pa, na);
  if (!rc) rc = fetch_posteriors(postB, d_pb, nb);
  if (!rc && loglike) rc = fetch_loglike(loglike, d_ll, p->n);
  g_last_kernel = p->hasEnv ? "k_profile_two_merge_env_rowpost" : "k_profile_two_merge_rowpost";
  return rc;
}

int mb_profile_twos_set_rows(mb_profile_twos *p, const double *logA, const double *logB) {
  ApiGuard guard;
  if (!p) { set_error("null argument"); return 1; }
  const long long na = logA ? p->totalIn * (p->m->nIn + 1) : 0, nb = logB ? p->totalRows * pt_width(p) : 0;
  if (!profile_values_ok(logA, na) || !profile_values_ok(logB, nb)) return 1;      // (before either copy: a refused table leaves both in effect)
  if ((na && h2d_large(p->d_logA, logA, (size_t)na * sizeof(double))) || (nb && h2d_large(p->d_logB, logB, (size_t)nb * sizeof(double)))) return 1;
  return hip_ok(hipStreamSynchronize(g_stream), "H2D profiles") ? 0 : 1;
}

static int profile_two_fill(mb_machine *m, int mode, const double *logA, int64_t nIn, const double *logB, int64_t nRows, int32_t nCols,
                            const int32_t *colTok, const int32_t *envStart, const int32_t *envEnd, double *cellsOut) {
  if (!m || !cellsOut || nRows < 0 || nIn < 0 || (nRows && !logB) || (nIn && !logA)) { set_error("null argument"); return 1; }
  if (!fill_mode_ok(mode)) return 1;
  g_last_ms = 0.0; g_last_launches = 0;
  const int64_t rOff[2] = {0, nRows}, iOff[2] = {0, nIn};
  mb_profile_twos *p = profile_twos_create(m, 1, logA, iOff, logB, rOff, nCols, colTok);
  if (!p) return 1;
  const bool env = envStart && envEnd;
  if (env) {
    const int64_t eOff[2] = {0, nRows + 1};
    if (profile_twos_set_envelopes(p, nCols > 0, eOff, envStart, envEnd)) { mb_profile_twos_destroy(p); return 1; }
  }
  std::vector<Chunk> chunks;
  if (!lattice_chunks(1, "pair", [&](long long k) { return pt_cell_bytes(p, k) + pt_ring_bytes(p, k, false); }, chunks)) { mb_profile_twos_destroy(p); return 1; }
  int rc;
  {
    TwoProfPlan pl;
    rc = two_profile_descs(p, 0, 1, false, pl);
    std::vector<double> compact(!rc && env ? (size_t)pl.cells : 0);      // under an envelope the lattice comes back compact
    if (!rc) rc = fill_one(pl.cells, pl.ring, env ? compact.data() : cellsOut, [&](double *pool, double *scratch, double *d_ll) {
      return mode == MB_BACKWARD ? pt_bwd(p, pl, 1, pool, scratch, d_ll) : pt_fwd_mat(p, mode, pl, 1, pool, scratch, d_ll);
    });
    if (!rc && env) {      // the compact lattice into the full rectangle, -inf outside the envelope
      const size_t cellD = 3 * (size_t)m->S * (size_t)(nCols + 1);
      std::fill(cellsOut, cellsOut + (size_t)(nIn + 1) * (size_t)(nRows + 1) * cellD, -INFINITY);
      size_t at = 0;
      for (int64_t r = 0; r <= nRows; ++r)
        for (int64_t i = envStart[r]; i < envEnd[r]; ++i, at += cellD)
          std::memcpy(cellsOut + ((size_t)i * (size_t)(nRows + 1) + (size_t)r) * cellD, compact.data() + at, cellD * sizeof(double));
    }
  }
  g_last_kernel = mode == MB_BACKWARD ? pt_name(p, "k_profile_two_bwd", "k_profile_two_env_bwd", "k_profile_two_merge_bwd", "k_profile_two_merge_env_bwd") : pt_fwd_name(p, mode, true);
  mb_profile_twos_destroy(p);
  return rc;
}

int mb_profile_two_fill(mb_machine *m, int mode, const double *logA, int64_t nIn, const double *logB, int64_t nRows, double *cellsOut) {
  ApiGuard guard;
  return profile_two_fill(m, mode, logA, nIn, logB, nRows, 0, nullptr, nullptr, nullptr, cellsOut);
}

int mb_profile_two_fill_merged(mb_machine *m, int mode, const double *logA, int64_t nIn, const double *logB, int64_t nRows, int32_t nCols,
                               const int32_t *colTok, double *cellsOut) {
  ApiGuard guard;
  if (!merge_map_ok(m, nCols, colTok)) return 1;
  return profile_two_fill(m, mode, logA, nIn, logB, nRows, nCols, colTok, nullptr, nullptr, cellsOut);
}

int mb_profile_two_fill_env(mb_machine *m, int mode, const double *logA, int64_t nIn, const double *logB, int64_t nRows, const int32_t *envStart,
                            const int32_t *envEnd, double *cellsOut) {
  ApiGuard guard;
  if ((envStart == nullptr) != (envEnd == nullptr)) { set_error("null argument"); return 1; }
  return profile_two_fill(m, mode, logA, nIn, logB, nRows, 0, nullptr, envStart, envEnd, cellsOut);
}

int mb_profile_two_fill_merged_env(mb_machine *m, int mode, const double *logA, int64_t nIn, const double *logB, int64_t nRows, int32_t nCols,
                                   const int32_t *colTok, const int32_t *envStart, const int32_t *envEnd, double *cellsOut) {
  ApiGuard guard;
  if (!merge_map_ok(m, nCols, colTok)) return 1;
  if ((envStart == nullptr) != (envEnd == nullptr)) { set_error("null argument"); return 1; }
  return profile_two_fill(m, mode, logA, nIn, logB, nRows, nCols, colTok, envStart, envEnd, cellsOut);
}

}  // extern "C"
