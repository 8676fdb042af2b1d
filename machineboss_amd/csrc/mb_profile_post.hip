// mb_profile_post.hip -- row posteriors of the one-tape profile sweeps, plain and CTC-merged (docs/profile_tapes.md, "Row posteriors
// of one-tape profiles"): post[(rowBase + r) * C + x] = the posterior probability that row r of the profile was consumed as column x
// (0: the blank), the gradient of the log-likelihood in P[r][x].  The terms are those of k_profile_bwd / k_profile_merge_bwd,
// regrouped by (row, column), read off the materialised Forward and Backward lattices:
//
//   plain    post[r][0] = sum_s exp((N_F[r][s] - LL) + (P[r][0] + NB[r+1][s]))
//            post[r][o] = sum_{t: s->d, in = eps, out = o} exp((W_F[r][s] - LL) + ((w_t + P[r][o]) + NB[r+1][d]))
//   merged   post[r][0] = sum_p sum_s exp((N_F[r][p][s] - LL) + (P[r][0] + NB[r+1][0][s]))
//            post[r][c] = sum_s exp((N_F[r][c][s] - LL) + (P[r][c] + NB[r+1][c][s]))                                  (the repeat)
//                       + sum_{k != c} sum_{t: s->d, out = colTok[c]} exp((W_F[r][k][s] - LL) + ((w_t + P[r][c]) + NB[r+1][c][d]))
//
// The sweeps that fill the lattices are serial in the rows; this is not: a flat grid over all rows of all profiles.  The scheme is the
// one of k_profile_pair_rowpost (mb_profile_pair.hip).  The work items are (row, state) -- merged: (row, plane, state) -- in that
// order, and a workgroup owns whole rows: blocks of profile_pair_rowpost_rows rows, dealt round robin to the profile's groups.  A lane
// sums its terms of one column in a register, one CSR row of its state in CSR order; where all 64 lanes of the wavefront hold items
// of one row the lane sums are reduced across the lanes and one lane adds the result to the workgroup's LDS table (rows of the block
// x C), else every lane adds its own (rowpost_add, mb_profile_common.h).  The table is then stored with plain stores: every bin has
// one writing workgroup, so there is no global atomic and nothing to clear beforehand.  A row of more than tabMax columns is summed in
// its global bins instead, cleared by the workgroup that owns it.  A profile whose likelihood is -inf gets zeros by the same stores.
// A merged item (r, k, s) adds the blank term, at column k >= 1 the repeat term and at every other column the emissions out of plane
// k: the sum over k != c runs over the items, the exclusion vector of the Forward sweep is not needed.
// det: a lane sum is turned into 64-bit fixed point at 2^-36 (mb_internal.h) before it meets another; post then holds the integers.
#include "mb_profile_common.h"
#include "mb_profile_merge.h"
#include "mb_profile_pair.h"
#include "mb_profile_post.h"

namespace mb {

template <bool MERGED>
__global__ __launch_bounds__(ROWPOST_THREADS) void k_profile_rowpost(DevMachine m, MergeMap mm, const ProfDesc *__restrict__ descs, int groupsPerProf,
                                                                     const double *__restrict__ logP, const double *__restrict__ fwdPool,
                                                                     const double *__restrict__ bwdPool, const double *__restrict__ loglike,
                                                                     double *post, int tabMax, int det) {
  __shared__ double ltab[ROWPOST_LDS_MAX];
  const int k = blockIdx.x / groupsPerProf, group = blockIdx.x % groupsPerProf;
  const ProfDesc pd = descs[k];
  const int S = m.S, K = m.K, PL = MERGED ? mm.nCols + 1 : 1, C = MERGED ? PL : m.nOut + 1, L = pd.nRows;
  if (L == 0) return;
  const long long PS = (long long)PL * S;
  const double *P = logP + pd.rowBase * C;
  const double *F = fwdPool + pd.cellBase, *B = bwdPool + pd.cellBase;
  const double LL = loglike[k];
  const int R = profile_pair_rowpost_rows((long long)(L + 1) * PL, S, L, C, tabMax);
  const bool useLds = C <= tabMax;
  const int lane = threadIdx.x & 63;
  for (long long rb = (long long)group * R; rb < L; rb += (long long)groupsPerProf * R) {
    const int r0 = (int)rb, r1 = (int)min((long long)L, rb + R), nBins = (r1 - r0) * C;
    double *out = post + (pd.rowBase + r0) * C;
    double *tab = useLds ? ltab : out;
    for (int e = threadIdx.x; e < nBins; e += blockDim.x) tab[e] = 0.0;      // (the fixed point's zero has the same bits)
    if (!useLds) __threadfence();
    __syncthreads();
    if (LL > -INFINITY) {
      const long long nItems = (long long)(r1 - r0) * PS;
      for (long long base = threadIdx.x - lane; base < nItems; base += blockDim.x) {      // (a wavefront stays whole in here)
        const long long idx = base + lane;
        const bool valid = idx < nItems;
        int r = r0, p = 0, s = 0;
        double f = -INFINITY, n = -INFINITY;
        if (valid) {
          const long long row = idx / PS, rem = idx - row * PS;
          r = r0 + (int)row;
          p = (int)(rem / S);
          s = (int)(rem - (long long)p * S);
          const double *Fr = F + (long long)r * 2 * PS + (long long)p * S;
          n = Fr[s] - LL;
          f = Fr[PS + s] - LL;
        }
        const bool whole = __all(valid && r == __shfl(r, 0));
        const double *Pr = P + (long long)r * C;
        const double *Nn = B + (long long)(r + 1) * 2 * PS;      // NB[r+1], plane 0
        const bool nLive = n > -INFINITY, fLive = f > -INFINITY;
        const int sRow = s * K, bin0 = (r - r0) * C;
        rowpost_add(tab, bin0, nLive ? exp(n + (Pr[0] + Nn[s])) : 0.0, whole, lane, det);
        for (int c = 1; c < C; ++c) {      // the out-edges of s that write the column's token are one CSR row
          double v = 0.0;
          if (MERGED && valid && c == p) {
            if (nLive) v = exp(n + (Pr[c] + Nn[(long long)c * S + s]));
          } else if (fLive) {
            const int tok = MERGED ? mm.colTok[c - 1] : c;
            const double pc = Pr[c];
            const double *Nd = MERGED ? Nn + (long long)c * S : Nn;
            const int a1 = m.outOff[sRow + tok + 1];
            for (int a = m.outOff[sRow + tok]; a < a1; ++a) v += exp(f + ((m.outW[a] + pc) + Nd[m.outDst[a]]));
          }
          rowpost_add(tab, bin0 + c, v, whole, lane, det);
        }
      }
    }
    __syncthreads();
    if (useLds) {
      for (int e = threadIdx.x; e < nBins; e += blockDim.x) out[e] = tab[e];
      __syncthreads();
    }
  }
}

int launch_profile_rowpost(const mb_machine *m, MergeMap mm, const ProfDesc *d, int n, int groupsPerProf, int tabMax, const double *logP,
                           const double *fwdPool, const double *bwdPool, const double *loglike, double *post, hipStream_t st) {
  if (n <= 0) return 0;
  const dim3 g((unsigned)((long long)n * groupsPerProf)), b(ROWPOST_THREADS);
  const int det = g_deterministic ? 1 : 0;
  if (mm.nCols) k_profile_rowpost<true><<<g, b, 0, st>>>(m->dev, mm, d, groupsPerProf, logP, fwdPool, bwdPool, loglike, post, tabMax, det);
  else k_profile_rowpost<false><<<g, b, 0, st>>>(m->dev, mm, d, groupsPerProf, logP, fwdPool, bwdPool, loglike, post, tabMax, det);
  return hip_ok(hipGetLastError(), mm.nCols ? "k_profile_merge_rowpost" : "k_profile_rowpost") ? 0 : 1;
}

}  // namespace mb
