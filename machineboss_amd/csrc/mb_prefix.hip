// mb_prefix.hip -- the node fill of the prefix search (src/ctc.cpp:25-88), restated in docs/decoding.md.  For a node with input
// symbol a (a root has none), parent P, output y[1..L], rows j = 0..L:
//
//   A[j][d]      = [root, j = 0, d = 0] (+) sum_{t: s->d, in = a, out = y[j]} P.seq[j-1][s] + w_t (+) sum_{t: s->d, in = a, out = eps} P.seq[j][s] + w_t
//   seq[j][d]    = A[j][d] (+) sum_{t: s->d, in = eps, out = y[j]} seq[j-1][s] + w_t (+) sum_{silent t: s->d, s < d} seq[j][s] + w_t
//   V[j-1][s]    = logsum_p prefix[j-1][p] + R[p][s]
//   prefix[j][d] = A[j][d] (+) sum_{t: s->d, any in, out = y[j]} V[j-1][s] + w_t
//   logSeqProb = seq[L][S-1],  logPrefixProb = logsum_d prefix[L][d] + R[d][S-1]
//
// One workgroup per node, lanes over states, serial over j.  Per row: the V product (lane s owns column s of R, which the host hands
// over by column with its -inf entries dropped), a barrier, one phase for A, the prefix cell and the emitting part of the seq cell
// (all of them read rows that are complete: the parent's lattice, the node's previous row, V), a barrier, then one barrier per
// silent level above 0 as k_profile_fwd does.  The product stays in log space (a maximum pass and a sum pass per column): a linear
// product under one maximum per row would drop the columns fed only by entries 745 nats below it, and a prefix probability that
// turns -inf prunes a branch of the search (docs/decoding.md).  Cells are fp64, sums the exact log-sum-exp; every cell has one
// writer and a fixed order of terms, so a fill gives the same bits from run to run.
#include <algorithm>

#include "mb_device_math.h"
#include "mb_prefix.h"

namespace mb {

static constexpr int PX_THREADS = 1024;

// log sum_p exp(row[p] + R[p][s]) over the finite entries of column s
__device__ __forceinline__ double px_column(const PrefixR &R, int s, const double *row) {
  const long long k0 = R.rOff[s], k1 = R.rOff[s + 1];
  double mx = -INFINITY;
  for (long long k = k0; k < k1; ++k) mx = dmax(mx, row[R.rIdx[k]] + R.rVal[k]);
  if (!(mx > -INFINITY)) return -INFINITY;
  double sum = 0.0;
  for (long long k = k0; k < k1; ++k) sum += exp((row[R.rIdx[k]] + R.rVal[k]) - mx);
  return mx + log(sum);
}

__global__ __launch_bounds__(PX_THREADS) void k_prefix_fill(DevMachine m, PrefixR R, const PrefixDesc *__restrict__ descs,
                                                            const int *__restrict__ outTok, double *pool, double *__restrict__ result) {
  extern __shared__ double px_V[];
  const PrefixDesc nd = descs[blockIdx.x];
  const int S = m.S, K = m.K, C = m.nOut + 1, L = nd.outLen, a = nd.inTok;
  const bool root = nd.parentBase < 0;
  const double *par = root ? nullptr : pool + nd.parentBase;
  double *cells = pool + nd.childBase;
  const int *y = outTok + nd.outBase;
  for (int j = 0; j <= L; ++j) {
    const int o = j ? y[j - 1] : 0;
    double *sq = cells + (long long)j * 2 * S, *px = sq + S;
    const double *sqPrev = sq - 2 * S, *pxPrev = sq - S;   // (read for j > 0 only)
    if (j) {
#ifdef MB_PREFIX_SKIP_PRODUCT   // timing builds only (docs/decoding.md, "Measured rates"): what a fill costs without the V product
      for (int s = threadIdx.x; s < S; s += blockDim.x) px_V[s] = pxPrev[s];
#else
      for (int s = threadIdx.x; s < S; s += blockDim.x) px_V[s] = px_column(R, s, pxPrev);
#endif
      __syncthreads();
    }
    for (int d = threadIdx.x; d < S; d += blockDim.x) {
      const int row0 = d * K;
      double A = (root && j == 0 && d == 0) ? 0.0 : -INFINITY;
      if (!root) {
        if (j) {
          const double *pq = par + (long long)(j - 1) * 2 * S;
          for (int e = m.inOff[row0 + a * C + o], e1 = m.inOff[row0 + a * C + o + 1]; e < e1; ++e) A = lse2_exact(A, pq[m.inSrc[e]] + m.inW[e]);
        }
        const double *pq = par + (long long)j * 2 * S;
        for (int e = m.inOff[row0 + a * C], e1 = m.inOff[row0 + a * C + 1]; e < e1; ++e) A = lse2_exact(A, pq[m.inSrc[e]] + m.inW[e]);
      }
      double pre = A, acc = A;
      if (j) {
        for (int i = 0; i <= m.nIn; ++i)
          for (int e = m.inOff[row0 + i * C + o], e1 = m.inOff[row0 + i * C + o + 1]; e < e1; ++e) pre = lse2_exact(pre, px_V[m.inSrc[e]] + m.inW[e]);
        for (int e = m.inOff[row0 + o], e1 = m.inOff[row0 + o + 1]; e < e1; ++e) acc = lse2_exact(acc, sqPrev[m.inSrc[e]] + m.inW[e]);
      }
      px[d] = pre;
      sq[d] = acc;
    }
    __syncthreads();
    for (int lev = 1; lev < m.nLevF; ++lev) {          // level 0 has no silent edge coming in: its cells are final
      const int l0 = m.levFOff[lev], ns = m.levFOff[lev + 1] - l0;
      for (int k = threadIdx.x; k < ns; k += blockDim.x) {
        const int q = m.levFState[l0 + k];
        double acc = sq[q];
        for (int e = m.inOff[q * K], e1 = m.inOff[q * K + 1]; e < e1; ++e) {
          const int s = (int)m.inSrc[e];
          if (s >= q) continue;                         // as the token sweeps: a silent self-loop never fires
          acc = lse2_exact(acc, sq[s] + m.inW[e]);
        }
        sq[q] = acc;
      }
      __syncthreads();
    }
  }
  if (threadIdx.x == 0) {
    const double *last = cells + (long long)L * 2 * S;
    result[2 * blockIdx.x] = last[S - 1];
    result[2 * blockIdx.x + 1] = px_column(R, S - 1, last + S);
  }
}

int launch_prefix_fill(const mb_machine *m, const PrefixR &R, const PrefixDesc *d, int n, const int *outTok, double *pool,
                       double *result, hipStream_t st) {
  if (n <= 0) return 0;
  const size_t lds = (size_t)m->S * sizeof(double);
  static size_t ldsAllowed = 64 * 1024;      // beyond the default the kernel must be told; asked for once, and only when a machine needs it
  if (lds > ldsAllowed) {
    if (!hip_ok(hipFuncSetAttribute((const void *)&k_prefix_fill, hipFuncAttributeMaxDynamicSharedMemorySize, PREFIX_MAX_STATES * (int)sizeof(double)),
                "k_prefix_fill: raising the LDS limit for a machine of more than 8192 states")) return 1;
    ldsAllowed = (size_t)PREFIX_MAX_STATES * sizeof(double);
  }
  const int threads = std::min(PX_THREADS, std::max(64, (m->S + 63) / 64 * 64));
  k_prefix_fill<<<dim3(n), dim3(threads), lds, st>>>(m->dev, R, d, outTok, pool, result);
  return hip_ok(hipGetLastError(), "k_prefix_fill") ? 0 : 1;
}

// The same node against a PROFILE P[0..L) (rows of nOut + 1 log weights, column 0 the blank) in place of y: the token search on
// compose(M, profile recogniser) with an empty output, swept over rows r = 0..L and M's own states (docs/decoding.md).  As in
// k_profile_fwd a row has two stages: N, the mass that has arrived at the row -- only there may the blank fire -- and W, the
// mass after M's output-less moves; the composition fixes that order (the recogniser waits), so a blank and an output-less move
// are not counted in both orders.
//
//   An[r][d] = [root, r = 0, d = 0] (+) sum_{t: s->d, in = a, out = o} Pa.W[r-1][s] + w_t + P[r-1][o]
//   Aw[r][d] = sum_{t: s->d, in = a, out = eps} Pa.W[r][s] + w_t
//   N[r][d]  = An[r][d] (+) (N[r-1][d] + P[r-1][0]) (+) sum_{t: s->d, in = eps, out = o} W[r-1][s] + w_t + P[r-1][o]
//   W[r][d]  = Aw[r][d] (+) N[r][d] (+) sum_{silent t: s->d, s < d} W[r][s] + w_t
//   Xn[r][d] = An[r][d] (+) (Xn[r-1][d] + P[r-1][0]) (+) sum_{t: s->d, any in, out = o} Y[r-1][s] + w_t + P[r-1][o]
//   X[r][d]  = Aw[r][d] (+) Xn[r][d]
//   Y[r][s]  = logsum_p X[r][p] + R[p][s];   logSeqProb = W[L][S-1],  logPrefixProb = Y[L][S-1]
//
// Layer 0 of a slot is W, layer 1 is X.  The phases of a row are those of k_prefix_fill: the Y product into LDS, the middle phase,
// the silent levels.  N and Xn are read by the next row only, and only by the lane that wrote them: they live in LDS beside Y
// (3 S doubles in all) and are not stored.  The row's nOut + 1 weights go into LDS while the product runs, one load each per row;
// a symbol of weight -inf is skipped as a whole (the branch is uniform over the workgroup).  The terms of a cell keep one order
// -- the node's own symbol, the blank, then the edges by output symbol -- so a fill gives the same bits from run to run.
__global__ __launch_bounds__(PX_THREADS) void k_prefix_fill_profile(DevMachine m, PrefixR R, const PrefixDesc *__restrict__ descs,
                                                                    const double *__restrict__ logP, double *pool, double *__restrict__ result) {
  extern __shared__ double px_V[];             // Y[r-1], N[r-1], Xn[r-1] (S doubles each), then the row's weights (nOut + 1)
  const PrefixDesc nd = descs[blockIdx.x];
  const int S = m.S, K = m.K, C = m.nOut + 1, L = nd.outLen, a = nd.inTok;
  double *px_N = px_V + S, *px_Xn = px_N + S, *px_P = px_Xn + S;
  const bool root = nd.parentBase < 0;
  const double *par = root ? nullptr : pool + nd.parentBase;
  double *cells = pool + nd.childBase;
  const double *P = logP + nd.outBase * C;
  for (int r = 0; r <= L; ++r) {
    double *W = cells + (long long)r * 2 * S, *X = W + S;
    const double *Wprev = W - 2 * S, *Xprev = W - S;       // (read for r > 0 only)
    if (r) {
      for (int c = threadIdx.x; c < C; c += blockDim.x) px_P[c] = P[(long long)(r - 1) * C + c];
      for (int s = threadIdx.x; s < S; s += blockDim.x) px_V[s] = px_column(R, s, Xprev);
      __syncthreads();
    }
    for (int d = threadIdx.x; d < S; d += blockDim.x) {
      const int row0 = d * K;
      double An = (root && r == 0 && d == 0) ? 0.0 : -INFINITY, Aw = -INFINITY;
      if (!root) {
        const double *pq = par + (long long)r * 2 * S;
        for (int e = m.inOff[row0 + a * C], e1 = m.inOff[row0 + a * C + 1]; e < e1; ++e) Aw = lse2_exact(Aw, pq[m.inSrc[e]] + m.inW[e]);
        if (r) {
          pq -= 2 * S;
          for (int o = 1; o < C; ++o) {
            const double po = px_P[o];
            if (!(po > -INFINITY)) continue;
            for (int e = m.inOff[row0 + a * C + o], e1 = m.inOff[row0 + a * C + o + 1]; e < e1; ++e) An = lse2_exact(An, (pq[m.inSrc[e]] + m.inW[e]) + po);
          }
        }
      }
      double pre = An, acc = An;                           // Xn and N
      if (r) {
        const double blank = px_P[0];
        acc = lse2_exact(acc, px_N[d] + blank);
        pre = lse2_exact(pre, px_Xn[d] + blank);
        for (int o = 1; o < C; ++o) {
          const double po = px_P[o];
          if (!(po > -INFINITY)) continue;
          for (int e = m.inOff[row0 + o], e1 = m.inOff[row0 + o + 1]; e < e1; ++e) acc = lse2_exact(acc, (Wprev[m.inSrc[e]] + m.inW[e]) + po);
          for (int i = 0; i <= m.nIn; ++i)
            for (int e = m.inOff[row0 + i * C + o], e1 = m.inOff[row0 + i * C + o + 1]; e < e1; ++e) pre = lse2_exact(pre, (px_V[m.inSrc[e]] + m.inW[e]) + po);
        }
      }
      px_N[d] = acc;                                       // (this lane's own entries: nobody else reads them)
      px_Xn[d] = pre;
      X[d] = lse2_exact(Aw, pre);
      W[d] = lse2_exact(Aw, acc);
    }
    __syncthreads();
    for (int lev = 1; lev < m.nLevF; ++lev) {          // level 0 has no silent edge coming in: its cells are final
      const int l0 = m.levFOff[lev], ns = m.levFOff[lev + 1] - l0;
      for (int k = threadIdx.x; k < ns; k += blockDim.x) {
        const int q = m.levFState[l0 + k];
        double acc = W[q];
        for (int e = m.inOff[q * K], e1 = m.inOff[q * K + 1]; e < e1; ++e) {
          const int s = (int)m.inSrc[e];
          if (s >= q) continue;                         // as the token sweeps: a silent self-loop never fires
          acc = lse2_exact(acc, W[s] + m.inW[e]);
        }
        W[q] = acc;
      }
      __syncthreads();
    }
  }
  if (threadIdx.x == 0) {
    const double *last = cells + (long long)L * 2 * S;
    result[2 * blockIdx.x] = last[S - 1];
    result[2 * blockIdx.x + 1] = px_column(R, S - 1, last + S);      // Y[L][S-1]: the only column of the last product that is needed
  }
}

int launch_prefix_fill_profile(const mb_machine *m, const PrefixR &R, const PrefixDesc *d, int n, const double *logP, double *pool,
                               double *result, hipStream_t st) {
  if (n <= 0) return 0;
  const size_t lds = ((size_t)3 * m->S + m->nOut + 1) * sizeof(double);
  static size_t ldsAllowed = 64 * 1024;      // as launch_prefix_fill: asked for once, and only when a machine needs it
  if (lds > ldsAllowed) {
    if (lds > PREFIX_PROFILE_MAX_LDS) { set_error("prefix search against profiles: 3 x states + output symbols doubles exceed the LDS of a workgroup (about 6 800 states)"); return 1; }
    if (!hip_ok(hipFuncSetAttribute((const void *)&k_prefix_fill_profile, hipFuncAttributeMaxDynamicSharedMemorySize, (int)PREFIX_PROFILE_MAX_LDS),
                "k_prefix_fill_profile: raising the LDS limit for a machine of more than 2 700 states")) return 1;
    ldsAllowed = PREFIX_PROFILE_MAX_LDS;
  }
  const int threads = std::min(PX_THREADS, std::max(64, (m->S + 63) / 64 * 64));
  k_prefix_fill_profile<<<dim3(n), dim3(threads), lds, st>>>(m->dev, R, d, logP, pool, result);
  return hip_ok(hipGetLastError(), "k_prefix_fill_profile") ? 0 : 1;
}

}  // namespace mb
