// mb_prefix_merge.hip -- the node fill of the prefix search against a CTC-MERGED profile: the token search on
// compose(M, transpose(CSVProfile::mergingMachine())) with an empty output, swept natively over rows r = 0..L, the nCols + 1 "last
// column seen" planes of mb_profile_merge.hip and M's own states (docs/decoding.md, "Decoding against a merged profile").  With a the
// node's symbol, Pa its parent, P[r][0] the blank, colTok[c] the output token of column c and excl_c(V)[s] = (+)_{k != c} V[k][s]:
//
//   An[r][0][d] = [root, r = 0, d = 0]
//   An[r][c][d] = sum_{t: s->d, in = a, out = colTok[c]} excl_c(Pa.W[r-1])[s] + w_t + P[r-1][c]
//   Aw[r][p][d] = sum_{t: s->d, in = a, out = eps} Pa.W[r][p][s] + w_t
//   N[r][0][d]  = An[r][0][d] (+) ((+)_p N[r-1][p][d]) + P[r-1][0]
//   N[r][c][d]  = An[r][c][d] (+) (N[r-1][c][d] + P[r-1][c]) (+) sum_{t: in = eps, out = colTok[c]} excl_c(W[r-1])[s] + w_t + P[r-1][c]
//   W[r][p][d]  = Aw[r][p][d] (+) N[r][p][d] (+) sum_{silent t: s->d, s < d} W[r][p][s] + w_t
//   Xn[r][0][d] = An[r][0][d] (+) ((+)_p Xn[r-1][p][d]) + P[r-1][0]
//   Xn[r][c][d] = An[r][c][d] (+) (Xn[r-1][c][d] + P[r-1][c]) (+) sum_{t: any in, out = colTok[c]} excl_c(Y[r-1])[s] + w_t + P[r-1][c]
//   X[r][p][d]  = Aw[r][p][d] (+) Xn[r][p][d]
//   Y[r][p][s]  = logsum_q X[r][p][q] + R[q][s]
//   logSeqProb  = (+)_p W[L][p][S-1],   logPrefixProb = (+)_p Y[L][p][S-1]
//
// The blank and the repeat read the ARRIVED stage (N, Xn), never W or X, as in k_prefix_fill_profile.  Layer 0 of a slot is W, layer 1
// is X, at cells[(((r*2) + layer)*(nCols+1) + p)*S + q] (the layout of mb_profile_fill_merged).
//
// One workgroup per node; the lanes are split into one group per plane and a group's lanes run over the states (the grouping of
// mb_profile_merge.hip).  Per row: (1) the Y product per plane with the token kernel's column code, the row's weights into LDS;
// a barrier; (2) the three exclusion vectors (of Pa.W[r-1], of the node's own W[r-1], of Y[r-1]) by the groups of the columns and
// the two blank sums (+)_p N[r-1][p], (+)_p Xn[r-1][p] by the group of plane 0 -- nCols terms per item, so that no edge loop runs over
// planes and no lane reads an N another lane is replacing; a barrier; (3) the middle phase: Aw, An, N, Xn, W, X; a barrier; (4) the
// silent levels of W, all planes at once, one barrier per level.  N and Xn are read only by the lane that wrote them (and by the
// blank sums, a barrier apart); they, Y, the exclusion vectors and the blank sums live in LDS and are not stored:
// merged_prefix_lds_doubles.  A column of weight -inf is skipped as a whole (the branch is uniform over its group).  Cells are fp64,
// sums the exact log-sum-exp; every cell has one writer and a fixed order of terms -- the node's own symbol, the blank or the repeat,
// then the edges in `incoming` order -- so a fill gives the same bits from run to run.
#include <algorithm>

#include "mb_device_math.h"
#include "mb_prefix.h"

namespace mb {

static constexpr int PXM_THREADS = 1024;

// log sum_p exp(row[p] + R[p][s]) over the finite entries of column s (px_column of mb_prefix.hip)
__device__ __forceinline__ double pxm_column(const PrefixR &R, int s, const double *row) {
  const long long k0 = R.rOff[s], k1 = R.rOff[s + 1];
  double mx = -INFINITY;
  for (long long k = k0; k < k1; ++k) mx = dmax(mx, row[R.rIdx[k]] + R.rVal[k]);
  if (!(mx > -INFINITY)) return -INFINITY;
  double sum = 0.0;
  for (long long k = k0; k < k1; ++k) sum += exp((row[R.rIdx[k]] + R.rVal[k]) - mx);
  return mx + log(sum);
}

// (+)_{k != c} V[k][s] over the PL planes of V (plane stride S), c >= 1, planes ascending
__device__ __forceinline__ double pxm_excl(const double *V, int PL, int S, int c, int s) {
  double acc = V[s];                                    // plane 0 is never the excluded one
  for (int k = 1; k < PL; ++k)
    if (k != c) acc = lse2_exact(acc, V[(long long)k * S + s]);
  return acc;
}

__global__ __launch_bounds__(PXM_THREADS) void k_prefix_fill_merged(DevMachine m, PrefixR R, int nCols, const int *__restrict__ colTok,
                                                                    const PrefixDesc *__restrict__ descs, const double *__restrict__ logP,
                                                                    double *pool, double *__restrict__ result) {
  extern __shared__ double pxm_sh[];
  const PrefixDesc nd = descs[blockIdx.x];
  const int S = m.S, K = m.K, C = m.nOut + 1, PL = nCols + 1, L = nd.outLen, a = nd.inTok;
  const long long PS = (long long)PL * S, CS = (long long)nCols * S;
  double *sY = pxm_sh, *sN = sY + PS, *sXn = sN + PS;                     // [PL][S] each
  double *eP = sXn + PS, *eW = eP + CS, *eY = eW + CS;                    // [nCols][S] each: the exclusion vectors, column c at (c-1)*S
  double *bN = eY + CS, *bXn = bN + S, *sP = bXn + S;                     // the blank sums [S] each, the row's weights [PL]
  const bool root = nd.parentBase < 0;
  const double *par = root ? nullptr : pool + nd.parentBase;
  double *cells = pool + nd.childBase;
  const double *P = logP + nd.outBase * PL;
  // the lanes as plane groups: G groups of LPP lanes, a lane serves planes p0, p0 + G, ... and states ln, ln + LPP, ... of each
  const int G = min(PL, (int)blockDim.x), LPP = (int)blockDim.x / G;
  int p0 = (int)threadIdx.x / LPP;
  const int ln = (int)threadIdx.x - p0 * LPP;
  if (p0 >= G) p0 = PL;                                                    // lanes beyond G * LPP idle but keep the barriers
  for (int r = 0; r <= L; ++r) {
    double *W = cells + (long long)r * 2 * PS, *X = W + PS;
    const double *Wprev = W - 2 * PS, *Xprev = W - PS;                     // (read for r > 0 only)
    if (r) {
      for (int c = threadIdx.x; c < PL; c += blockDim.x) sP[c] = P[(long long)(r - 1) * PL + c];
      for (int p = p0; p < PL; p += G)
        for (int s = ln; s < S; s += LPP) sY[(long long)p * S + s] = pxm_column(R, s, Xprev + (long long)p * S);
      __syncthreads();
      const double *parPrev = root ? nullptr : par + (long long)(r - 1) * 2 * PS;
      for (int p = p0; p < PL; p += G) {
        if (!(sP[p] > -INFINITY)) continue;
        if (p == 0) {
          for (int s = ln; s < S; s += LPP) {
            double n = sN[s], x = sXn[s];
            for (int k = 1; k < PL; ++k) { n = lse2_exact(n, sN[(long long)k * S + s]); x = lse2_exact(x, sXn[(long long)k * S + s]); }
            bN[s] = n; bXn[s] = x;
          }
        } else {
          const long long o = (long long)(p - 1) * S;
          for (int s = ln; s < S; s += LPP) {
            if (!root) eP[o + s] = pxm_excl(parPrev, PL, S, p, s);
            eW[o + s] = pxm_excl(Wprev, PL, S, p, s);
            eY[o + s] = pxm_excl(sY, PL, S, p, s);
          }
        }
      }
      __syncthreads();
    }
    for (int p = p0; p < PL; p += G) {
      const double wp = r ? sP[p] : -INFINITY;
      const bool live = wp > -INFINITY;
      const int tok = p ? colTok[p - 1] : 0;
      const long long o = (long long)(p - 1) * S, po = (long long)p * S;
      const double *pq = root ? nullptr : par + (long long)r * 2 * PS + po;
      for (int d = ln; d < S; d += LPP) {
        const int row0 = d * K;
        double An = (root && r == 0 && p == 0 && d == 0) ? 0.0 : -INFINITY, Aw = -INFINITY;
        if (!root) {
          for (int e = m.inOff[row0 + a * C], e1 = m.inOff[row0 + a * C + 1]; e < e1; ++e) Aw = lse2_exact(Aw, pq[m.inSrc[e]] + m.inW[e]);
          if (p && live)
            for (int e = m.inOff[row0 + a * C + tok], e1 = m.inOff[row0 + a * C + tok + 1]; e < e1; ++e) An = lse2_exact(An, (eP[o + m.inSrc[e]] + m.inW[e]) + wp);
        }
        double pre = An, acc = An;                           // Xn and N
        if (live) {
          if (p == 0) {
            acc = lse2_exact(acc, bN[d] + wp);
            pre = lse2_exact(pre, bXn[d] + wp);
          } else {
            acc = lse2_exact(acc, sN[po + d] + wp);
            pre = lse2_exact(pre, sXn[po + d] + wp);
            for (int e = m.inOff[row0 + tok], e1 = m.inOff[row0 + tok + 1]; e < e1; ++e) acc = lse2_exact(acc, (eW[o + m.inSrc[e]] + m.inW[e]) + wp);
            for (int i = 0; i <= m.nIn; ++i)
              for (int e = m.inOff[row0 + i * C + tok], e1 = m.inOff[row0 + i * C + tok + 1]; e < e1; ++e) pre = lse2_exact(pre, (eY[o + m.inSrc[e]] + m.inW[e]) + wp);
          }
        }
        sN[po + d] = acc;                                    // (this lane's own entries; the blank sums read them a barrier later)
        sXn[po + d] = pre;
        X[po + d] = lse2_exact(Aw, pre);
        W[po + d] = lse2_exact(Aw, acc);
      }
    }
    __syncthreads();
    for (int lev = 1; lev < m.nLevF; ++lev) {          // level 0 has no silent edge coming in: its cells are final
      const int l0 = m.levFOff[lev], ns = m.levFOff[lev + 1] - l0;
      for (int p = p0; p < PL; p += G) {
        double *Wp = W + (long long)p * S;
        for (int k = ln; k < ns; k += LPP) {
          const int q = m.levFState[l0 + k];
          double acc = Wp[q];
          for (int e = m.inOff[q * K], e1 = m.inOff[q * K + 1]; e < e1; ++e) {
            const int s = (int)m.inSrc[e];
            if (s >= q) continue;                         // as the token sweeps: a silent self-loop never fires
            acc = lse2_exact(acc, Wp[s] + m.inW[e]);
          }
          Wp[q] = acc;
        }
      }
      __syncthreads();
    }
  }
  if (threadIdx.x == 0) {
    const double *W = cells + (long long)L * 2 * PS, *X = W + PS;
    double lsp = W[S - 1], lpp = pxm_column(R, S - 1, X);          // Y[L][p][S-1]: the only column of the last product that is needed
    for (int p = 1; p < PL; ++p) {
      lsp = lse2_exact(lsp, W[(long long)p * S + S - 1]);
      lpp = lse2_exact(lpp, pxm_column(R, S - 1, X + (long long)p * S));
    }
    result[2 * blockIdx.x] = lsp;
    result[2 * blockIdx.x + 1] = lpp;
  }
}

int launch_prefix_fill_merged(const mb_machine *m, const PrefixR &R, int nCols, const int *colTok, const PrefixDesc *d, int n,
                              const double *logP, double *pool, double *result, hipStream_t st) {
  if (n <= 0) return 0;
  const size_t lds = (size_t)merged_prefix_lds_doubles(m->S, nCols) * sizeof(double);
  if (!merged_prefix_lds_fits(m->S, nCols)) {
    set_error("prefix search against merged profiles: ((6 nCols + 5) x states + nCols + 1) doubles exceed the LDS of a workgroup (160 KiB; " +
              std::to_string(m->S) + " states, " + std::to_string(nCols) + " columns)");
    return 1;
  }
  static size_t ldsAllowed = 64 * 1024;      // as launch_prefix_fill: asked for once, and only when a machine needs it
  if (lds > ldsAllowed) {
    if (!hip_ok(hipFuncSetAttribute((const void *)&k_prefix_fill_merged, hipFuncAttributeMaxDynamicSharedMemorySize, (int)PREFIX_PROFILE_MAX_LDS),
                "k_prefix_fill_merged: raising the LDS limit beyond 64 KiB")) return 1;
    ldsAllowed = PREFIX_PROFILE_MAX_LDS;
  }
  const long long items = (long long)(nCols + 1) * m->S;      // one lane per (plane, state) pair up to the workgroup's 1 024
  const int threads = (int)std::min<long long>(PXM_THREADS, std::max<long long>(64, (items + 63) / 64 * 64));
  k_prefix_fill_merged<<<dim3(n), dim3(threads), lds, st>>>(m->dev, R, nCols, colTok, d, logP, pool, result);
  return hip_ok(hipGetLastError(), "k_prefix_fill_merged") ? 0 : 1;
}

}  // namespace mb
