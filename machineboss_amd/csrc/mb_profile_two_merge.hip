// mb_profile_two_merge.hip -- Forward / Backward / Viterbi / posterior counts / row posteriors of a machine WITH an input alphabet between an input
// PROFILE A of K rows and a CTC-MERGED output profile B of L rows: the semantics of
// compose(A.machine(), compose(M, transpose(CSVProfile::mergingMachine()))) with both tapes empty, restated in docs/profile_tapes.md
// ("Pairs of profiles against a merged profile"):
//
//   XW[i][r][c][s] = (+)_{k != c} W[i][r][k][s]          XZ[i][r][c][s] = (+)_{k != c} Z[i][r][k][s]      (the exclusion vectors)
//   N[i][r][0][d]  = [i = 0, r = 0, d = 0]  (+)  (+)_p (N[i][r-1][p][d] + B[r-1][0])                        (output blank; r > 0)
//   N[i][r][c][d]  = (N[i][r-1][c][d] + B[r-1][c])                                                          (repeat; r > 0)
//                    (+) sum_{t: s->d, in = a,   out = colTok[c]} ((XZ[i-1][r-1][c][s] + w_t) + A[i-1][a]) + B[r-1][c]   (match)
//                    (+) sum_{t: s->d, in = eps, out = colTok[c]} (XW[i][r-1][c][s] + w_t) + B[r-1][c]                   (output-only)
//   W[i][r][p][d]  = N[i][r][p][d]
//                    (+) sum_{t: in = a, out = eps} (Z[i-1][r][p][s] + w_t) + A[i-1][a]                     (input-only; same plane)
//                    (+) sum_{silent t, s < d}      W[i][r][p][s] + w_t                                     (silent levels, per plane)
//   Z[i][r][p][d]  = W[i][r][p][d]  (+)  Z[i-1][r][p][d] + A[i-1][0]                                        (input blank; same plane)
//   loglike        = (+)_p Z[K][L][p][S-1]
//
// The anti-diagonal sweep of mb_profile_pair_merge.hip with the third layer and the all-input-token edge loops of mb_profile_two.hip
// (for a destination q the CSR rows q*K + a*C + o) and two exclusion vectors: the match edges leave the committed stage (XZ), the
// output-only edges the waiting stage (XW).  One workgroup per pair; the work items of a diagonal are (cell, plane, state).  Per
// diagonal: one phase for N and the non-silent part of W -- the item that finishes a state's W writes its Z -- and a barrier, one
// barrier per silent level, and one phase and barrier that forms XW and XZ, so that no edge loop runs over planes --
// (K + L + 1)(nLevF + 1) barriers per pair.  The rolling sweeps keep a ring of three diagonals of N, W, Z, XW and XZ,
// 3 (5 nCols + 3)(min(K, L) + 1) S doubles, in LDS when that fits 160 KiB, else in the pair's slice of a global scratch buffer; the
// materialised ones keep only XW and XZ there.  Cells are fp64, the sums the exact log-sum-exp.
//
// Every kernel is written once over TwoMergeLattice, which says which cells exist and where they live: its full form, the whole
// rectangle, or its envelope form, the cells of an envelope (docs/profile_tapes.md, "Pairs of profiles against a merged profile
// under an envelope"); the index rules of both are those of mb_profile_lattice.h.  Every plane of all three layers of a cell
// outside the envelope is -inf, and so are its XW, XZ, TZ and TW, so a neighbour outside is not read; the recurrence, the candidate
// order and the sums are the same text for both.
#include "mb_profile_common.h"
#include "mb_profile_two_merge.h"

namespace mb {

size_t profile_two_merge_lds_bytes(int S, int nCols, long long nIn, long long nRows, bool mat) {
  const double b = (double)profile_two_merge_ring(S, nCols, nIn, nRows, mat) * sizeof(double);
  return b <= (double)SWEEP_LDS_MAX ? (size_t)b : 0;
}

size_t profile_two_merge_env_lds_bytes(int S, int nCols, long long M, bool mat) {
  const double b = (double)profile_two_merge_env_ring(S, nCols, M, mat) * sizeof(double);
  return b <= (double)SWEEP_LDS_MAX ? (size_t)b : 0;
}

// Where cell (i, r) lives: the cells of mb_profile_lattice.h, RectCells or EnvCells, and this family's layout.  at(i, r, layer): its
// N (0), W (1) or Z (2), nCols + 1 planes of S states -- the materialised lattice of mb_profile_two_merge.h (under an envelope the
// compact one, cells[(((off[r] + i - inStart[r]) * 3 + layer) * (nCols + 1) + p) * S + q]), or the ring.  xw(i, r) / xz(i, r): its
// exclusion vectors over W / over Z, column c at (c - 1) * S -- always in the ring, beside the three layers when rolling.
template <class Cells, bool MAT>
struct TwoMergeStore : Cells {
  using Desc = std::conditional_t<Cells::ENV, TwoEnvDesc, PairProfDesc>;
  using Tables = std::conditional_t<Cells::ENV, TwoEnvTables, NoTables>;
  double *pool, *ring;
  int S, PL;
  __device__ __forceinline__ TwoMergeStore(const Desc &pd, const Tables &t, double *pool, double *ring, int S, int PL)
      : Cells(lattice_cells(pd, t)), pool(pool), ring(ring), S(S), PL(PL) {}
  __device__ __forceinline__ double *at(int i, int r, int layer) const {
    if (MAT) return pool + (this->index(i, r) * 3 + layer) * PL * S;
    return ring + (this->slot(i, r) * (5 * PL - 2) + layer * PL) * S;
  }
  __device__ __forceinline__ double *xw(int i, int r) const {
    if (MAT) return ring + this->slot(i, r) * 2 * (PL - 1) * S;
    return ring + (this->slot(i, r) * (5 * PL - 2) + 3 * PL) * S;
  }
  __device__ __forceinline__ double *xz(int i, int r) const { return xw(i, r) + (PL - 1) * S; }
};
template <bool MAT, bool ENV>
using TwoMergeLattice = TwoMergeStore<std::conditional_t<ENV, EnvCells, RectCells>, MAT>;

// Forward (MODE = MB_FORWARD) or Viterbi (MB_VITERBI) sweep.  MAT: every N, W and Z cell into pool (layout of
// mb_profile_two_merge.h) and only XW, XZ in the ring, else rolling.  Viterbi keeps the FIRST maximum: N[.][.][0] takes the planes
// ascending; N[.][.][c] the repeat first, then the match edges in `incoming` order (input token ascending), then the output-only
// edges; W takes N (no move) first, then the input-only edges, then the silent edges; Z takes W, then the input blank; XW, XZ and the
// end the planes ascending -- the order k_profile_two_merge_traceback re-enumerates.  A neighbour outside the lattice is -inf and
// is not read: (i, r - 1) feeds the output blank over all planes, the repeat and XW of the output-only edges, (i - 1, r - 1) XZ of
// the match edges, (i - 1, r) Z of the input-only edges and of the input blank.
template <int MODE, bool MAT, bool ENV>
__global__ __launch_bounds__(SWEEP_THREADS) void k_profile_two_merge_fwd(DevMachine m, MergeMap mm, const typename TwoMergeLattice<MAT, ENV>::Desc *__restrict__ descs,
                                                                         typename TwoMergeLattice<MAT, ENV>::Tables t,
                                                                         const double *__restrict__ logA, const double *__restrict__ logB,
                                                                         double *pool, double *scratch, double *__restrict__ loglike) {
  extern __shared__ double ptm_sh[];
  const auto pd = descs[blockIdx.x];
  const int S = m.S, KK = m.K, C = m.nOut + 1, CA = m.nIn + 1, nC = mm.nCols, PL = nC + 1, K = pd.nIn, L = pd.nRows;
  const double *A = logA + pd.inBase * CA;
  const double *B = logB + pd.rowBase * PL;
  const TwoMergeLattice<MAT, ENV> lat(pd, t, MAT ? pool + pd.cellBase : nullptr, pd.ringBase < 0 ? ptm_sh : scratch + pd.ringBase, S, PL);
  const int PS = PL * S;
  for (int d = 0; d <= K + L; ++d) {
    int ilo, nCells;
    lat.diag(d, ilo, nCells);
    const int nItems = nCells * PS;
    for (int it = threadIdx.x; it < nItems; it += blockDim.x) {
      const int c = it / PS, pq = it - c * PS, p = pq / S, q = pq - p * S, i = ilo + c, r = d - i;
      const double *Ai = A + (long long)max(i - 1, 0) * CA;      // row i - 1; read when i > 0
      double acc = (d == 0 && pq == 0) ? 0.0 : -INFINITY;
      if (r > 0) {
        const double w = B[(long long)(r - 1) * PL + p];
        const bool up = lat.inside(i, r - 1);
        const double *Np = lat.at(i, r - 1, 0);      // (an address alone: read only where the cell is inside)
        if (p == 0) {
          if (up) {
            acc = Np[q] + w;
            for (int k = 1; k < PL; ++k) acc = red<MODE>(acc, Np[k * S + q] + w);
          }
        } else if (w > -INFINITY) {                          // (a column the row rules out is skipped as a whole)
          const int tok = mm.colTok[p - 1];
          if (up) acc = Np[p * S + q] + w;
          if (i > 0 && lat.inside(i - 1, r - 1)) {
            const double *Xd = lat.xz(i - 1, r - 1) + (p - 1) * S;
            for (int a = 1; a <= m.nIn; ++a) {
              const int row = q * KK + a * C + tok;
              const double wa = Ai[a];
              const int e1 = m.inOff[row + 1];
              for (int e = m.inOff[row]; e < e1; ++e) acc = red<MODE>(acc, ((Xd[m.inSrc[e]] + m.inW[e]) + wa) + w);
            }
          }
          if (up) {
            const double *Xu = lat.xw(i, r - 1) + (p - 1) * S;
            const int e1 = m.inOff[q * KK + tok + 1];
            for (int e = m.inOff[q * KK + tok]; e < e1; ++e) acc = red<MODE>(acc, (Xu[m.inSrc[e]] + m.inW[e]) + w);
          }
        }
      }
      lat.at(i, r, 0)[pq] = acc;
      if (i > 0 && lat.inside(i - 1, r)) {
        const double *Zl = lat.at(i - 1, r, 2) + p * S;
        for (int a = 1; a <= m.nIn; ++a) {
          const int row = q * KK + a * C;
          const double wa = Ai[a];
          const int e1 = m.inOff[row + 1];
          for (int e = m.inOff[row]; e < e1; ++e) acc = red<MODE>(acc, (Zl[m.inSrc[e]] + m.inW[e]) + wa);
        }
        lat.at(i, r, 1)[pq] = acc;
        lat.at(i, r, 2)[pq] = red<MODE>(acc, Zl[q] + Ai[0]);
      } else {
        lat.at(i, r, 1)[pq] = acc;
        lat.at(i, r, 2)[pq] = acc;
      }
    }
    __syncthreads();
    for (int lev = 1; lev < m.nLevF; ++lev) {      // (level 0 has no silent edge coming in: its W and Z are complete)
      const int l0 = m.levFOff[lev], ns = m.levFOff[lev + 1] - l0;
      const int PN = PL * ns, nLevItems = nCells * PN;
      for (int it = threadIdx.x; it < nLevItems; it += blockDim.x) {
        const int c = it / PN, pj = it - c * PN, p = pj / ns, q = m.levFState[l0 + (pj - p * ns)], i = ilo + c, r = d - i;
        double *Wc = lat.at(i, r, 1) + p * S;
        double acc = Wc[q];
        const int e1 = m.inOff[q * KK + 1];
        for (int e = m.inOff[q * KK]; e < e1; ++e) {
          const int s = (int)m.inSrc[e];
          if (s >= q) continue;                       // as the token sweeps: a silent self-loop never fires
          acc = red<MODE>(acc, Wc[s] + m.inW[e]);
        }
        Wc[q] = acc;
        lat.at(i, r, 2)[p * S + q] = (i > 0 && lat.inside(i - 1, r)) ? red<MODE>(acc, lat.at(i - 1, r, 2)[p * S + q] + A[(long long)(i - 1) * CA]) : acc;
      }
      __syncthreads();
    }
    if (d < K + L) {
      const int XS = nC * S, nXItems = nCells * XS;
      for (int it = threadIdx.x; it < nXItems; it += blockDim.x) {
        const int c = it / XS, cs = it - c * XS, col = cs / S + 1, s = cs - (col - 1) * S, i = ilo + c;
        const double *Wc = lat.at(i, d - i, 1) + s, *Zc = lat.at(i, d - i, 2) + s;
        double aw = Wc[0], az = Zc[0];                   // plane 0 is never the excluded one
        for (int k = 1; k < PL; ++k)
          if (k != col) { aw = red<MODE>(aw, Wc[k * S]); az = red<MODE>(az, Zc[k * S]); }
        lat.xw(i, d - i)[cs] = aw;
        lat.xz(i, d - i)[cs] = az;
      }
      __syncthreads();
    }
  }
  if (threadIdx.x == 0) {
    const double *Ze = lat.at(K, L, 2) + S - 1;      // (an envelope is connected: (0, 0) and (K, L) are inside)
    double acc = Ze[0];
    for (int p = 1; p < PL; ++p) acc = red<MODE>(acc, Ze[p * S]);
    loglike[blockIdx.x] = acc;
  }
}

// Materialised Backward sweep, layer 0 = NB ("from the arrived stage"), 1 = WB ("from the waiting stage"), 2 = ZB ("from the
// committed stage"):
//   TZ[i][r][c][s] = sum_{t: s->d, in = a,   out = colTok[c]} ((w_t + A[i][a]) + B[r][c]) + NB[i+1][r+1][c][d]     (i < K, r < L)
//   TW[i][r][c][s] = sum_{t: s->d, in = eps, out = colTok[c]} (w_t + B[r][c]) + NB[i][r+1][c][d]                   (r < L)
//   ZB[i][r][k][s] = [i = K, r = L, s = S-1]  (+)  A[i][0] + ZB[i+1][r][k][s]  (+)  (+)_{c != k} TZ[i][r][c][s]
//                    (+) sum_{t: in = a, out = eps} (w_t + A[i][a]) + WB[i+1][r][k][d]                              (i < K)
//   WB[i][r][k][s] = ZB[i][r][k][s]  (+)  (+)_{c != k} TW[i][r][c][s]  (+)  sum_{silent t, s < d} w_t + WB[i][r][k][d]
//   NB[i][r][k][s] = WB[i][r][k][s] (+) (B[r][0] + NB[i][r+1][0][s]) (+) [k >= 1](B[r][k] + NB[i][r+1][k][s])       (r < L)
//   loglike        = NB[0][0][0][0]
// Anti-diagonals from K + L down.  TZ and TW, everything that leaves (i, r, s) through column c from the committed and from the
// waiting stage, are formed once per diagonal over (cell, column, state) -- the mirror of the Forward's XZ and XW -- so the edge
// loops do not run over planes; they live in the ring (one diagonal of them, the cell by its place on the diagonal, TZ then TW).  A
// state's WB is final once its backward level has run; the item that finishes it writes its NB.  A successor cell outside the
// lattice contributes nothing: (i + 1, r + 1) is asked before TZ reads it, (i, r + 1) before TW, the output blank and the repeat do,
// (i + 1, r) before the input blank and the input-only edges do.
template <bool ENV>
__global__ __launch_bounds__(SWEEP_THREADS) void k_profile_two_merge_bwd(DevMachine m, MergeMap mm, const typename TwoMergeLattice<true, ENV>::Desc *__restrict__ descs,
                                                                         typename TwoMergeLattice<true, ENV>::Tables t,
                                                                         const double *__restrict__ logA, const double *__restrict__ logB,
                                                                         double *pool, double *scratch, double *__restrict__ loglike) {
  extern __shared__ double ptm_sh[];
  const auto pd = descs[blockIdx.x];
  const int S = m.S, KK = m.K, C = m.nOut + 1, CA = m.nIn + 1, nC = mm.nCols, PL = nC + 1, K = pd.nIn, L = pd.nRows;
  const double *A = logA + pd.inBase * CA;
  const double *B = logB + pd.rowBase * PL;
  const TwoMergeLattice<true, ENV> lat(pd, t, pool + pd.cellBase, nullptr, S, PL);
  double *T = pd.ringBase < 0 ? ptm_sh : scratch + pd.ringBase;       // T[((cell on the diagonal * 2 + (0: TZ, 1: TW)) * nCols + c - 1) * S + s]
  const int PS = PL * S, XS = nC * S;
  for (int d = K + L; d >= 0; --d) {
    int ilo, nCells;
    lat.diag(d, ilo, nCells);
    if (d < K + L) {
      const int nTItems = nCells * XS;
      for (int it = threadIdx.x; it < nTItems; it += blockDim.x) {
        const int c = it / XS, cs = it - c * XS, col = cs / S + 1, s = cs - (col - 1) * S, i = ilo + c, r = d - i;
        double tz = -INFINITY, tw = -INFINITY;
        if (r < L) {
          const double pc = B[(long long)r * PL + col];
          if (pc > -INFINITY) {
            const int tok = mm.colTok[col - 1];
            if (i < K && lat.inside(i + 1, r + 1)) {
              const double *Nd = lat.at(i + 1, r + 1, 0) + col * S;
              const double *Ai = A + (long long)i * CA;
              for (int a = 1; a <= m.nIn; ++a) {
                const int row = s * KK + a * C + tok;
                const double wa = Ai[a];
                const int e1 = m.outOff[row + 1];
                for (int e = m.outOff[row]; e < e1; ++e) tz = lse2_exact(tz, ((m.outW[e] + wa) + pc) + Nd[m.outDst[e]]);
              }
            }
            if (lat.inside(i, r + 1)) {
              const double *Nu = lat.at(i, r + 1, 0) + col * S;
              const int e1 = m.outOff[s * KK + tok + 1];
              for (int e = m.outOff[s * KK + tok]; e < e1; ++e) tw = lse2_exact(tw, (m.outW[e] + pc) + Nu[m.outDst[e]]);
            }
          }
        }
        T[(long long)c * 2 * XS + cs] = tz;
        T[(long long)c * 2 * XS + XS + cs] = tw;
      }
      __syncthreads();
    }
    const int nItems = nCells * PS;
    for (int it = threadIdx.x; it < nItems; it += blockDim.x) {
      const int c = it / PS, ks = it - c * PS, k = ks / S, s = ks - k * S, i = ilo + c, r = d - i;
      const double *Tc = T + (long long)c * 2 * XS + s;
      double v = (d == K + L && s == S - 1) ? 0.0 : -INFINITY;
      if (i < K) {
        const double *Ai = A + (long long)i * CA;
        const bool right = lat.inside(i + 1, r);
        if (right) v = lse2_exact(v, Ai[0] + lat.at(i + 1, r, 2)[ks]);
        if (r < L)      // (TZ of a target outside is -inf)
          for (int col = 1; col < PL; ++col)
            if (col != k) v = lse2_exact(v, Tc[(col - 1) * S]);
        if (right) {
          const double *Wl = lat.at(i + 1, r, 1) + k * S;
          for (int a = 1; a <= m.nIn; ++a) {
            const int row = s * KK + a * C;
            const double wa = Ai[a];
            const int e1 = m.outOff[row + 1];
            for (int e = m.outOff[row]; e < e1; ++e) v = lse2_exact(v, (m.outW[e] + wa) + Wl[m.outDst[e]]);
          }
        }
      }
      lat.at(i, r, 2)[ks] = v;
      if (r < L)
        for (int col = 1; col < PL; ++col)
          if (col != k) v = lse2_exact(v, Tc[XS + (col - 1) * S]);
      lat.at(i, r, 1)[ks] = v;
      if (r < L && lat.inside(i, r + 1)) {
        const double *Nn = lat.at(i, r + 1, 0), *Br = B + (long long)r * PL;
        v = lse2_exact(v, Br[0] + Nn[s]);
        if (k) v = lse2_exact(v, Br[k] + Nn[ks]);
      }
      lat.at(i, r, 0)[ks] = v;
    }
    __syncthreads();
    for (int lev = 1; lev < m.nLevB; ++lev) {
      const int l0 = m.levBOff[lev], ns = m.levBOff[lev + 1] - l0;
      const int PN = PL * ns, nLevItems = nCells * PN;
      for (int it = threadIdx.x; it < nLevItems; it += blockDim.x) {
        const int c = it / PN, kj = it - c * PN, k = kj / ns, s = m.levBState[l0 + (kj - k * ns)], i = ilo + c, r = d - i;
        double *Wc = lat.at(i, r, 1) + k * S;
        double v = Wc[s];
        const int e1 = m.outOff[s * KK + 1];
        for (int e = m.outOff[s * KK]; e < e1; ++e) {
          const int t = (int)m.outDst[e];
          if (t <= s) continue;
          v = lse2_exact(v, Wc[t] + m.outW[e]);
        }
        Wc[s] = v;
        if (r < L && lat.inside(i, r + 1)) {
          const double *Nn = lat.at(i, r + 1, 0), *Br = B + (long long)r * PL;
          v = lse2_exact(v, Br[0] + Nn[s]);
          if (k) v = lse2_exact(v, Br[k] + Nn[k * S + s]);
        }
        lat.at(i, r, 0)[k * S + s] = v;
      }
      __syncthreads();
    }
  }
  if (threadIdx.x == 0) loglike[blockIdx.x] = lat.at(0, 0, 0)[0];
}

// Posterior counts.  With both lattices in memory every (cell, plane, edge) term is independent:
//   count[t] += exp(F[i][r][k][s] - LL + term_t), term_t the edge's summand of ZB (read from Z_F: the input-reading edges) or of WB
//   (read from W_F: the others) above, through TZ / TW for the emitting edges: every column c != k,
// so the sweep is a flat grid over (pair, group of the pair, (cell, plane, state)), accumulated by CountsAcc (mb_profile_common.h).
// A pair whose likelihood is -inf adds nothing; the blanks of either tape and the repeat rows are not edges.  The cells of an
// envelope are counted through its compact index (a cell finds its row by bisection in off); a term whose destination lies outside
// is left out.
template <bool ENV>
__global__ __launch_bounds__(256) void k_profile_two_merge_counts(DevMachine m, MergeMap mm, const typename TwoMergeLattice<true, ENV>::Desc *__restrict__ descs,
                                                                  typename TwoMergeLattice<true, ENV>::Tables t,
                                                                  int groupsPerPair, const double *__restrict__ logA,
                                                                  const double *__restrict__ logB, const double *__restrict__ fwdPool,
                                                                  const double *__restrict__ bwdPool, long long nTrans,
                                                                  double *__restrict__ counts, int det) {
  __shared__ double lcount[COUNTS_LDS_MAX];
  const CountsAcc acc(lcount, counts, nTrans, det);
  const int pair = blockIdx.x / groupsPerPair, group = blockIdx.x % groupsPerPair;
  const auto pd = descs[pair];
  const int S = m.S, KK = m.K, C = m.nOut + 1, CA = m.nIn + 1, nC = mm.nCols, PL = nC + 1, K = pd.nIn, L = pd.nRows;
  const double *A = logA + pd.inBase * CA;
  const double *B = logB + pd.rowBase * PL;
  const TwoMergeLattice<true, ENV> F(pd, t, const_cast<double *>(fwdPool) + pd.cellBase, nullptr, S, PL),
      Bk(pd, t, const_cast<double *>(bwdPool) + pd.cellBase, nullptr, S, PL);
  double LL;
  {
    const double *Ze = F.at(K, L, 2) + S - 1;
    LL = Ze[0];
    for (int p = 1; p < PL; ++p) LL = lse2_exact(LL, Ze[p * S]);
  }
  if (LL > -INFINITY) {
    const long long PS = (long long)PL * S, nItems = F.cells() * PS;
    for (long long idx = (long long)group * blockDim.x + threadIdx.x; idx < nItems; idx += (long long)groupsPerPair * blockDim.x) {
      const long long cell = idx / PS;
      const int ks = (int)(idx - cell * PS), k = ks / S, s = ks - k * S;
      int i, r;
      F.cell(cell, i, r);
      const double f = F.at(i, r, 1)[ks] - LL, z = F.at(i, r, 2)[ks] - LL;
      if (!(z > -INFINITY)) continue;                 // (Z holds W: a dead Z is a dead W)
      const double *Br = B + (long long)r * PL;       // read when r < L
      if (i < K) {
        const double *Ai = A + (long long)i * CA;
        const bool right = Bk.inside(i + 1, r), across = r < L && Bk.inside(i + 1, r + 1);
        const double *Wl = Bk.at(i + 1, r, 1) + k * S;      // (an address alone: read only where the cell is inside)
        for (int a = 1; a <= m.nIn; ++a) {
          const int row = s * KK + a * C;
          const double wa = Ai[a];
          if (across) {
            const double *Nd = Bk.at(i + 1, r + 1, 0);
            for (int col = 1; col < PL; ++col) {
              const double pc = Br[col];
              if (col == k || !(pc > -INFINITY)) continue;
              const int tok = mm.colTok[col - 1];
              const int e1 = m.outOff[row + tok + 1];
              for (int e = m.outOff[row + tok]; e < e1; ++e)
                acc.add(m.outEid[e], exp(z + (((m.outW[e] + wa) + pc) + Nd[col * S + m.outDst[e]])));
            }
          }
          if (right) {
            const int e1 = m.outOff[row + 1];
            for (int e = m.outOff[row]; e < e1; ++e) acc.add(m.outEid[e], exp(z + ((m.outW[e] + wa) + Wl[m.outDst[e]])));
          }
        }
      }
      if (!(f > -INFINITY)) continue;
      if (r < L && Bk.inside(i, r + 1)) {
        const double *Nu = Bk.at(i, r + 1, 0);
        for (int col = 1; col < PL; ++col) {
          const double pc = Br[col];
          if (col == k || !(pc > -INFINITY)) continue;
          const int tok = mm.colTok[col - 1];
          const int e1 = m.outOff[s * KK + tok + 1];
          for (int e = m.outOff[s * KK + tok]; e < e1; ++e) acc.add(m.outEid[e], exp(f + ((m.outW[e] + pc) + Nu[col * S + m.outDst[e]])));
        }
      }
      const double *Wc = Bk.at(i, r, 1) + k * S;
      const int e1 = m.outOff[s * KK + 1];
      for (int e = m.outOff[s * KK]; e < e1; ++e) {
        const int t = (int)m.outDst[e];
        if (t <= s) continue;
        acc.add(m.outEid[e], exp(f + (Wc[t] + m.outW[e])));
      }
    }
  }
  acc.flush();
}

// Row posteriors of both tapes (docs/profile_tapes.md, "Row posteriors of pairs of profiles against a merged profile"): the terms of
// k_profile_two_merge_counts, the blank masses of either tape and the repeats, binned by (line, column) instead of by transition.
// AXIS 0 bins output rows -- post[(rowBase + r) * (nCols + 1) + c] is the gradient of the log-likelihood in B[r][c]:
//   post[r][0] = sum_i sum_p sum_s exp((N_F[i][r][p][s] - LL) + (B[r][0] + NB[i][r+1][0][s]))
//   post[r][c] = sum_i sum_s exp((N_F[i][r][c][s] - LL) + (B[r][c] + NB[i][r+1][c][s]))                     (the repeat)
//              + the match terms (read from Z_F) and the output-only terms (read from W_F) of every plane k != c
// AXIS 1 bins input rows -- post[(inBase + i) * (nIn + 1) + a] is the gradient in A[i][a]:
//   post[i][0] = sum_r sum_p sum_s exp((Z_F[i][r][p][s] - LL) + (A[i][0] + ZB[i+1][r][p][s]))
//   post[i][a] = the input-only terms (into WB[i+1][r], same plane) and the match terms of every column c != k, all read from Z_F
// The scheme is the one of k_profile_pair_merge_rowpost (mb_profile_pair_merge.hip) once per axis, as k_profile_two_rowpost
// (mb_profile_two.hip) applies k_profile_pair_rowpost: the work items are (line, cell of the line, plane, state) in that order and a
// workgroup owns whole lines, blocks of profile_pair_rowpost_rows lines dealt round robin to the pair's groups.  A lane sums its
// terms of one column in a register, in CSR order (axis 0, column c: the rows s*K + a*C + colTok[c] for a = 1..nIn, then
// s*K + colTok[c]; axis 1, column a: the row s*K + a*C, then the rows s*K + a*C + colTok[c] for c ascending): the sum over k != c runs
// over the items, neither exclusion vector of the Forward sweep is needed.  rowpost_add reduces the lane sums of a wavefront that
// lies in one line and adds to the workgroup's LDS table, which is then stored: every bin has one writing workgroup, so there is no
// global atomic and nothing to clear beforehand.  A line of more than tabMax columns is summed in its global bins instead, cleared
// by the workgroup that owns it.  A pair whose likelihood is -inf gets zeros by the same stores.  loglike: the Forward sweep's, per
// pair of the launch.  det: post holds 64-bit fixed point at 2^-36.
// Under an envelope the lines are those of the lattice (lineFirst / lineCell): on axis 0 the compact index already counts row by row;
// on axis 1 the lines are COLUMNS of the envelope -- by monotonicity the cells of input row i are the run r = colStart[i] ..
// colEnd[i] - 1, an item finds its column by bisection in colOff and its cell through at().  A term whose destination lies outside
// is left out, the match terms to (i + 1, r + 1) independently of the input-only and input-blank terms to (i + 1, r).
template <int AXIS, bool ENV>
__global__ __launch_bounds__(ROWPOST_THREADS) void k_profile_two_merge_rowpost(DevMachine m, MergeMap mm, const typename TwoMergeLattice<true, ENV>::Desc *__restrict__ descs,
                                                                               typename TwoMergeLattice<true, ENV>::Tables t, int groupsPerPair, const double *__restrict__ logA,
                                                                               const double *__restrict__ logB, const double *__restrict__ fwdPool,
                                                                               const double *__restrict__ bwdPool, const double *__restrict__ loglike,
                                                                               double *post, int tabMax, int det) {
  __shared__ double ltab[ROWPOST_LDS_MAX];
  const int pair = blockIdx.x / groupsPerPair, group = blockIdx.x % groupsPerPair;
  const auto pd = descs[pair];
  const int S = m.S, KK = m.K, C = m.nOut + 1, CA = m.nIn + 1, nC = mm.nCols, PL = nC + 1, K = pd.nIn, L = pd.nRows;
  const int NL = AXIS ? K : L, NC = AXIS ? CA : PL;      // lines, bins of a line
  if (NL == 0) return;
  const double *A = logA + pd.inBase * CA;
  const double *B = logB + pd.rowBase * PL;
  const TwoMergeLattice<true, ENV> F(pd, t, const_cast<double *>(fwdPool) + pd.cellBase, nullptr, S, PL),
      Bk(pd, t, const_cast<double *>(bwdPool) + pd.cellBase, nullptr, S, PL);
  const double LL = loglike[pair];
  const long long PS = (long long)PL * S;
  const int R = profile_pair_rowpost_rows(F.cells() * PL, S, NL, NC, tabMax);
  const bool useLds = NC <= tabMax;
  const int lane = threadIdx.x & 63;
  for (long long lb = (long long)group * R; lb < NL; lb += (long long)groupsPerPair * R) {
    const int l0 = (int)lb, l1 = (int)min((long long)NL, lb + R), nBins = (l1 - l0) * NC;
    double *out = post + ((AXIS ? pd.inBase : pd.rowBase) + l0) * NC;
    double *tab = useLds ? ltab : out;
    for (int e = threadIdx.x; e < nBins; e += blockDim.x) tab[e] = 0.0;      // (the fixed point's zero has the same bits)
    if (!useLds) __threadfence();
    __syncthreads();
    if (LL > -INFINITY) {
      const long long c0 = F.template lineFirst<AXIS>(l0), nItems = (F.template lineFirst<AXIS>(l1) - c0) * PS;
      for (long long base = threadIdx.x - lane; base < nItems; base += blockDim.x) {      // (a wavefront stays whole in here)
        const long long idx = base + lane;
        const bool valid = idx < nItems;
        int i = AXIS ? l0 : 0, r = AXIS ? 0 : l0, k = 0, s = 0, ks = 0;
        if (valid) {
          const long long cell = idx / PS;
          ks = (int)(idx - cell * PS);
          k = ks / S;
          s = ks - k * S;
          F.template lineCell<AXIS>(c0 + cell, i, r);
        }
        const int line = AXIS ? i : r;
        const double z = valid ? F.at(i, r, 2)[ks] - LL : -INFINITY;
        const bool whole = __all(valid && line == __shfl(line, 0));
        // (the line's own coordinate is inside: r < L on axis 0, i < K on axis 1)
        const bool diag = valid && i < K && r < L && Bk.inside(i + 1, r + 1);
        const double *Ai = A + (long long)i * CA;        // read when i < K
        const double *Br = B + (long long)r * PL;        // read when r < L
        const double *Nd = diag ? Bk.at(i + 1, r + 1, 0) : nullptr;
        const int sRow = s * KK, bin0 = (line - l0) * NC;
        const bool zLive = z > -INFINITY;
        if (AXIS == 0) {
          const double f = valid ? F.at(i, r, 1)[ks] - LL : -INFINITY, n = valid ? F.at(i, r, 0)[ks] - LL : -INFINITY;
          const bool up = Bk.inside(i, r + 1);
          const double *Nu = Bk.at(i, r + 1, 0);         // (an address alone where the item is not valid or the cell outside: read only where f or n lives)
          const bool nLive = up && n > -INFINITY, fLive = up && f > -INFINITY, dLive = diag && zLive;
          rowpost_add(tab, bin0, nLive ? exp(n + (Br[0] + Nu[s])) : 0.0, whole, lane, det);
          for (int c = 1; c < PL; ++c) {      // the out-edges of (s, a) that write the column's token are one CSR row
            double v = 0.0;
            if (valid && c == k) {
              if (nLive) v = exp(n + (Br[c] + Nu[ks]));
            } else if (fLive || dLive) {
              const double pc = Br[c];
              if (pc > -INFINITY) {
                const int tok = mm.colTok[c - 1];
                if (dLive) {
                  const double *Ndc = Nd + (long long)c * S;
                  for (int a = 1; a <= m.nIn; ++a) {
                    const int row = sRow + a * C + tok;
                    const double wa = Ai[a];
                    const int e1 = m.outOff[row + 1];
                    for (int e = m.outOff[row]; e < e1; ++e) v += exp(z + (((m.outW[e] + wa) + pc) + Ndc[m.outDst[e]]));
                  }
                }
                if (fLive) {
                  const double *Nuc = Nu + (long long)c * S;
                  const int e1 = m.outOff[sRow + tok + 1];
                  for (int e = m.outOff[sRow + tok]; e < e1; ++e) v += exp(f + ((m.outW[e] + pc) + Nuc[m.outDst[e]]));
                }
              }
            }
            rowpost_add(tab, bin0 + c, v, whole, lane, det);
          }
        } else {
          const bool right = Bk.inside(i + 1, r);      // (i < K: the cell is inside the rectangle)
          const double *Zl = Bk.at(i + 1, r, 2), *Wl = Bk.at(i + 1, r, 1) + (long long)k * S;
          rowpost_add(tab, bin0, (right && zLive) ? exp(z + (Ai[0] + Zl[ks])) : 0.0, whole, lane, det);
          for (int a = 1; a < CA; ++a) {      // the out-edges of s that read a: the input-only row, then the rows of the columns' tokens
            double v = 0.0;
            if (zLive) {
              const int row = sRow + a * C;
              const double wa = Ai[a];
              if (right) {
                const int e1 = m.outOff[row + 1];
                for (int e = m.outOff[row]; e < e1; ++e) v += exp(z + ((m.outW[e] + wa) + Wl[m.outDst[e]]));
              }
              if (diag)
                for (int c = 1; c < PL; ++c) {
                  const double pc = Br[c];
                  if (c == k || !(pc > -INFINITY)) continue;
                  const int tok = mm.colTok[c - 1];
                  const double *Ndc = Nd + (long long)c * S;
                  const int t1 = m.outOff[row + tok + 1];
                  for (int e = m.outOff[row + tok]; e < t1; ++e) v += exp(z + (((m.outW[e] + wa) + pc) + Ndc[m.outDst[e]]));
                }
            }
            rowpost_add(tab, bin0 + a, v, whole, lane, det);
          }
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

// Viterbi traceback over a materialised max lattice, one lane per pair: from the first plane that attains the score at
// Z[K][L][.][S-1] back to N[0][0][0][0], taking at every cell the first candidate (in the fill's order) whose value equals the cell;
// an emitting edge comes from the lowest plane k != c whose Z (match) or W (output-only) equals the edge's XZ / XW.  Blanks of
// either tape and repeat rows are not edges.  Edges go start -> end into the pair's slot (profile_pair_path_bound entries) with
// both coordinates at which each fired, as k_profile_two_traceback.  len = -1: no finite path, -2: the slot was too small, -3: no
// candidate matched (a corrupt matrix).  A candidate whose source cell lies outside the lattice is left out: it is -inf, and the
// cells on the path are finite.
template <bool ENV>
__global__ void k_profile_two_merge_traceback(DevMachine m, MergeMap mm, const typename TwoMergeLattice<true, ENV>::Desc *__restrict__ descs,
                                              typename TwoMergeLattice<true, ENV>::Tables t, int n,
                                              const double *__restrict__ logA, const double *__restrict__ logB,
                                              const double *__restrict__ pool, uint32_t *edges, int32_t *rows, int32_t *inRows, long long *len) {
  const int pair = blockIdx.x * blockDim.x + threadIdx.x;
  if (pair >= n) return;
  const auto pd = descs[pair];
  const int S = m.S, KK = m.K, C = m.nOut + 1, CA = m.nIn + 1, nC = mm.nCols, PL = nC + 1, K = pd.nIn, L = pd.nRows;
  const double *A = logA + pd.inBase * CA;
  const double *B = logB + pd.rowBase * PL;
  const TwoMergeLattice<true, ENV> lat(pd, t, const_cast<double *>(pool) + pd.cellBase, nullptr, S, PL);
  uint32_t *pe = edges + pd.pathBase;
  int32_t *pr = rows + pd.pathBase, *pi = inRows + pd.pathBase;
  int i = K, r = L, q = S - 1, layer = 2, p = 0;
  const long long cap = K + L + (long long)(K + L + 1) * (m.nLevF - 1);
  long long cnt = 0;
  {
    const double *Ze = lat.at(K, L, 2) + q;
    double best = Ze[0];
    for (int k = 1; k < PL; ++k)
      if (best < Ze[k * S]) { best = Ze[k * S]; p = k; }
    if (!(best > -INFINITY)) { len[pair] = -1; return; }
  }
  for (;;) {
    const double *Ai = A + (long long)max(i - 1, 0) * CA;      // row i - 1; read when i > 0
    int e = 0, found = -1, ni = i, nl = 1;
    if (layer == 2) {
      const double cur = lat.at(i, r, 2)[p * S + q];
      if (lat.at(i, r, 1)[p * S + q] == cur) { layer = 1; continue; }
      if (i > 0 && lat.inside(i - 1, r) && lat.at(i - 1, r, 2)[p * S + q] + Ai[0] == cur) { --i; continue; }
      len[pair] = -3; return;
    } else if (layer == 1) {
      const double *W = lat.at(i, r, 1) + p * S;
      const double cur = W[q];
      if (lat.at(i, r, 0)[p * S + q] == cur) { layer = 0; continue; }
      if (i > 0 && lat.inside(i - 1, r)) {
        const double *Zl = lat.at(i - 1, r, 2) + p * S;
        for (int a = 1; a <= m.nIn && found < 0; ++a) {
          const int row = q * KK + a * C;
          const double wa = Ai[a];
          e = m.inOff[row];
          for (const int e1 = m.inOff[row + 1]; e < e1; ++e)
            if ((Zl[m.inSrc[e]] + m.inW[e]) + wa == cur) { found = (int)m.inSrc[e]; ni = i - 1; nl = 2; break; }
        }
      }
      if (found < 0) {
        e = m.inOff[q * KK];
        for (const int e1 = m.inOff[q * KK + 1]; e < e1; ++e) {
          const int s = (int)m.inSrc[e];
          if (s < q && W[s] + m.inW[e] == cur) { found = s; break; }
        }
      }
      if (found < 0) { len[pair] = -3; return; }
      if (cnt >= cap) { len[pair] = -2; return; }
      pe[cnt] = m.inEid[e]; pr[cnt] = r; pi[cnt] = ni; ++cnt;
      i = ni; q = found; layer = nl;
    } else {
      if (r == 0) { if (i != 0 || q != 0 || p != 0) { len[pair] = -3; return; } break; }
      const bool up = lat.inside(i, r - 1);
      const double *Np = lat.at(i, r - 1, 0);      // (an address alone: read only where the cell is inside)
      const double cur = lat.at(i, r, 0)[p * S + q], w = B[(long long)(r - 1) * PL + p];
      if (p == 0) {
        int k = up ? 0 : PL;
        while (k < PL && !(Np[k * S + q] + w == cur)) ++k;
        if (k == PL) { len[pair] = -3; return; }
        p = k; --r;
        continue;
      }
      if (up && Np[p * S + q] + w == cur) { --r; continue; }
      const int tok = mm.colTok[p - 1];
      int from = -1;
      // the edge's exclusion value over the planes of V and the lowest plane that attains it
      auto excl = [&](const double *V, int s, int &kx) {
        double xs = V[s];
        kx = 0;
        for (int k = 1; k < PL; ++k)
          if (k != p && xs < V[k * S + s]) { xs = V[k * S + s]; kx = k; }
        return xs;
      };
      if (i > 0 && lat.inside(i - 1, r - 1)) {
        const double *Zd = lat.at(i - 1, r - 1, 2);
        for (int a = 1; a <= m.nIn && found < 0; ++a) {
          const int row = q * KK + a * C + tok;
          const double wa = Ai[a];
          e = m.inOff[row];
          for (const int e1 = m.inOff[row + 1]; e < e1; ++e) {
            int kx;
            const double xs = excl(Zd, (int)m.inSrc[e], kx);
            if (((xs + m.inW[e]) + wa) + w == cur) { found = (int)m.inSrc[e]; from = kx; ni = i - 1; nl = 2; break; }
          }
        }
      }
      if (found < 0 && up) {
        const double *Wu = lat.at(i, r - 1, 1);
        e = m.inOff[q * KK + tok];
        for (const int e1 = m.inOff[q * KK + tok + 1]; e < e1; ++e) {
          int kx;
          const double xs = excl(Wu, (int)m.inSrc[e], kx);
          if ((xs + m.inW[e]) + w == cur) { found = (int)m.inSrc[e]; from = kx; break; }
        }
      }
      if (found < 0) { len[pair] = -3; return; }
      if (cnt >= cap) { len[pair] = -2; return; }
      --r;
      pe[cnt] = m.inEid[e]; pr[cnt] = r; pi[cnt] = ni; ++cnt;
      i = ni; q = found; p = from; layer = nl;
    }
  }
  reverse_path(cnt, pe, pr, pi);
  len[pair] = cnt;
}

// every kernel that may get a ring in dynamic LDS (allow_sweep_lds, mb_profile_common.h)
static bool ptm_allow_lds(size_t lds) {
  static size_t ldsAllowed = 64 * 1024;
  return allow_sweep_lds(ldsAllowed, lds,
                         {(const void *)&k_profile_two_merge_fwd<MB_FORWARD, false, false>, (const void *)&k_profile_two_merge_fwd<MB_VITERBI, false, false>,
                          (const void *)&k_profile_two_merge_fwd<MB_FORWARD, true, false>, (const void *)&k_profile_two_merge_fwd<MB_VITERBI, true, false>,
                          (const void *)&k_profile_two_merge_bwd<false>,
                          (const void *)&k_profile_two_merge_fwd<MB_FORWARD, false, true>, (const void *)&k_profile_two_merge_fwd<MB_VITERBI, false, true>,
                          (const void *)&k_profile_two_merge_fwd<MB_FORWARD, true, true>, (const void *)&k_profile_two_merge_fwd<MB_VITERBI, true, true>,
                          (const void *)&k_profile_two_merge_bwd<true>},
                         "k_profile_two_merge: raising the LDS limit");
}

// The launchers: each sweep once over a form of the lattice, and the two overloads of the header that name one.
template <bool ENV>
static int ptm_fwd(const mb_machine *m, MergeMap mm, int mode, bool mat, const typename TwoMergeLattice<true, ENV>::Desc *d, typename TwoMergeLattice<true, ENV>::Tables t,
                   int n, size_t lds, long long maxItems, const double *logA, const double *logB, double *pool, double *scratch, double *loglike, hipStream_t st) {
  if (n <= 0) return 0;
  if (!ptm_allow_lds(lds)) return 1;
  const dim3 g(n), b(sweep_threads(maxItems));
  if (mode == MB_VITERBI) {
    if (mat) k_profile_two_merge_fwd<MB_VITERBI, true, ENV><<<g, b, lds, st>>>(m->dev, mm, d, t, logA, logB, pool, scratch, loglike);
    else k_profile_two_merge_fwd<MB_VITERBI, false, ENV><<<g, b, lds, st>>>(m->dev, mm, d, t, logA, logB, pool, scratch, loglike);
  } else {
    if (mat) k_profile_two_merge_fwd<MB_FORWARD, true, ENV><<<g, b, lds, st>>>(m->dev, mm, d, t, logA, logB, pool, scratch, loglike);
    else k_profile_two_merge_fwd<MB_FORWARD, false, ENV><<<g, b, lds, st>>>(m->dev, mm, d, t, logA, logB, pool, scratch, loglike);
  }
  return hip_ok(hipGetLastError(), ENV ? "k_profile_two_merge_env_fwd" : "k_profile_two_merge_fwd") ? 0 : 1;
}
int launch_profile_two_merge_fwd(const mb_machine *m, MergeMap mm, int mode, bool mat, const PairProfDesc *d, int n, size_t lds,
                                 long long maxItems, const double *logA, const double *logB, double *pool, double *scratch,
                                 double *loglike, hipStream_t st) {
  return ptm_fwd<false>(m, mm, mode, mat, d, {}, n, lds, maxItems, logA, logB, pool, scratch, loglike, st);
}
int launch_profile_two_merge_fwd(const mb_machine *m, MergeMap mm, int mode, bool mat, const TwoEnvDesc *d, const TwoEnvTables &t, int n, size_t lds,
                                 long long maxItems, const double *logA, const double *logB, double *pool, double *scratch,
                                 double *loglike, hipStream_t st) {
  return ptm_fwd<true>(m, mm, mode, mat, d, t, n, lds, maxItems, logA, logB, pool, scratch, loglike, st);
}

template <bool ENV>
static int ptm_bwd(const mb_machine *m, MergeMap mm, const typename TwoMergeLattice<true, ENV>::Desc *d, typename TwoMergeLattice<true, ENV>::Tables t, int n, size_t lds,
                   long long maxItems, const double *logA, const double *logB, double *pool, double *scratch, double *loglike, hipStream_t st) {
  if (n <= 0) return 0;
  if (!ptm_allow_lds(lds)) return 1;
  k_profile_two_merge_bwd<ENV><<<dim3(n), dim3(sweep_threads(maxItems)), lds, st>>>(m->dev, mm, d, t, logA, logB, pool, scratch, loglike);
  return hip_ok(hipGetLastError(), ENV ? "k_profile_two_merge_env_bwd" : "k_profile_two_merge_bwd") ? 0 : 1;
}
int launch_profile_two_merge_bwd(const mb_machine *m, MergeMap mm, const PairProfDesc *d, int n, size_t lds, long long maxItems,
                                 const double *logA, const double *logB, double *pool, double *scratch, double *loglike, hipStream_t st) {
  return ptm_bwd<false>(m, mm, d, {}, n, lds, maxItems, logA, logB, pool, scratch, loglike, st);
}
int launch_profile_two_merge_bwd(const mb_machine *m, MergeMap mm, const TwoEnvDesc *d, const TwoEnvTables &t, int n, size_t lds, long long maxItems,
                                 const double *logA, const double *logB, double *pool, double *scratch, double *loglike, hipStream_t st) {
  return ptm_bwd<true>(m, mm, d, t, n, lds, maxItems, logA, logB, pool, scratch, loglike, st);
}

template <bool ENV>
static int ptm_counts(const mb_machine *m, MergeMap mm, const typename TwoMergeLattice<true, ENV>::Desc *d, typename TwoMergeLattice<true, ENV>::Tables t, int n,
                      int groupsPerPair, const double *logA, const double *logB, const double *fwdPool, const double *bwdPool, double *counts, hipStream_t st) {
  if (n <= 0 || m->nTrans <= 0) return 0;
  k_profile_two_merge_counts<ENV><<<dim3((unsigned)((long long)n * groupsPerPair)), dim3(256), 0, st>>>(
      m->dev, mm, d, t, groupsPerPair, logA, logB, fwdPool, bwdPool, m->nTrans, counts, g_deterministic ? 1 : 0);
  return hip_ok(hipGetLastError(), ENV ? "k_profile_two_merge_env_counts" : "k_profile_two_merge_counts") ? 0 : 1;
}
int launch_profile_two_merge_counts(const mb_machine *m, MergeMap mm, const PairProfDesc *d, int n, int groupsPerPair, const double *logA,
                                    const double *logB, const double *fwdPool, const double *bwdPool, double *counts, hipStream_t st) {
  return ptm_counts<false>(m, mm, d, {}, n, groupsPerPair, logA, logB, fwdPool, bwdPool, counts, st);
}
int launch_profile_two_merge_counts(const mb_machine *m, MergeMap mm, const TwoEnvDesc *d, const TwoEnvTables &t, int n, int groupsPerPair, const double *logA,
                                    const double *logB, const double *fwdPool, const double *bwdPool, double *counts, hipStream_t st) {
  return ptm_counts<true>(m, mm, d, t, n, groupsPerPair, logA, logB, fwdPool, bwdPool, counts, st);
}

template <bool ENV>
static int ptm_rowpost(const mb_machine *m, MergeMap mm, int axis, const typename TwoMergeLattice<true, ENV>::Desc *d, typename TwoMergeLattice<true, ENV>::Tables t, int n,
                       int groupsPerPair, int tabMax, const double *logA, const double *logB, const double *fwdPool, const double *bwdPool,
                       const double *loglike, double *post, hipStream_t st) {
  if (n <= 0) return 0;
  const dim3 g((unsigned)((long long)n * groupsPerPair)), b(ROWPOST_THREADS);
  const int det = g_deterministic ? 1 : 0;
  if (axis) k_profile_two_merge_rowpost<1, ENV><<<g, b, 0, st>>>(m->dev, mm, d, t, groupsPerPair, logA, logB, fwdPool, bwdPool, loglike, post, tabMax, det);
  else k_profile_two_merge_rowpost<0, ENV><<<g, b, 0, st>>>(m->dev, mm, d, t, groupsPerPair, logA, logB, fwdPool, bwdPool, loglike, post, tabMax, det);
  return hip_ok(hipGetLastError(), ENV ? "k_profile_two_merge_env_rowpost" : "k_profile_two_merge_rowpost") ? 0 : 1;
}
int launch_profile_two_merge_rowpost(const mb_machine *m, MergeMap mm, int axis, const PairProfDesc *d, int n, int groupsPerPair, int tabMax,
                                     const double *logA, const double *logB, const double *fwdPool, const double *bwdPool,
                                     const double *loglike, double *post, hipStream_t st) {
  return ptm_rowpost<false>(m, mm, axis, d, {}, n, groupsPerPair, tabMax, logA, logB, fwdPool, bwdPool, loglike, post, st);
}
int launch_profile_two_merge_rowpost(const mb_machine *m, MergeMap mm, int axis, const TwoEnvDesc *d, const TwoEnvTables &t, int n, int groupsPerPair, int tabMax,
                                     const double *logA, const double *logB, const double *fwdPool, const double *bwdPool,
                                     const double *loglike, double *post, hipStream_t st) {
  return ptm_rowpost<true>(m, mm, axis, d, t, n, groupsPerPair, tabMax, logA, logB, fwdPool, bwdPool, loglike, post, st);
}

template <bool ENV>
static int ptm_traceback(const mb_machine *m, MergeMap mm, const typename TwoMergeLattice<true, ENV>::Desc *d, typename TwoMergeLattice<true, ENV>::Tables t, int n,
                         const double *logA, const double *logB, const double *pool, uint32_t *edges, int32_t *rows, int32_t *inRows, long long *len, hipStream_t st) {
  if (n <= 0) return 0;
  k_profile_two_merge_traceback<ENV><<<(n + 63) / 64, 64, 0, st>>>(m->dev, mm, d, t, n, logA, logB, pool, edges, rows, inRows, len);
  return hip_ok(hipGetLastError(), ENV ? "k_profile_two_merge_env_traceback" : "k_profile_two_merge_traceback") ? 0 : 1;
}
int launch_profile_two_merge_traceback(const mb_machine *m, MergeMap mm, const PairProfDesc *d, int n, const double *logA,
                                       const double *logB, const double *pool, uint32_t *edges, int32_t *rows, int32_t *inRows,
                                       long long *len, hipStream_t st) {
  return ptm_traceback<false>(m, mm, d, {}, n, logA, logB, pool, edges, rows, inRows, len, st);
}
int launch_profile_two_merge_traceback(const mb_machine *m, MergeMap mm, const TwoEnvDesc *d, const TwoEnvTables &t, int n, const double *logA,
                                       const double *logB, const double *pool, uint32_t *edges, int32_t *rows, int32_t *inRows,
                                       long long *len, hipStream_t st) {
  return ptm_traceback<true>(m, mm, d, t, n, logA, logB, pool, edges, rows, inRows, len, st);
}

}  // namespace mb
