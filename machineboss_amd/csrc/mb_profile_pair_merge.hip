// mb_profile_pair_merge.hip -- Forward / Backward / Viterbi / posterior counts / row posteriors of a machine WITH an input alphabet,
// run on a known input sequence x[1..I] against a CTC-MERGED profile of L rows: the semantics of
// compose(M, transpose(CSVProfile::mergingMachine())) on input x with an empty output, restated in docs/profile_tapes.md ("Pairs
// against a merged profile"):
//
//   X[i][r][c][s] = (+)_{k != c} W[i][r][k][s]                                                          (the exclusion vector)
//   N[i][r][0][d] = [i = 0, r = 0, d = 0]  (+)  (+)_p (N[i][r-1][p][d] + P[r-1][0])                      (blank; r > 0)
//   N[i][r][c][d] = (N[i][r-1][c][d] + P[r-1][c])                                                        (repeat; r > 0)
//                   (+) sum_{t: s->d, in = x_i, out = colTok[c]} X[i-1][r-1][c][s] + w_t + P[r-1][c]      (match; i > 0, r > 0)
//                   (+) sum_{t: s->d, in = eps, out = colTok[c]} X[i][r-1][c][s]   + w_t + P[r-1][c]      (output-only; r > 0)
//   W[i][r][p][d] = N[i][r][p][d]
//                   (+) sum_{t: s->d, in = x_i, out = eps} W[i-1][r][p][s] + w_t                          (input-only; same plane)
//                   (+) sum_{silent t: s->d, s < d}        W[i][r][p][s]   + w_t                          (silent levels, per plane)
//   loglike       = (+)_p W[I][L][p][S-1]
//
// The anti-diagonal sweep of mb_profile_pair.hip with the plane axis and the exclusion vector of mb_profile_merge.hip.  One
// workgroup per pair; the work items of a diagonal are (cell, plane, state) and the lanes stride over them.  Per diagonal: one phase
// for N and the non-silent part of W and a barrier, one barrier per silent level, and one phase and barrier that forms X, so that no
// edge loop runs over planes -- (I + L + 1)(nLevF + 1) barriers per pair.  The rolling sweeps keep a ring of three diagonals of N, W
// and X, 3 (3 nCols + 2)(min(I, L) + 1) S doubles, in LDS when that fits 160 KiB, else in the pair's slice of a global scratch
// buffer; the materialised ones keep only X there.  Cells are fp64, the sums the exact log-sum-exp.
//
// Every kernel is written once over PairMergeLattice, which says which cells exist and where they live: its full form, the whole
// rectangle, or its envelope form, the cells of an envelope (docs/profile_tapes.md, "Pairs against a merged profile under an
// envelope"); the index rules of both are those of mb_profile_lattice.h.  Every plane of both layers of a cell outside the envelope
// is -inf, and so are its X and T, so a neighbour outside is not read; the recurrence, the candidate order and the sums are the same
// text for both.
#include "mb_profile_common.h"
#include "mb_profile_pair_merge.h"

namespace mb {

size_t profile_pair_merge_lds_bytes(int S, int nCols, long long nIn, long long nRows, bool mat) {
  const double b = (double)profile_pair_merge_ring(S, nCols, nIn, nRows, mat) * sizeof(double);
  return b <= (double)SWEEP_LDS_MAX ? (size_t)b : 0;
}

size_t profile_pair_merge_env_lds_bytes(int S, int nCols, long long M, bool mat) {
  const double b = (double)profile_pair_merge_env_ring(S, nCols, M, mat) * sizeof(double);
  return b <= (double)SWEEP_LDS_MAX ? (size_t)b : 0;
}

// Where cell (i, r) lives: the cells of mb_profile_lattice.h, RectCells or EnvCells, and this family's layout.  nw(i, r, layer): its
// N (layer 0) or W (layer 1), nCols + 1 planes of S states -- the materialised lattice of mb_profile_pair_merge.h (under an envelope
// the compact one, cells[(((off[r] + i - inStart[r]) * 2 + layer) * (nCols + 1) + p) * S + q]), or the ring.  xv(i, r): its exclusion
// vectors, column c at (c - 1) * S -- always in the ring, beside N and W when rolling.
template <class Cells, bool MAT>
struct PairMergeStore : Cells {
  using Desc = std::conditional_t<Cells::ENV, PairEnvDesc, PairProfDesc>;
  using Tables = std::conditional_t<Cells::ENV, PairEnvTables, NoTables>;
  double *pool, *ring;
  int S, PL;
  __device__ __forceinline__ PairMergeStore(const Desc &pd, const Tables &t, double *pool, double *ring, int S, int PL)
      : Cells(lattice_cells(pd, t)), pool(pool), ring(ring), S(S), PL(PL) {}
  __device__ __forceinline__ double *nw(int i, int r, int layer) const {
    if (MAT) return pool + (this->index(i, r) * 2 + layer) * PL * S;
    return ring + (this->slot(i, r) * (3 * PL - 1) + layer * PL) * S;
  }
  __device__ __forceinline__ double *xv(int i, int r) const {
    if (MAT) return ring + this->slot(i, r) * (PL - 1) * S;
    return ring + (this->slot(i, r) * (3 * PL - 1) + 2 * PL) * S;
  }
};
template <bool MAT, bool ENV>
using PairMergeLattice = PairMergeStore<std::conditional_t<ENV, EnvCells, RectCells>, MAT>;

// Forward (MODE = MB_FORWARD) or Viterbi (MB_VITERBI) sweep.  MAT: every N and W cell into pool (layout of mb_profile_pair_merge.h)
// and only X in the ring, else rolling.  Viterbi keeps the FIRST maximum: N[.][.][0] takes the planes ascending; N[.][.][c] the
// repeat first, then the match edges in `incoming` order, then the output-only edges in `incoming` order; W takes N (no move)
// first, then the input-only edges, then the silent edges, each in `incoming` order; X and the end the planes ascending -- the
// order k_profile_pair_merge_traceback re-enumerates.  A neighbour outside the lattice is -inf and is not read: (i, r - 1) feeds the
// blank over all planes, the repeat and X of the output-only edges, (i - 1, r - 1) X of the match edges, (i - 1, r) W of the
// input-only edges.
template <int MODE, bool MAT, bool ENV>
__global__ __launch_bounds__(SWEEP_THREADS) void k_profile_pair_merge_fwd(DevMachine m, MergeMap mm, const typename PairMergeLattice<MAT, ENV>::Desc *__restrict__ descs,
                                                                          typename PairMergeLattice<MAT, ENV>::Tables t,
                                                                          const int *__restrict__ inTok, const double *__restrict__ logP,
                                                                          double *pool, double *scratch, double *__restrict__ loglike) {
  extern __shared__ double ppm_sh[];
  const auto pd = descs[blockIdx.x];
  const int S = m.S, K = m.K, C = m.nOut + 1, nC = mm.nCols, PL = nC + 1, I = pd.nIn, L = pd.nRows;
  const int *x = inTok + pd.inBase;
  const double *P = logP + pd.rowBase * PL;
  const PairMergeLattice<MAT, ENV> lat(pd, t, MAT ? pool + pd.cellBase : nullptr, pd.ringBase < 0 ? ppm_sh : scratch + pd.ringBase, S, PL);
  const int PS = PL * S;
  for (int d = 0; d <= I + L; ++d) {
    int ilo, nCells;
    lat.diag(d, ilo, nCells);
    const int nItems = nCells * PS;
    for (int it = threadIdx.x; it < nItems; it += blockDim.x) {
      const int c = it / PS, pq = it - c * PS, p = pq / S, q = pq - p * S, i = ilo + c, r = d - i;
      const int xRow = i > 0 ? q * K + x[i - 1] * C : 0;     // CSR rows q*K + key(x_i, o), o = 0..nOut: contiguous
      double acc = (d == 0 && pq == 0) ? 0.0 : -INFINITY;
      if (r > 0) {
        const double w = P[(long long)(r - 1) * PL + p];
        const bool up = lat.inside(i, r - 1);
        const double *Np = lat.nw(i, r - 1, 0);      // (an address alone: read only where the cell is inside)
        if (p == 0) {
          if (up) {
            acc = Np[q] + w;
            for (int k = 1; k < PL; ++k) acc = red<MODE>(acc, Np[k * S + q] + w);
          }
        } else if (w > -INFINITY) {                          // (a column the row rules out is skipped as a whole)
          const int tok = mm.colTok[p - 1];
          if (up) acc = Np[p * S + q] + w;
          if (i > 0 && lat.inside(i - 1, r - 1)) {
            const double *Xd = lat.xv(i - 1, r - 1) + (p - 1) * S;
            const int a1 = m.inOff[xRow + tok + 1];
            for (int a = m.inOff[xRow + tok]; a < a1; ++a) acc = red<MODE>(acc, (Xd[m.inSrc[a]] + m.inW[a]) + w);
          }
          if (up) {
            const double *Xu = lat.xv(i, r - 1) + (p - 1) * S;
            const int a1 = m.inOff[q * K + tok + 1];
            for (int a = m.inOff[q * K + tok]; a < a1; ++a) acc = red<MODE>(acc, (Xu[m.inSrc[a]] + m.inW[a]) + w);
          }
        }
      }
      lat.nw(i, r, 0)[pq] = acc;
      if (i > 0 && lat.inside(i - 1, r)) {
        const double *Wl = lat.nw(i - 1, r, 1) + p * S;
        const int a1 = m.inOff[xRow + 1];
        for (int a = m.inOff[xRow]; a < a1; ++a) acc = red<MODE>(acc, Wl[m.inSrc[a]] + m.inW[a]);
      }
      lat.nw(i, r, 1)[pq] = acc;
    }
    __syncthreads();
    for (int lev = 1; lev < m.nLevF; ++lev) {      // (level 0 has no silent edge coming in: its W is complete)
      const int l0 = m.levFOff[lev], ns = m.levFOff[lev + 1] - l0;
      const int PN = PL * ns, nLevItems = nCells * PN;
      for (int it = threadIdx.x; it < nLevItems; it += blockDim.x) {
        const int c = it / PN, pj = it - c * PN, p = pj / ns, q = m.levFState[l0 + (pj - p * ns)], i = ilo + c;
        double *Wc = lat.nw(i, d - i, 1) + p * S;
        double acc = Wc[q];
        const int a1 = m.inOff[q * K + 1];
        for (int a = m.inOff[q * K]; a < a1; ++a) {
          const int s = (int)m.inSrc[a];
          if (s >= q) continue;                       // as the token sweeps: a silent self-loop never fires
          acc = red<MODE>(acc, Wc[s] + m.inW[a]);
        }
        Wc[q] = acc;
      }
      __syncthreads();
    }
    if (d < I + L) {
      const int XS = nC * S, nXItems = nCells * XS;
      for (int it = threadIdx.x; it < nXItems; it += blockDim.x) {
        const int c = it / XS, cs = it - c * XS, col = cs / S + 1, s = cs - (col - 1) * S, i = ilo + c;
        const double *Wc = lat.nw(i, d - i, 1) + s;
        double acc = Wc[0];                             // plane 0 is never the excluded one
        for (int k = 1; k < PL; ++k)
          if (k != col) acc = red<MODE>(acc, Wc[k * S]);
        lat.xv(i, d - i)[cs] = acc;
      }
      __syncthreads();
    }
  }
  if (threadIdx.x == 0) {
    const double *We = lat.nw(I, L, 1) + S - 1;      // (an envelope is connected: (0, 0) and (I, L) are inside)
    double acc = We[0];
    for (int p = 1; p < PL; ++p) acc = red<MODE>(acc, We[p * S]);
    loglike[blockIdx.x] = acc;
  }
}

// Materialised Backward sweep, layer 0 = NB ("from the arrived stage"), layer 1 = WB ("from the waiting stage"):
//   T[i][r][c][s]  = sum_{t: s->d, in = x_{i+1}, out = colTok[c]} (w_t + P[r][c]) + NB[i+1][r+1][c][d]     (i < I, r < L)
//                    (+) sum_{t: s->d, in = eps, out = colTok[c]} (w_t + P[r][c]) + NB[i][r+1][c][d]       (r < L)
//   WB[i][r][k][s] = [i = I, r = L, s = S-1]  (+)  (+)_{c != k} T[i][r][c][s]
//                    (+) sum_{t: in = x_{i+1}, out = eps} w_t + WB[i+1][r][k][d]                           (i < I)
//                    (+) sum_{silent t, s < d}            w_t + WB[i][r][k][d]
//   NB[i][r][k][s] = WB[i][r][k][s] (+) (P[r][0] + NB[i][r+1][0][s]) (+) [k >= 1](P[r][k] + NB[i][r+1][k][s])   (r < L)
//   loglike        = NB[0][0][0][0]
// Anti-diagonals from I + L down.  T, everything that leaves (i, r, s) through column c, is formed once per diagonal over (cell,
// column, state) -- the mirror of the Forward's X -- so the edge loops do not run over planes; it lives in the ring (one diagonal of
// it, the cell by its place on the diagonal).  A state's WB is final once its backward level has run; the item that finishes it
// writes its NB.  A successor cell outside the lattice contributes nothing.
template <bool ENV>
__global__ __launch_bounds__(SWEEP_THREADS) void k_profile_pair_merge_bwd(DevMachine m, MergeMap mm, const typename PairMergeLattice<true, ENV>::Desc *__restrict__ descs,
                                                                          typename PairMergeLattice<true, ENV>::Tables t,
                                                                          const int *__restrict__ inTok, const double *__restrict__ logP,
                                                                          double *pool, double *scratch, double *__restrict__ loglike) {
  extern __shared__ double ppm_sh[];
  const auto pd = descs[blockIdx.x];
  const int S = m.S, K = m.K, C = m.nOut + 1, nC = mm.nCols, PL = nC + 1, I = pd.nIn, L = pd.nRows;
  const int *x = inTok + pd.inBase;
  const double *P = logP + pd.rowBase * PL;
  const PairMergeLattice<true, ENV> lat(pd, t, pool + pd.cellBase, nullptr, S, PL);
  double *T = pd.ringBase < 0 ? ppm_sh : scratch + pd.ringBase;       // T[(cell on the diagonal * nCols + c - 1) * S + s]
  const int PS = PL * S, XS = nC * S;
  for (int d = I + L; d >= 0; --d) {
    int ilo, nCells;
    lat.diag(d, ilo, nCells);
    if (d < I + L) {
      const int nTItems = nCells * XS;
      for (int it = threadIdx.x; it < nTItems; it += blockDim.x) {
        const int c = it / XS, cs = it - c * XS, col = cs / S + 1, s = cs - (col - 1) * S, i = ilo + c, r = d - i;
        double v = -INFINITY;
        if (r < L) {
          const double pc = P[(long long)r * PL + col];
          if (pc > -INFINITY) {
            const int tok = mm.colTok[col - 1];
            if (i < I && lat.inside(i + 1, r + 1)) {
              const double *Nd = lat.nw(i + 1, r + 1, 0) + col * S;
              const int xRow = s * K + x[i] * C;
              const int a1 = m.outOff[xRow + tok + 1];
              for (int a = m.outOff[xRow + tok]; a < a1; ++a) v = lse2_exact(v, (m.outW[a] + pc) + Nd[m.outDst[a]]);
            }
            if (lat.inside(i, r + 1)) {
              const double *Nu = lat.nw(i, r + 1, 0) + col * S;
              const int a1 = m.outOff[s * K + tok + 1];
              for (int a = m.outOff[s * K + tok]; a < a1; ++a) v = lse2_exact(v, (m.outW[a] + pc) + Nu[m.outDst[a]]);
            }
          }
        }
        T[it] = v;
      }
      __syncthreads();
    }
    const int nItems = nCells * PS;
    for (int it = threadIdx.x; it < nItems; it += blockDim.x) {
      const int c = it / PS, ks = it - c * PS, k = ks / S, s = ks - k * S, i = ilo + c, r = d - i;
      double v = (d == I + L && s == S - 1) ? 0.0 : -INFINITY;
      if (r < L) {
        const double *Tc = T + (long long)c * XS + s;
        for (int col = 1; col < PL; ++col)
          if (col != k) v = lse2_exact(v, Tc[(col - 1) * S]);
      }
      if (i < I && lat.inside(i + 1, r)) {
        const double *Wl = lat.nw(i + 1, r, 1) + k * S;
        const int xRow = s * K + x[i] * C;
        const int a1 = m.outOff[xRow + 1];
        for (int a = m.outOff[xRow]; a < a1; ++a) v = lse2_exact(v, Wl[m.outDst[a]] + m.outW[a]);
      }
      lat.nw(i, r, 1)[ks] = v;
      if (r < L && lat.inside(i, r + 1)) {
        const double *Nn = lat.nw(i, r + 1, 0), *Pr = P + (long long)r * PL;
        v = lse2_exact(v, Pr[0] + Nn[s]);
        if (k) v = lse2_exact(v, Pr[k] + Nn[ks]);
      }
      lat.nw(i, r, 0)[ks] = v;
    }
    __syncthreads();
    for (int lev = 1; lev < m.nLevB; ++lev) {
      const int l0 = m.levBOff[lev], ns = m.levBOff[lev + 1] - l0;
      const int PN = PL * ns, nLevItems = nCells * PN;
      for (int it = threadIdx.x; it < nLevItems; it += blockDim.x) {
        const int c = it / PN, kj = it - c * PN, k = kj / ns, s = m.levBState[l0 + (kj - k * ns)], i = ilo + c, r = d - i;
        double *Wc = lat.nw(i, r, 1) + k * S;
        double v = Wc[s];
        const int a1 = m.outOff[s * K + 1];
        for (int a = m.outOff[s * K]; a < a1; ++a) {
          const int t = (int)m.outDst[a];
          if (t <= s) continue;
          v = lse2_exact(v, Wc[t] + m.outW[a]);
        }
        Wc[s] = v;
        if (r < L && lat.inside(i, r + 1)) {
          const double *Nn = lat.nw(i, r + 1, 0), *Pr = P + (long long)r * PL;
          v = lse2_exact(v, Pr[0] + Nn[s]);
          if (k) v = lse2_exact(v, Pr[k] + Nn[k * S + s]);
        }
        lat.nw(i, r, 0)[k * S + s] = v;
      }
      __syncthreads();
    }
  }
  if (threadIdx.x == 0) loglike[blockIdx.x] = lat.nw(0, 0, 0)[0];
}

// Posterior counts.  With both lattices in memory every (cell, plane, edge) term is independent:
//   count[t] += exp(W_F[i][r][k][s] - LL + term_t), term_t the edge's summand of WB[i][r][k][s] above (through T for the emitting
//   edges: every column c != k),
// so the sweep is a flat grid over (pair, group of the pair, (cell, plane, state)), accumulated by CountsAcc (mb_profile_common.h).
// A pair whose likelihood is -inf adds nothing.  The cells are the lattice's own count (under an envelope the compact index, its row
// found by bisection).
template <bool ENV>
__global__ __launch_bounds__(256) void k_profile_pair_merge_counts(DevMachine m, MergeMap mm, const typename PairMergeLattice<true, ENV>::Desc *__restrict__ descs,
                                                                   typename PairMergeLattice<true, ENV>::Tables t, int groupsPerPair, const int *__restrict__ inTok,
                                                                   const double *__restrict__ logP, const double *__restrict__ fwdPool,
                                                                   const double *__restrict__ bwdPool, long long nTrans,
                                                                   double *__restrict__ counts, int det) {
  __shared__ double lcount[COUNTS_LDS_MAX];
  const CountsAcc acc(lcount, counts, nTrans, det);
  const int pair = blockIdx.x / groupsPerPair, group = blockIdx.x % groupsPerPair;
  const auto pd = descs[pair];
  const int S = m.S, K = m.K, C = m.nOut + 1, nC = mm.nCols, PL = nC + 1, I = pd.nIn, L = pd.nRows;
  const int *x = inTok + pd.inBase;
  const double *P = logP + pd.rowBase * PL;
  const PairMergeLattice<true, ENV> F(pd, t, const_cast<double *>(fwdPool) + pd.cellBase, nullptr, S, PL),
      B(pd, t, const_cast<double *>(bwdPool) + pd.cellBase, nullptr, S, PL);
  double LL;
  {
    const double *We = F.nw(I, L, 1) + S - 1;
    LL = We[0];
    for (int p = 1; p < PL; ++p) LL = lse2_exact(LL, We[p * S]);
  }
  if (LL > -INFINITY) {
    const long long PS = (long long)PL * S, nItems = F.cells() * PS;
    for (long long idx = (long long)group * blockDim.x + threadIdx.x; idx < nItems; idx += (long long)groupsPerPair * blockDim.x) {
      const long long cell = idx / PS;
      const int ks = (int)(idx - cell * PS), k = ks / S, s = ks - k * S;
      int i, r;
      F.cell(cell, i, r);
      const double f = F.nw(i, r, 1)[ks] - LL;
      if (!(f > -INFINITY)) continue;
      const int xRow = i < I ? s * K + x[i] * C : 0;
      if (r < L) {
        const double *Pr = P + (long long)r * PL;
        const bool across = i < I && B.inside(i + 1, r + 1), up = B.inside(i, r + 1);
        for (int col = 1; col < PL; ++col) {
          const double pc = Pr[col];
          if (col == k || !(pc > -INFINITY)) continue;
          const int tok = mm.colTok[col - 1];
          if (across) {
            const double *Nd = B.nw(i + 1, r + 1, 0) + col * S;
            const int a1 = m.outOff[xRow + tok + 1];
            for (int a = m.outOff[xRow + tok]; a < a1; ++a) acc.add(m.outEid[a], exp(f + ((m.outW[a] + pc) + Nd[m.outDst[a]])));
          }
          if (up) {
            const double *Nu = B.nw(i, r + 1, 0) + col * S;
            const int a1 = m.outOff[s * K + tok + 1];
            for (int a = m.outOff[s * K + tok]; a < a1; ++a) acc.add(m.outEid[a], exp(f + ((m.outW[a] + pc) + Nu[m.outDst[a]])));
          }
        }
      }
      if (i < I && B.inside(i + 1, r)) {
        const double *Wl = B.nw(i + 1, r, 1) + k * S;
        const int a1 = m.outOff[xRow + 1];
        for (int a = m.outOff[xRow]; a < a1; ++a) acc.add(m.outEid[a], exp(f + (Wl[m.outDst[a]] + m.outW[a])));
      }
      const double *Wc = B.nw(i, r, 1) + k * S;
      const int a1 = m.outOff[s * K + 1];
      for (int a = m.outOff[s * K]; a < a1; ++a) {
        const int t = (int)m.outDst[a];
        if (t <= s) continue;
        acc.add(m.outEid[a], exp(f + (Wc[t] + m.outW[a])));
      }
    }
  }
  acc.flush();
}

// Row posteriors: post[(rowBase + r) * (nCols + 1) + c] = the posterior probability that row r of the pair's merged profile was
// consumed as column c (0: the blank), the gradient of the log-likelihood in P[r][c] (docs/profile_tapes.md, "Row posteriors of
// pairs against a merged profile"):
//   post[r][0] = sum_i sum_p sum_s exp((N_F[i][r][p][s] - LL) + (P[r][0] + NB[i][r+1][0][s]))
//   post[r][c] = sum_i sum_s exp((N_F[i][r][c][s] - LL) + (P[r][c] + NB[i][r+1][c][s]))                     (the repeat)
//              + the emitting terms of k_profile_pair_merge_counts above, binned by (row, column) instead of by transition.
// The scheme is the one of k_profile_pair_rowpost (mb_profile_pair.hip) with the plane axis of k_profile_rowpost<true>
// (mb_profile_post.hip).  The work items are (row, cell of the row, plane, state) in that order and a workgroup owns whole rows:
// blocks of profile_pair_rowpost_rows rows, dealt round robin to the pair's groups.  An item (r, i, k, s) adds the blank term out of
// its plane, at k >= 1 the repeat term into column k, and at every other column c whose P[r][c] is finite the match edges of
// (s, x_{i+1}, colTok[c]) into NB[i+1][r+1][c] and the output-only edges of (s, colTok[c]) into NB[i][r+1][c], one CSR row each,
// summed in a register: the sum over k != c runs over the items, the exclusion vector of the Forward sweep is not needed.  Where all
// 64 lanes of the wavefront hold items of one row the lane sums are reduced across the lanes and one lane adds the result to the
// workgroup's LDS table (rows of the block x (nCols + 1)), else every lane adds its own (rowpost_add, mb_profile_common.h).  The
// table is then stored with plain stores: every bin has one writing workgroup, so there is no global atomic and nothing to clear
// beforehand.  A row of more than tabMax columns is summed in its global bins instead, cleared by the workgroup that owns it.  A pair
// whose likelihood is -inf gets zeros by the same stores.  loglike: the Forward sweep's, per pair of the launch.
// det: a lane sum is turned into 64-bit fixed point at 2^-36 (mb_internal.h) before it meets another; post then holds the integers.
// The rows are walked through the lattice's lineFirst<0> / lineCell<0>: under an envelope row r has (inEnd[r] - inStart[r]) (nCols + 1) S
// items, and the cells (i, r + 1) and (i + 1, r + 1) are asked inside() before they are read.  Every bin of every row is still
// written, so a row all of whose terms are dead gets zeros.
template <bool ENV>
__global__ __launch_bounds__(ROWPOST_THREADS) void k_profile_pair_merge_rowpost(DevMachine m, MergeMap mm, const typename PairMergeLattice<true, ENV>::Desc *__restrict__ descs,
                                                                                typename PairMergeLattice<true, ENV>::Tables t, int groupsPerPair, const int *__restrict__ inTok,
                                                                                const double *__restrict__ logP, const double *__restrict__ fwdPool,
                                                                                const double *__restrict__ bwdPool, const double *__restrict__ loglike,
                                                                                double *post, int tabMax, int det) {
  __shared__ double ltab[ROWPOST_LDS_MAX];
  const int pair = blockIdx.x / groupsPerPair, group = blockIdx.x % groupsPerPair;
  const auto pd = descs[pair];
  const int S = m.S, K = m.K, C = m.nOut + 1, nC = mm.nCols, PL = nC + 1, I = pd.nIn, L = pd.nRows;
  if (L == 0) return;
  const int *x = inTok + pd.inBase;
  const double *P = logP + pd.rowBase * PL;
  const PairMergeLattice<true, ENV> F(pd, t, const_cast<double *>(fwdPool) + pd.cellBase, nullptr, S, PL),
      B(pd, t, const_cast<double *>(bwdPool) + pd.cellBase, nullptr, S, PL);
  const double LL = loglike[pair];
  const long long PS = (long long)PL * S;
  const int R = profile_pair_rowpost_rows(F.cells() * PL, S, L, PL, tabMax);
  const bool useLds = PL <= tabMax;
  const int lane = threadIdx.x & 63;
  for (long long rb = (long long)group * R; rb < L; rb += (long long)groupsPerPair * R) {
    const int r0 = (int)rb, r1 = (int)min((long long)L, rb + R), nBins = (r1 - r0) * PL;
    double *out = post + (pd.rowBase + r0) * PL;
    double *tab = useLds ? ltab : out;
    for (int e = threadIdx.x; e < nBins; e += blockDim.x) tab[e] = 0.0;      // (the fixed point's zero has the same bits)
    if (!useLds) __threadfence();
    __syncthreads();
    if (LL > -INFINITY) {
      const long long c0 = F.template lineFirst<0>(r0), nItems = (F.template lineFirst<0>(r1) - c0) * PS;
      for (long long base = threadIdx.x - lane; base < nItems; base += blockDim.x) {      // (a wavefront stays whole in here)
        const long long idx = base + lane;
        const bool valid = idx < nItems;
        int r = r0, i = 0, k = 0, s = 0, ks = 0;
        double f = -INFINITY, n = -INFINITY;
        if (valid) {
          const long long cell = idx / PS;
          ks = (int)(idx - cell * PS);
          F.template lineCell<0>(c0 + cell, i, r);
          k = ks / S;
          s = ks - k * S;
          n = F.nw(i, r, 0)[ks] - LL;
          f = F.nw(i, r, 1)[ks] - LL;
        }
        const bool whole = __all(valid && r == __shfl(r, 0));
        const bool up = valid && B.inside(i, r + 1), across = valid && i < I && B.inside(i + 1, r + 1);
        const double *Pr = P + (long long)r * PL;
        const double *Nu = B.nw(i, r + 1, 0), *Nd = across ? B.nw(i + 1, r + 1, 0) : nullptr;      // (Nu: an address alone, read only where `up`)
        const int sRow = s * K, xRow = across ? sRow + x[i] * C : 0;
        const bool nLive = up && n > -INFINITY, fLive = f > -INFINITY;
        const int bin0 = (r - r0) * PL;
        rowpost_add(tab, bin0, nLive ? exp(n + (Pr[0] + Nu[s])) : 0.0, whole, lane, det);
        for (int c = 1; c < PL; ++c) {      // the out-edges of (s, input token) that write the column's token are one CSR row
          double v = 0.0;
          if (valid && c == k) {
            if (nLive) v = exp(n + (Pr[c] + Nu[ks]));
          } else if (fLive) {
            const double pc = Pr[c];
            if (pc > -INFINITY) {
              const int tok = mm.colTok[c - 1];
              if (across) {
                const double *Ndc = Nd + (long long)c * S;
                const int a1 = m.outOff[xRow + tok + 1];
                for (int a = m.outOff[xRow + tok]; a < a1; ++a) v += exp(f + ((m.outW[a] + pc) + Ndc[m.outDst[a]]));
              }
              if (up) {
                const double *Nuc = Nu + (long long)c * S;
                const int a1 = m.outOff[sRow + tok + 1];
                for (int a = m.outOff[sRow + tok]; a < a1; ++a) v += exp(f + ((m.outW[a] + pc) + Nuc[m.outDst[a]]));
              }
            }
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

// Viterbi traceback over a materialised max lattice, one lane per pair: from the first plane that attains the score at
// W[I][L][.][S-1] back to N[0][0][0][0], taking at every cell the first candidate (in the fill's order) whose value equals the cell;
// an emitting edge comes from the lowest plane k != c whose W equals the edge's X.  Blank and repeat rows are not edges.  Edges go
// start -> end into the pair's slot (profile_pair_path_bound entries) with the row each fired at, as k_profile_pair_traceback.
// len = -1: no finite path, -2: the slot was too small, -3: no candidate matched (a corrupt matrix).  A candidate whose source cell
// lies outside the lattice is left out: it is -inf, and the cells on the path are finite, so a live cell always has a live source
// inside.
template <bool ENV>
__global__ void k_profile_pair_merge_traceback(DevMachine m, MergeMap mm, const typename PairMergeLattice<true, ENV>::Desc *__restrict__ descs,
                                               typename PairMergeLattice<true, ENV>::Tables t, int n,
                                               const int *__restrict__ inTok, const double *__restrict__ logP,
                                               const double *__restrict__ pool, uint32_t *edges, int32_t *rows, long long *len) {
  const int pair = blockIdx.x * blockDim.x + threadIdx.x;
  if (pair >= n) return;
  const auto pd = descs[pair];
  const int S = m.S, K = m.K, C = m.nOut + 1, nC = mm.nCols, PL = nC + 1, I = pd.nIn, L = pd.nRows;
  const int *x = inTok + pd.inBase;
  const double *P = logP + pd.rowBase * PL;
  const PairMergeLattice<true, ENV> lat(pd, t, const_cast<double *>(pool) + pd.cellBase, nullptr, S, PL);
  uint32_t *pe = edges + pd.pathBase;
  int32_t *pr = rows + pd.pathBase;
  int i = I, r = L, q = S - 1, layer = 1, p = 0;
  const long long cap = I + L + (long long)(I + L + 1) * (m.nLevF - 1);
  long long cnt = 0;
  {
    const double *We = lat.nw(I, L, 1) + q;
    double best = We[0];
    for (int k = 1; k < PL; ++k)
      if (best < We[k * S]) { best = We[k * S]; p = k; }
    if (!(best > -INFINITY)) { len[pair] = -1; return; }
  }
  for (;;) {
    const int xRow = i > 0 ? q * K + x[i - 1] * C : 0;
    int a = 0, found = -1, ni = i;
    if (layer == 1) {
      const double *W = lat.nw(i, r, 1) + p * S;
      const double cur = W[q];
      if (lat.nw(i, r, 0)[p * S + q] == cur) { layer = 0; continue; }
      if (i > 0 && lat.inside(i - 1, r)) {
        const double *Wl = lat.nw(i - 1, r, 1) + p * S;
        a = m.inOff[xRow];
        for (const int a1 = m.inOff[xRow + 1]; a < a1; ++a)
          if (Wl[m.inSrc[a]] + m.inW[a] == cur) { found = (int)m.inSrc[a]; ni = i - 1; break; }
      }
      if (found < 0) {
        a = m.inOff[q * K];
        for (const int a1 = m.inOff[q * K + 1]; a < a1; ++a) {
          const int s = (int)m.inSrc[a];
          if (s < q && W[s] + m.inW[a] == cur) { found = s; break; }
        }
      }
      if (found < 0) { len[pair] = -3; return; }
      if (cnt >= cap) { len[pair] = -2; return; }
      pe[cnt] = m.inEid[a]; pr[cnt] = r; ++cnt;
      i = ni; q = found;
    } else {
      if (r == 0) { if (i != 0 || q != 0 || p != 0) { len[pair] = -3; return; } break; }
      const bool up = lat.inside(i, r - 1);
      const double *Np = up ? lat.nw(i, r - 1, 0) : nullptr;
      const double cur = lat.nw(i, r, 0)[p * S + q], w = P[(long long)(r - 1) * PL + p];
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
      // the edge's X and the lowest plane that attains it
      auto excl = [&](const double *Wv, int s, int &kx) {
        double xs = Wv[s];
        kx = 0;
        for (int k = 1; k < PL; ++k)
          if (k != p && xs < Wv[k * S + s]) { xs = Wv[k * S + s]; kx = k; }
        return xs;
      };
      if (i > 0 && lat.inside(i - 1, r - 1)) {
        const double *Wd = lat.nw(i - 1, r - 1, 1);
        a = m.inOff[xRow + tok];
        for (const int a1 = m.inOff[xRow + tok + 1]; a < a1; ++a) {
          int kx;
          const double xs = excl(Wd, (int)m.inSrc[a], kx);
          if ((xs + m.inW[a]) + w == cur) { found = (int)m.inSrc[a]; from = kx; ni = i - 1; break; }
        }
      }
      if (found < 0 && up) {
        const double *Wu = lat.nw(i, r - 1, 1);
        a = m.inOff[q * K + tok];
        for (const int a1 = m.inOff[q * K + tok + 1]; a < a1; ++a) {
          int kx;
          const double xs = excl(Wu, (int)m.inSrc[a], kx);
          if ((xs + m.inW[a]) + w == cur) { found = (int)m.inSrc[a]; from = kx; break; }
        }
      }
      if (found < 0) { len[pair] = -3; return; }
      if (cnt >= cap) { len[pair] = -2; return; }
      --r;
      pe[cnt] = m.inEid[a]; pr[cnt] = r; ++cnt;
      i = ni; q = found; p = from; layer = 1;
    }
  }
  reverse_path(cnt, pe, pr);
  len[pair] = cnt;
}

// Posterior path samples over a materialised SUM lattice (docs/profile_tapes.md, "Posterior path samples of pairs against a merged
// profile"), one lane per (pair slot, sample) as k_profile_pair_sample (mb_profile_pair.hip): lane id serves slot id / nSamples,
// sample id % nSamples.  Decision 0 takes the end plane among W[I][L][.][S-1], planes ascending, against the likelihood folded as
// k_profile_pair_merge_fwd folds it.  Then back to N[0][0][0][0]: at a W cell "stay" (N), the input-only edges, the silent edges, all
// on the cell's plane; at N[.][r][0], r > 0, the blank out of every plane ascending; at N[.][r][c] the repeat, then the match edges
// and then the output-only edges of colTok[c] in `incoming` order, every edge once per source plane k != c ascending -- the lattice
// holds W, not the fill's X, so the (edge, plane) pairs are the candidates and their p sum to 1 up to the rounding of that
// regrouping; the last candidate with p > 0 takes what is left.  SampleDraw's kind carries the candidate's kind in its low two bits
// and the source plane above them.  rowCol[(rowBase - rowBase0) * nSamples + j * L + r]: the column row r took (0: the blank), -1 in
// every row of a dead pair.  The uniform of decision t of sample j of pair k (pairIdx[slot]) is philox_uniform(t, j, k, seed).
// Paths, len and logq are k_profile_pair_sample's; a candidate whose source cell lies outside the lattice is left out.
template <bool ENV>
__global__ __launch_bounds__(64) void k_profile_pair_merge_sample(DevMachine m, MergeMap mm, const typename PairMergeLattice<true, ENV>::Desc *__restrict__ descs,
                                                                  typename PairMergeLattice<true, ENV>::Tables t, long long nLanes, int nSamples,
                                                                  const long long *__restrict__ pairIdx, unsigned long long seed, const int *__restrict__ inTok,
                                                                  const double *__restrict__ logP, const double *__restrict__ pool, long long rowBase0,
                                                                  uint32_t *edges, int32_t *rows, int32_t *rowCol, long long *len, double *logq) {
  const long long id = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (id >= nLanes) return;
  const int slot = (int)(id / nSamples), j = (int)(id - (long long)slot * nSamples);
  const auto pd = descs[slot];
  const unsigned long long k = (unsigned long long)pairIdx[slot];
  const uint32_t k0 = (uint32_t)seed, k1 = (uint32_t)(seed >> 32), c2 = (uint32_t)k, c3 = (uint32_t)(k >> 32);
  const int S = m.S, K = m.K, C = m.nOut + 1, PL = mm.nCols + 1, I = pd.nIn, L = pd.nRows;
  const int *x = inTok + pd.inBase;
  const double *P = logP + pd.rowBase * PL;
  const PairMergeLattice<true, ENV> lat(pd, t, const_cast<double *>(pool) + pd.cellBase, nullptr, S, PL);
  const long long cap = I + L + (long long)(I + L + 1) * (m.nLevF - 1);
  uint32_t *pe = edges + pd.pathBase * nSamples + (long long)j * cap;
  int32_t *pr = rows + pd.pathBase * nSamples + (long long)j * cap;
  int32_t *rc = rowCol + (pd.rowBase - rowBase0) * nSamples + (long long)j * L;
  int i = I, r = L, q = S - 1, layer = 1, p = 0;
  long long cnt = 0;
  uint32_t dec = 0;
  double lq = 0.0;
  {
    const double *We = lat.nw(I, L, 1) + q;
    double LL = We[0];
    for (int pl = 1; pl < PL; ++pl) LL = lse2_exact(LL, We[pl * S]);
    if (!(LL > -INFINITY)) {
      for (int e = 0; e < L; ++e) rc[e] = -1;
      len[id] = -1; logq[id] = -INFINITY;
      return;
    }
    SampleDraw d(philox_uniform(dec++, (uint32_t)j, c2, c3, k0, k1), LL);
    for (int pl = 0; pl < PL && !d.done; ++pl) d.offer(We[pl * S], 0, 0, pl);
    if (d.kind < 0) { len[id] = -3; logq[id] = lq; return; }
    lq += d.term - d.cur;
    p = d.src;
  }
  for (;;) {
    const int xRow = i > 0 ? q * K + x[i - 1] * C : 0;
    if (layer == 1) {
      const double *W = lat.nw(i, r, 1) + p * S;
      SampleDraw d(philox_uniform(dec++, (uint32_t)j, c2, c3, k0, k1), W[q]);
      d.offer(lat.nw(i, r, 0)[p * S + q], 0, 0, q);
      if (i > 0 && lat.inside(i - 1, r)) {
        const double *Wl = lat.nw(i - 1, r, 1) + p * S;
        const int a1 = m.inOff[xRow + 1];
        for (int a = m.inOff[xRow]; a < a1 && !d.done; ++a) d.offer(Wl[m.inSrc[a]] + m.inW[a], 1, a, (int)m.inSrc[a]);
      }
      const int a1 = m.inOff[q * K + 1];
      for (int a = m.inOff[q * K]; a < a1 && !d.done; ++a) {
        const int s = (int)m.inSrc[a];
        if (s < q) d.offer(W[s] + m.inW[a], 2, a, s);
      }
      if (d.kind < 0) { len[id] = -3; logq[id] = lq; return; }
      lq += d.term - d.cur;
      if (d.kind == 0) { layer = 0; continue; }
      if (cnt >= cap) { len[id] = -2; logq[id] = lq; return; }
      pe[cnt] = m.inEid[d.a]; pr[cnt] = r; ++cnt;
      if (d.kind == 1) --i;
      q = d.src;
    } else {
      if (r == 0) { if (i != 0 || q != 0 || p != 0) { len[id] = -3; logq[id] = lq; return; } break; }
      const double *Pr = P + (long long)(r - 1) * PL;
      SampleDraw d(philox_uniform(dec++, (uint32_t)j, c2, c3, k0, k1), lat.nw(i, r, 0)[p * S + q]);
      const bool up = lat.inside(i, r - 1);
      const double *Np = lat.nw(i, r - 1, 0);      // (an address alone: read only where the cell is inside)
      if (p == 0) {
        if (up)
          for (int pl = 0; pl < PL && !d.done; ++pl) d.offer(Np[pl * S + q] + Pr[0], 0, 0, pl);
        if (d.kind < 0) { len[id] = -3; logq[id] = lq; return; }
        lq += d.term - d.cur;
        --r;
        rc[r] = 0;
        p = d.src;
        continue;
      }
      const double w = Pr[p];
      const int tok = mm.colTok[p - 1];
      if (up) d.offer(Np[p * S + q] + w, 0, 0, q);
      if (i > 0 && lat.inside(i - 1, r - 1)) {
        const double *Wd = lat.nw(i - 1, r - 1, 1);
        const int a1 = m.inOff[xRow + tok + 1];
        for (int a = m.inOff[xRow + tok]; a < a1 && !d.done; ++a) {
          const int s = (int)m.inSrc[a];
          for (int pl = 0; pl < PL && !d.done; ++pl)
            if (pl != p) d.offer((Wd[pl * S + s] + m.inW[a]) + w, 1 | (pl << 2), a, s);
        }
      }
      if (up) {
        const double *Wu = lat.nw(i, r - 1, 1);
        const int a1 = m.inOff[q * K + tok + 1];
        for (int a = m.inOff[q * K + tok]; a < a1 && !d.done; ++a) {
          const int s = (int)m.inSrc[a];
          for (int pl = 0; pl < PL && !d.done; ++pl)
            if (pl != p) d.offer((Wu[pl * S + s] + m.inW[a]) + w, 2 | (pl << 2), a, s);
        }
      }
      if (d.kind < 0) { len[id] = -3; logq[id] = lq; return; }
      lq += d.term - d.cur;
      --r;
      rc[r] = p;
      if (d.kind == 0) continue;      // the repeat: the walk stays in N on its plane
      if (cnt >= cap) { len[id] = -2; logq[id] = lq; return; }
      pe[cnt] = m.inEid[d.a]; pr[cnt] = r; ++cnt;
      if ((d.kind & 3) == 1) --i;
      q = d.src; p = d.kind >> 2; layer = 1;
    }
  }
  reverse_path(cnt, pe, pr);
  len[id] = cnt;
  logq[id] = lq;
}

// every kernel that may get a ring in dynamic LDS (allow_sweep_lds, mb_profile_common.h)
static bool ppm_allow_lds(size_t lds) {
  static size_t ldsAllowed = 64 * 1024;
  return allow_sweep_lds(ldsAllowed, lds,
                         {(const void *)&k_profile_pair_merge_fwd<MB_FORWARD, false, false>, (const void *)&k_profile_pair_merge_fwd<MB_VITERBI, false, false>,
                          (const void *)&k_profile_pair_merge_fwd<MB_FORWARD, true, false>, (const void *)&k_profile_pair_merge_fwd<MB_VITERBI, true, false>,
                          (const void *)&k_profile_pair_merge_bwd<false>,
                          (const void *)&k_profile_pair_merge_fwd<MB_FORWARD, false, true>, (const void *)&k_profile_pair_merge_fwd<MB_VITERBI, false, true>,
                          (const void *)&k_profile_pair_merge_fwd<MB_FORWARD, true, true>, (const void *)&k_profile_pair_merge_fwd<MB_VITERBI, true, true>,
                          (const void *)&k_profile_pair_merge_bwd<true>},
                         "k_profile_pair_merge: raising the LDS limit");
}

// The launchers: each sweep once over a form of the lattice, and the two overloads of the header that name one.
template <bool ENV>
static int ppm_fwd(const mb_machine *m, MergeMap mm, int mode, bool mat, const typename PairMergeLattice<true, ENV>::Desc *d, typename PairMergeLattice<true, ENV>::Tables t,
                   int n, size_t lds, long long maxItems, const int *inTok, const double *logP, double *pool, double *scratch, double *loglike, hipStream_t st) {
  if (n <= 0) return 0;
  if (!ppm_allow_lds(lds)) return 1;
  const dim3 g(n), b(sweep_threads(maxItems));
  if (mode == MB_VITERBI) {
    if (mat) k_profile_pair_merge_fwd<MB_VITERBI, true, ENV><<<g, b, lds, st>>>(m->dev, mm, d, t, inTok, logP, pool, scratch, loglike);
    else k_profile_pair_merge_fwd<MB_VITERBI, false, ENV><<<g, b, lds, st>>>(m->dev, mm, d, t, inTok, logP, pool, scratch, loglike);
  } else {
    if (mat) k_profile_pair_merge_fwd<MB_FORWARD, true, ENV><<<g, b, lds, st>>>(m->dev, mm, d, t, inTok, logP, pool, scratch, loglike);
    else k_profile_pair_merge_fwd<MB_FORWARD, false, ENV><<<g, b, lds, st>>>(m->dev, mm, d, t, inTok, logP, pool, scratch, loglike);
  }
  return hip_ok(hipGetLastError(), ENV ? "k_profile_pair_merge_env_fwd" : "k_profile_pair_merge_fwd") ? 0 : 1;
}
int launch_profile_pair_merge_fwd(const mb_machine *m, MergeMap mm, int mode, bool mat, const PairProfDesc *d, int n, size_t lds,
                                  long long maxItems, const int *inTok, const double *logP, double *pool, double *scratch,
                                  double *loglike, hipStream_t st) {
  return ppm_fwd<false>(m, mm, mode, mat, d, {}, n, lds, maxItems, inTok, logP, pool, scratch, loglike, st);
}
int launch_profile_pair_merge_fwd(const mb_machine *m, MergeMap mm, int mode, bool mat, const PairEnvDesc *d, const PairEnvTables &t, int n, size_t lds,
                                  long long maxItems, const int *inTok, const double *logP, double *pool, double *scratch,
                                  double *loglike, hipStream_t st) {
  return ppm_fwd<true>(m, mm, mode, mat, d, t, n, lds, maxItems, inTok, logP, pool, scratch, loglike, st);
}

template <bool ENV>
static int ppm_bwd(const mb_machine *m, MergeMap mm, const typename PairMergeLattice<true, ENV>::Desc *d, typename PairMergeLattice<true, ENV>::Tables t, int n, size_t lds,
                   long long maxItems, const int *inTok, const double *logP, double *pool, double *scratch, double *loglike, hipStream_t st) {
  if (n <= 0) return 0;
  if (!ppm_allow_lds(lds)) return 1;
  k_profile_pair_merge_bwd<ENV><<<dim3(n), dim3(sweep_threads(maxItems)), lds, st>>>(m->dev, mm, d, t, inTok, logP, pool, scratch, loglike);
  return hip_ok(hipGetLastError(), ENV ? "k_profile_pair_merge_env_bwd" : "k_profile_pair_merge_bwd") ? 0 : 1;
}
int launch_profile_pair_merge_bwd(const mb_machine *m, MergeMap mm, const PairProfDesc *d, int n, size_t lds, long long maxItems,
                                  const int *inTok, const double *logP, double *pool, double *scratch, double *loglike, hipStream_t st) {
  return ppm_bwd<false>(m, mm, d, {}, n, lds, maxItems, inTok, logP, pool, scratch, loglike, st);
}
int launch_profile_pair_merge_bwd(const mb_machine *m, MergeMap mm, const PairEnvDesc *d, const PairEnvTables &t, int n, size_t lds, long long maxItems,
                                  const int *inTok, const double *logP, double *pool, double *scratch, double *loglike, hipStream_t st) {
  return ppm_bwd<true>(m, mm, d, t, n, lds, maxItems, inTok, logP, pool, scratch, loglike, st);
}

template <bool ENV>
static int ppm_counts(const mb_machine *m, MergeMap mm, const typename PairMergeLattice<true, ENV>::Desc *d, typename PairMergeLattice<true, ENV>::Tables t, int n,
                      int groupsPerPair, const int *inTok, const double *logP, const double *fwdPool, const double *bwdPool, double *counts, hipStream_t st) {
  if (n <= 0 || m->nTrans <= 0) return 0;
  k_profile_pair_merge_counts<ENV><<<dim3((unsigned)((long long)n * groupsPerPair)), dim3(256), 0, st>>>(
      m->dev, mm, d, t, groupsPerPair, inTok, logP, fwdPool, bwdPool, m->nTrans, counts, g_deterministic ? 1 : 0);
  return hip_ok(hipGetLastError(), ENV ? "k_profile_pair_merge_env_counts" : "k_profile_pair_merge_counts") ? 0 : 1;
}
int launch_profile_pair_merge_counts(const mb_machine *m, MergeMap mm, const PairProfDesc *d, int n, int groupsPerPair, const int *inTok,
                                     const double *logP, const double *fwdPool, const double *bwdPool, double *counts, hipStream_t st) {
  return ppm_counts<false>(m, mm, d, {}, n, groupsPerPair, inTok, logP, fwdPool, bwdPool, counts, st);
}
int launch_profile_pair_merge_counts(const mb_machine *m, MergeMap mm, const PairEnvDesc *d, const PairEnvTables &t, int n, int groupsPerPair, const int *inTok,
                                     const double *logP, const double *fwdPool, const double *bwdPool, double *counts, hipStream_t st) {
  return ppm_counts<true>(m, mm, d, t, n, groupsPerPair, inTok, logP, fwdPool, bwdPool, counts, st);
}

template <bool ENV>
static int ppm_rowpost(const mb_machine *m, MergeMap mm, const typename PairMergeLattice<true, ENV>::Desc *d, typename PairMergeLattice<true, ENV>::Tables t, int n,
                       int groupsPerPair, int tabMax, const int *inTok, const double *logP, const double *fwdPool, const double *bwdPool,
                       const double *loglike, double *post, hipStream_t st) {
  if (n <= 0) return 0;
  k_profile_pair_merge_rowpost<ENV><<<dim3((unsigned)((long long)n * groupsPerPair)), dim3(ROWPOST_THREADS), 0, st>>>(
      m->dev, mm, d, t, groupsPerPair, inTok, logP, fwdPool, bwdPool, loglike, post, tabMax, g_deterministic ? 1 : 0);
  return hip_ok(hipGetLastError(), ENV ? "k_profile_pair_merge_env_rowpost" : "k_profile_pair_merge_rowpost") ? 0 : 1;
}
int launch_profile_pair_merge_rowpost(const mb_machine *m, MergeMap mm, const PairProfDesc *d, int n, int groupsPerPair, int tabMax,
                                      const int *inTok, const double *logP, const double *fwdPool, const double *bwdPool,
                                      const double *loglike, double *post, hipStream_t st) {
  return ppm_rowpost<false>(m, mm, d, {}, n, groupsPerPair, tabMax, inTok, logP, fwdPool, bwdPool, loglike, post, st);
}
int launch_profile_pair_merge_rowpost(const mb_machine *m, MergeMap mm, const PairEnvDesc *d, const PairEnvTables &t, int n, int groupsPerPair, int tabMax,
                                      const int *inTok, const double *logP, const double *fwdPool, const double *bwdPool,
                                      const double *loglike, double *post, hipStream_t st) {
  return ppm_rowpost<true>(m, mm, d, t, n, groupsPerPair, tabMax, inTok, logP, fwdPool, bwdPool, loglike, post, st);
}

template <bool ENV>
static int ppm_traceback(const mb_machine *m, MergeMap mm, const typename PairMergeLattice<true, ENV>::Desc *d, typename PairMergeLattice<true, ENV>::Tables t, int n,
                         const int *inTok, const double *logP, const double *pool, uint32_t *edges, int32_t *rows, long long *len, hipStream_t st) {
  if (n <= 0) return 0;
  k_profile_pair_merge_traceback<ENV><<<(n + 63) / 64, 64, 0, st>>>(m->dev, mm, d, t, n, inTok, logP, pool, edges, rows, len);
  return hip_ok(hipGetLastError(), ENV ? "k_profile_pair_merge_env_traceback" : "k_profile_pair_merge_traceback") ? 0 : 1;
}
int launch_profile_pair_merge_traceback(const mb_machine *m, MergeMap mm, const PairProfDesc *d, int n, const int *inTok,
                                        const double *logP, const double *pool, uint32_t *edges, int32_t *rows, long long *len,
                                        hipStream_t st) {
  return ppm_traceback<false>(m, mm, d, {}, n, inTok, logP, pool, edges, rows, len, st);
}
int launch_profile_pair_merge_traceback(const mb_machine *m, MergeMap mm, const PairEnvDesc *d, const PairEnvTables &t, int n, const int *inTok,
                                        const double *logP, const double *pool, uint32_t *edges, int32_t *rows, long long *len,
                                        hipStream_t st) {
  return ppm_traceback<true>(m, mm, d, t, n, inTok, logP, pool, edges, rows, len, st);
}

template <bool ENV>
static int ppm_sample(const mb_machine *m, MergeMap mm, const typename PairMergeLattice<true, ENV>::Desc *d, typename PairMergeLattice<true, ENV>::Tables t, int n,
                      int nSamples, const long long *pairIdx, unsigned long long seed, const int *inTok, const double *logP, const double *pool, long long rowBase0,
                      uint32_t *edges, int32_t *rows, int32_t *rowCol, long long *len, double *logq, hipStream_t st) {
  if (n <= 0) return 0;
  const long long nLanes = (long long)n * nSamples;      // (the caller keeps it within 2^31 - 1)
  k_profile_pair_merge_sample<ENV><<<(unsigned)((nLanes + 63) / 64), 64, 0, st>>>(m->dev, mm, d, t, nLanes, nSamples, pairIdx, seed, inTok, logP, pool, rowBase0, edges,
                                                                                rows, rowCol, len, logq);
  return hip_ok(hipGetLastError(), ENV ? "k_profile_pair_merge_env_sample" : "k_profile_pair_merge_sample") ? 0 : 1;
}
int launch_profile_pair_merge_sample(const mb_machine *m, MergeMap mm, const PairProfDesc *d, int n, int nSamples, const long long *pairIdx, unsigned long long seed,
                                     const int *inTok, const double *logP, const double *pool, long long rowBase0, uint32_t *edges, int32_t *rows, int32_t *rowCol,
                                     long long *len, double *logq, hipStream_t st) {
  return ppm_sample<false>(m, mm, d, {}, n, nSamples, pairIdx, seed, inTok, logP, pool, rowBase0, edges, rows, rowCol, len, logq, st);
}
int launch_profile_pair_merge_sample(const mb_machine *m, MergeMap mm, const PairEnvDesc *d, const PairEnvTables &t, int n, int nSamples, const long long *pairIdx,
                                     unsigned long long seed, const int *inTok, const double *logP, const double *pool, long long rowBase0, uint32_t *edges,
                                     int32_t *rows, int32_t *rowCol, long long *len, double *logq, hipStream_t st) {
  return ppm_sample<true>(m, mm, d, t, n, nSamples, pairIdx, seed, inTok, logP, pool, rowBase0, edges, rows, rowCol, len, logq, st);
}

}  // namespace mb
