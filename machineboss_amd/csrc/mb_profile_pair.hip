// mb_profile_pair.hip -- Forward / Backward / Viterbi / posterior counts of a machine WITH an input alphabet, run on a known input
// sequence x[1..I] against a PROFILE tape of L rows: the semantics of compose(M, transpose(CSVProfile::machine())) on input x with an
// empty output, restated in docs/profile_tapes.md ("Pairs: an input sequence against a profile"):
//
//   N[i][r][d] = [i = 0, r = 0, d = 0]
//                (+) N[i][r-1][d] + P[r-1][0]                                              (blank; r > 0)
//                (+) sum_{t: s->d, in = x_i, out = o}  W[i-1][r-1][s] + w_t + P[r-1][o]      (match;  i > 0, r > 0)
//                (+) sum_{t: s->d, in = eps, out = o}  W[i][r-1][s]   + w_t + P[r-1][o]      (output-only; r > 0)
//   W[i][r][d] = N[i][r][d]
//                (+) sum_{t: s->d, in = x_i, out = eps} W[i-1][r][s] + w_t                   (input-only; i > 0)
//                (+) sum_{silent t: s->d, s < d}        W[i][r][s]   + w_t                   (silent levels)
//   loglike    = W[I][L][S-1]
//
// One workgroup per pair, swept along the anti-diagonals i + r: the cells of a diagonal are independent (N reads the diagonals d-1
// and d-2, W reads d-1 and its own cell), so the work items of a diagonal are (cell, state) and the lanes stride over them.  Per
// diagonal: one phase for N and the non-silent part of W and one barrier, then one barrier per silent level -- (I + L + 1) nLevF
// barriers per pair.  The rolling sweeps keep a ring of three diagonals of both layers, 3 * 2 * (min(I, L) + 1) * S doubles, in LDS
// when that fits 160 KiB, else in the pair's slice of a global scratch buffer.  Cells are fp64, the sums the exact log-sum-exp.
//
// Every kernel is written once over a GEOMETRY, which says which cells exist and where they live: FullGeom, the whole rectangle, or
// EnvGeom, the cells of an envelope (docs/profile_tapes.md, "Pairs under an envelope").  The index rules of both are those of
// mb_profile_lattice.h; PairLattice below adds the two layers.  Both layers of a cell outside the envelope are -inf, so a neighbour
// outside is not read; the recurrence, the candidate order and the sums are the same text for both.
#include "mb_profile_common.h"
#include "mb_profile_pair_env.h"

namespace mb {

size_t profile_pair_lds_bytes(int S, long long nIn, long long nRows) {
  const double b = (double)profile_pair_ring(S, nIn, nRows) * sizeof(double);
  return b <= (double)SWEEP_LDS_MAX ? (size_t)b : 0;
}
size_t profile_pair_env_lds_bytes(int S, long long M) {
  const double b = (double)profile_pair_env_ring(S, M) * sizeof(double);
  return b <= (double)SWEEP_LDS_MAX ? (size_t)b : 0;
}

// A pair's lattice: the cells of mb_profile_lattice.h, RectCells or EnvCells, with two layers of S doubles in each.  MAT: the
// materialised lattice of mb_profile_pair.h (the compact one of mb_profile_pair_env.h) at base, else the ring.
template <class Cells, bool MAT>
struct PairLattice : Cells {
  using Desc = std::conditional_t<Cells::ENV, PairEnvDesc, PairProfDesc>;
  using Tables = std::conditional_t<Cells::ENV, PairEnvTables, NoTables>;
  double *base;
  int S;
  __device__ __forceinline__ PairLattice(const Desc &pd, const Tables &t, double *base, int S) : Cells(lattice_cells(pd, t)), base(base), S(S) {}
  __device__ __forceinline__ double *at(int i, int r, int layer) const { return base + ((MAT ? this->index(i, r) : this->slot(i, r)) * 2 + layer) * S; }
};
template <bool MAT> using FullGeom = PairLattice<RectCells, MAT>;
template <bool MAT> using EnvGeom = PairLattice<EnvCells, MAT>;

// Forward (MODE = MB_FORWARD) or Viterbi (MB_VITERBI) sweep.  MAT: every cell into pool (the geometry's layout), else rolling.
// Viterbi keeps the FIRST maximum: N takes the blank first, then the match edges in `incoming` order, then the output-only edges in
// `incoming` order; W takes N (no move) first, then the input-only edges, then the silent edges, each in `incoming` order -- the
// order k_profile_pair_traceback re-enumerates.
template <int MODE, bool MAT, template <bool> class Geom>
__global__ __launch_bounds__(SWEEP_THREADS) void k_profile_pair_fwd(DevMachine m, const typename Geom<MAT>::Desc *__restrict__ descs, typename Geom<MAT>::Tables t,
                                                                    const int *__restrict__ inTok, const double *__restrict__ logP,
                                                                    double *pool, double *scratch, double *__restrict__ loglike) {
  extern __shared__ double pp_sh[];
  const auto pd = descs[blockIdx.x];
  const int S = m.S, K = m.K, C = m.nOut + 1, I = pd.nIn, L = pd.nRows;
  const int *x = inTok + pd.inBase;
  const double *P = logP + pd.rowBase * C;
  const Geom<MAT> lat(pd, t, MAT ? pool + pd.cellBase : (pd.ringBase < 0 ? pp_sh : scratch + pd.ringBase), S);
  for (int d = 0; d <= I + L; ++d) {
    int ilo, nCells;
    lat.diag(d, ilo, nCells);
    const int nItems = nCells * S;
    for (int it = threadIdx.x; it < nItems; it += blockDim.x) {
      const int c = it / S, q = it - c * S, i = ilo + c, r = d - i;
      const int xRow = i > 0 ? q * K + x[i - 1] * C : 0;     // CSR rows q*K + key(x_i, o), o = 0..nOut: contiguous
      double acc;
      if (r > 0) {
        const double *Pr = P + (long long)(r - 1) * C;
        const bool up = lat.inside(i, r - 1);
        acc = up ? lat.at(i, r - 1, 0)[q] + Pr[0] : -INFINITY;
        if (i > 0 && lat.inside(i - 1, r - 1)) {
          const double *Wd = lat.at(i - 1, r - 1, 1);
          const int a1 = m.inOff[xRow + C];
          for (int a = m.inOff[xRow + 1]; a < a1; ++a)
            acc = red<MODE>(acc, (Wd[m.inSrc[a]] + m.inW[a]) + Pr[m.eOutTok[m.inEid[a]]]);
        }
        if (up) {
          const double *Wu = lat.at(i, r - 1, 1);
          const int a1 = m.inOff[q * K + C];
          for (int a = m.inOff[q * K + 1]; a < a1; ++a)
            acc = red<MODE>(acc, (Wu[m.inSrc[a]] + m.inW[a]) + Pr[m.eOutTok[m.inEid[a]]]);
        }
      } else {
        acc = (i == 0 && q == 0) ? 0.0 : -INFINITY;
      }
      lat.at(i, r, 0)[q] = acc;
      if (i > 0 && lat.inside(i - 1, r)) {
        const double *Wl = lat.at(i - 1, r, 1);
        const int a1 = m.inOff[xRow + 1];
        for (int a = m.inOff[xRow]; a < a1; ++a) acc = red<MODE>(acc, Wl[m.inSrc[a]] + m.inW[a]);
      }
      lat.at(i, r, 1)[q] = acc;
    }
    __syncthreads();
    for (int lev = 1; lev < m.nLevF; ++lev) {      // (level 0 has no silent edge coming in: its W is complete)
      const int l0 = m.levFOff[lev], ns = m.levFOff[lev + 1] - l0;
      const int nLevItems = nCells * ns;
      for (int it = threadIdx.x; it < nLevItems; it += blockDim.x) {
        const int c = it / ns, q = m.levFState[l0 + (it - c * ns)], i = ilo + c;
        double *Wc = lat.at(i, d - i, 1);
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
  }
  if (threadIdx.x == 0) loglike[blockIdx.x] = lat.at(I, L, 1)[S - 1];      // (an envelope is connected: (0, 0) and (I, L) are inside)
}

// Materialised Backward sweep, layer 0 = NB ("from the arrived stage"), layer 1 = WB ("from the waiting stage"):
//   WB[i][r][s] = [i = I, r = L, s = S-1]
//                 (+) sum_{t: s->d, in = x_{i+1}, out = o} (w_t + P[r][o]) + NB[i+1][r+1][d]     (i < I, r < L)
//                 (+) sum_{t: s->d, in = eps, out = o}     (w_t + P[r][o]) + NB[i][r+1][d]       (r < L)
//                 (+) sum_{t: s->d, in = x_{i+1}, out = eps} w_t + WB[i+1][r][d]                 (i < I)
//                 (+) sum_{silent t: s->d, s < d}            w_t + WB[i][r][d]
//   NB[i][r][s] = WB[i][r][s] (+) (P[r][0] + NB[i][r+1][s])   (r < L);   loglike = NB[0][0][0]
// Anti-diagonals from I + L down.  A state's WB is final once its backward level has run; the item that finishes it writes its NB.
// A successor cell outside the geometry contributes nothing.
template <template <bool> class Geom>
__global__ __launch_bounds__(SWEEP_THREADS) void k_profile_pair_bwd(DevMachine m, const typename Geom<true>::Desc *__restrict__ descs, typename Geom<true>::Tables t,
                                                                    const int *__restrict__ inTok, const double *__restrict__ logP,
                                                                    double *pool, double *__restrict__ loglike) {
  const auto pd = descs[blockIdx.x];
  const int S = m.S, K = m.K, C = m.nOut + 1, I = pd.nIn, L = pd.nRows;
  const int *x = inTok + pd.inBase;
  const double *P = logP + pd.rowBase * C;
  const Geom<true> lat(pd, t, pool + pd.cellBase, S);
  for (int d = I + L; d >= 0; --d) {
    int ilo, nCells;
    lat.diag(d, ilo, nCells);
    const int nItems = nCells * S;
    for (int it = threadIdx.x; it < nItems; it += blockDim.x) {
      const int c = it / S, s = it - c * S, i = ilo + c, r = d - i;
      const int xRow = i < I ? s * K + x[i] * C : 0;
      const double *Pr = P + (long long)r * C;
      const bool down = r < L && lat.inside(i, r + 1);
      double v = (i == I && r == L && s == S - 1) ? 0.0 : -INFINITY;
      if (r < L) {
        if (i < I && lat.inside(i + 1, r + 1)) {
          const double *Nd = lat.at(i + 1, r + 1, 0);
          const int a1 = m.outOff[xRow + C];
          for (int a = m.outOff[xRow + 1]; a < a1; ++a)
            v = lse2_exact(v, (m.outW[a] + Pr[m.eOutTok[m.outEid[a]]]) + Nd[m.outDst[a]]);
        }
        if (down) {
          const double *Nu = lat.at(i, r + 1, 0);
          const int a1 = m.outOff[s * K + C];
          for (int a = m.outOff[s * K + 1]; a < a1; ++a)
            v = lse2_exact(v, (m.outW[a] + Pr[m.eOutTok[m.outEid[a]]]) + Nu[m.outDst[a]]);
        }
      }
      if (i < I && lat.inside(i + 1, r)) {
        const double *Wl = lat.at(i + 1, r, 1);
        const int a1 = m.outOff[xRow + 1];
        for (int a = m.outOff[xRow]; a < a1; ++a) v = lse2_exact(v, Wl[m.outDst[a]] + m.outW[a]);
      }
      lat.at(i, r, 1)[s] = v;
      lat.at(i, r, 0)[s] = down ? lse2_exact(v, Pr[0] + lat.at(i, r + 1, 0)[s]) : v;
    }
    __syncthreads();
    for (int lev = 1; lev < m.nLevB; ++lev) {
      const int l0 = m.levBOff[lev], ns = m.levBOff[lev + 1] - l0;
      const int nLevItems = nCells * ns;
      for (int it = threadIdx.x; it < nLevItems; it += blockDim.x) {
        const int c = it / ns, s = m.levBState[l0 + (it - c * ns)], i = ilo + c, r = d - i;
        double *Wc = lat.at(i, r, 1);
        double v = Wc[s];
        const int a1 = m.outOff[s * K + 1];
        for (int a = m.outOff[s * K]; a < a1; ++a) {
          const int t = (int)m.outDst[a];
          if (t <= s) continue;
          v = lse2_exact(v, Wc[t] + m.outW[a]);
        }
        Wc[s] = v;
        lat.at(i, r, 0)[s] = (r < L && lat.inside(i, r + 1)) ? lse2_exact(v, P[(long long)r * C] + lat.at(i, r + 1, 0)[s]) : v;
      }
      __syncthreads();
    }
  }
  if (threadIdx.x == 0) loglike[blockIdx.x] = lat.at(0, 0, 0)[0];
}

// Posterior counts.  With both lattices in memory every (cell, edge) term is independent:
//   count[t] += exp(W_F[i][r][s] - LL + term_t), term_t the edge's summand of WB[i][r][s] above,
// so the sweep is a flat grid over (pair, group of the pair, (cell, state)), accumulated by CountsAcc (mb_profile_common.h).  A pair
// whose likelihood is -inf adds nothing.
template <template <bool> class Geom>
__global__ __launch_bounds__(256) void k_profile_pair_counts(DevMachine m, const typename Geom<true>::Desc *__restrict__ descs, typename Geom<true>::Tables t, int groupsPerPair,
                                                             const int *__restrict__ inTok, const double *__restrict__ logP,
                                                             const double *__restrict__ fwdPool, const double *__restrict__ bwdPool,
                                                             long long nTrans, double *__restrict__ counts, int det) {
  __shared__ double lcount[COUNTS_LDS_MAX];
  const CountsAcc acc(lcount, counts, nTrans, det);
  const int k = blockIdx.x / groupsPerPair, group = blockIdx.x % groupsPerPair;
  const auto pd = descs[k];
  const int S = m.S, K = m.K, C = m.nOut + 1, I = pd.nIn, L = pd.nRows;
  const int *x = inTok + pd.inBase;
  const double *P = logP + pd.rowBase * C;
  const Geom<true> F(pd, t, const_cast<double *>(fwdPool) + pd.cellBase, S), B(pd, t, const_cast<double *>(bwdPool) + pd.cellBase, S);
  const double LL = F.at(I, L, 1)[S - 1];
  if (LL > -INFINITY) {
    const long long nItems = F.cells() * S;
    for (long long idx = (long long)group * blockDim.x + threadIdx.x; idx < nItems; idx += (long long)groupsPerPair * blockDim.x) {
      const long long cell = idx / S;
      const int s = (int)(idx - cell * S);
      int i, r;
      F.cell(cell, i, r);
      const double f = F.at(i, r, 1)[s] - LL;
      if (!(f > -INFINITY)) continue;
      const int xRow = i < I ? s * K + x[i] * C : 0;
      const double *Pr = P + (long long)r * C;
      if (r < L) {
        if (i < I && B.inside(i + 1, r + 1)) {
          const double *Nd = B.at(i + 1, r + 1, 0);
          const int a1 = m.outOff[xRow + C];
          for (int a = m.outOff[xRow + 1]; a < a1; ++a)
            acc.add(m.outEid[a], exp(f + ((m.outW[a] + Pr[m.eOutTok[m.outEid[a]]]) + Nd[m.outDst[a]])));
        }
        if (B.inside(i, r + 1)) {
          const double *Nu = B.at(i, r + 1, 0);
          const int a1 = m.outOff[s * K + C];
          for (int a = m.outOff[s * K + 1]; a < a1; ++a)
            acc.add(m.outEid[a], exp(f + ((m.outW[a] + Pr[m.eOutTok[m.outEid[a]]]) + Nu[m.outDst[a]])));
        }
      }
      if (i < I && B.inside(i + 1, r)) {
        const double *Wl = B.at(i + 1, r, 1);
        const int a1 = m.outOff[xRow + 1];
        for (int a = m.outOff[xRow]; a < a1; ++a) acc.add(m.outEid[a], exp(f + (Wl[m.outDst[a]] + m.outW[a])));
      }
      const double *Wc = B.at(i, r, 1);
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

// Row posteriors: post[(rowBase + r) * C + o] = the posterior probability that row r of the pair's profile was consumed as column o
// (0: the blank), the gradient of the log-likelihood in P[r][o] (docs/profile_tapes.md, "Row posteriors"):
//   post[r][0] = sum_i sum_s exp((N_F[i][r][s] - LL) + (P[r][0] + NB[i][r+1][s]))
//   post[r][o] = the emitting terms of k_profile_pair_counts above, binned by (row, output token) instead of by transition.
// The bins are few and the lanes of a wavefront are consecutive states of a cell, so nothing is added per term.  The work items are
// (row, cell of the row, state) in that order and a workgroup owns whole rows: blocks of profile_pair_rowpost_rows rows, dealt round
// robin to the pair's groups.  A lane sums its terms of one column in a register, in CSR order; where all 64 lanes of the wavefront
// hold items of one row the lane sums are reduced across the lanes and one lane adds the result to the workgroup's LDS table (rows
// of the block x C), else (a row seam, the tail of the block) every lane adds its own.  The table is then stored: every bin has one
// writing workgroup, so there is no global atomic and nothing to clear beforehand.  A row of more than tabMax columns is summed in
// its global bins instead, cleared by the workgroup that owns it.  A pair whose likelihood is -inf gets zeros.
// det: a lane sum is turned into 64-bit fixed point at 2^-36 (mb_internal.h) before it meets another, and integers are reduced and
// added (rowpost_add, mb_profile_common.h); post then holds the integers.
template <template <bool> class Geom>
__global__ __launch_bounds__(ROWPOST_THREADS) void k_profile_pair_rowpost(DevMachine m, const typename Geom<true>::Desc *__restrict__ descs, typename Geom<true>::Tables t, int groupsPerPair,
                                                                          const int *__restrict__ inTok, const double *__restrict__ logP,
                                                                          const double *__restrict__ fwdPool, const double *__restrict__ bwdPool,
                                                                          double *post, int tabMax, int det) {
  __shared__ double ltab[ROWPOST_LDS_MAX];
  const int k = blockIdx.x / groupsPerPair, group = blockIdx.x % groupsPerPair;
  const auto pd = descs[k];
  const int S = m.S, K = m.K, C = m.nOut + 1, I = pd.nIn, L = pd.nRows;
  if (L == 0) return;
  const int *x = inTok + pd.inBase;
  const double *P = logP + pd.rowBase * C;
  const Geom<true> F(pd, t, const_cast<double *>(fwdPool) + pd.cellBase, S), B(pd, t, const_cast<double *>(bwdPool) + pd.cellBase, S);
  const double LL = F.at(I, L, 1)[S - 1];
  const int R = profile_pair_rowpost_rows(F.cells(), S, L, C, tabMax);
  const bool useLds = C <= tabMax;
  const int lane = threadIdx.x & 63;
  for (long long rb = (long long)group * R; rb < L; rb += (long long)groupsPerPair * R) {
    const int r0 = (int)rb, r1 = (int)min((long long)L, rb + R), nBins = (r1 - r0) * C;
    double *out = post + (pd.rowBase + r0) * C;
    double *tab = useLds ? ltab : out;
    for (int e = threadIdx.x; e < nBins; e += blockDim.x) tab[e] = 0.0;      // (the fixed point's zero has the same bits)
    if (!useLds) __threadfence();
    __syncthreads();
    if (LL > -INFINITY) {
      const long long c0 = F.template lineFirst<0>(r0), nItems = (F.template lineFirst<0>(r1) - c0) * S;
      for (long long base = threadIdx.x - lane; base < nItems; base += blockDim.x) {      // (a wavefront stays whole in here)
        const long long idx = base + lane;
        const bool valid = idx < nItems;
        int i = 0, r = r0, s = 0;
        double f = -INFINITY, n = -INFINITY;
        if (valid) {
          const long long cell = idx / S;
          s = (int)(idx - cell * S);
          F.template lineCell<0>(c0 + cell, i, r);
          f = F.at(i, r, 1)[s] - LL;
          n = F.at(i, r, 0)[s] - LL;
        }
        const bool whole = __all(valid && r == __shfl(r, 0));
        const bool up = valid && B.inside(i, r + 1), across = valid && i < I && B.inside(i + 1, r + 1);
        const double *Pr = P + (long long)r * C;
        const double *Nu = up ? B.at(i, r + 1, 0) : nullptr, *Nd = across ? B.at(i + 1, r + 1, 0) : nullptr;
        const int sRow = s * K, xRow = across ? sRow + x[i] * C : 0;
        const bool fLive = f > -INFINITY;
        const int bin0 = (r - r0) * C;
        rowpost_add(tab, bin0, (up && n > -INFINITY) ? exp(n + (Pr[0] + Nu[s])) : 0.0, whole, lane, det);
        for (int o = 1; o < C; ++o) {      // the out-edges of (s, input token) that write o are one CSR row
          double v = 0.0;
          if (fLive) {
            const double po = Pr[o];
            if (across) {
              const int a1 = m.outOff[xRow + o + 1];
              for (int a = m.outOff[xRow + o]; a < a1; ++a) v += exp(f + ((m.outW[a] + po) + Nd[m.outDst[a]]));
            }
            if (up) {
              const int a1 = m.outOff[sRow + o + 1];
              for (int a = m.outOff[sRow + o]; a < a1; ++a) v += exp(f + ((m.outW[a] + po) + Nu[m.outDst[a]]));
            }
          }
          rowpost_add(tab, bin0 + o, v, whole, lane, det);
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

// Viterbi traceback over a materialised max lattice, one lane per pair: from W[I][L][S-1] back to N[0][0][0], taking at every cell
// the first candidate (in the fill's order) whose value equals the cell.  Edges go start -> end into the pair's slot
// (profile_pair_path_bound entries) with the row each fired at: an emitting edge the row it consumed, an output-less edge the number
// of rows consumed before it.  len = -1: no finite path, -2: the slot was too small, -3: no candidate matched (a corrupt matrix).
// A candidate whose source cell lies outside the geometry is left out: it is -inf, and the cells on the path are finite.
template <template <bool> class Geom>
__global__ void k_profile_pair_traceback(DevMachine m, const typename Geom<true>::Desc *__restrict__ descs, typename Geom<true>::Tables t, int n, const int *__restrict__ inTok,
                                         const double *__restrict__ logP, const double *__restrict__ pool, uint32_t *edges,
                                         int32_t *rows, long long *len) {
  const int k = blockIdx.x * blockDim.x + threadIdx.x;
  if (k >= n) return;
  const auto pd = descs[k];
  const int S = m.S, K = m.K, C = m.nOut + 1, I = pd.nIn, L = pd.nRows;
  const int *x = inTok + pd.inBase;
  const double *P = logP + pd.rowBase * C;
  const Geom<true> lat(pd, t, const_cast<double *>(pool) + pd.cellBase, S);
  uint32_t *pe = edges + pd.pathBase;
  int32_t *pr = rows + pd.pathBase;
  int i = I, r = L, q = S - 1, layer = 1;
  const long long cap = I + L + (long long)(I + L + 1) * (m.nLevF - 1);
  long long cnt = 0;
  if (!(lat.at(i, r, 1)[q] > -INFINITY)) { len[k] = -1; return; }
  for (;;) {
    const int xRow = i > 0 ? q * K + x[i - 1] * C : 0;
    int a = 0, found = -1;
    if (layer == 1) {
      const double *W = lat.at(i, r, 1);
      const double cur = W[q];
      if (lat.at(i, r, 0)[q] == cur) { layer = 0; continue; }
      int ni = i;
      if (i > 0 && lat.inside(i - 1, r)) {
        const double *Wl = lat.at(i - 1, r, 1);
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
      if (found < 0) { len[k] = -3; return; }
      if (cnt >= cap) { len[k] = -2; return; }
      pe[cnt] = m.inEid[a]; pr[cnt] = r; ++cnt;
      i = ni; q = found;
    } else {
      if (r == 0) { if (i != 0 || q != 0) { len[k] = -3; return; } break; }
      const double *Pr = P + (long long)(r - 1) * C;
      const double cur = lat.at(i, r, 0)[q];
      const bool up = lat.inside(i, r - 1);
      if (up && lat.at(i, r - 1, 0)[q] + Pr[0] == cur) { --r; continue; }
      int ni = i;
      if (i > 0 && lat.inside(i - 1, r - 1)) {
        const double *Wd = lat.at(i - 1, r - 1, 1);
        a = m.inOff[xRow + 1];
        for (const int a1 = m.inOff[xRow + C]; a < a1; ++a)
          if ((Wd[m.inSrc[a]] + m.inW[a]) + Pr[m.eOutTok[m.inEid[a]]] == cur) { found = (int)m.inSrc[a]; ni = i - 1; break; }
      }
      if (found < 0 && up) {
        const double *Wu = lat.at(i, r - 1, 1);
        a = m.inOff[q * K + 1];
        for (const int a1 = m.inOff[q * K + C]; a < a1; ++a)
          if ((Wu[m.inSrc[a]] + m.inW[a]) + Pr[m.eOutTok[m.inEid[a]]] == cur) { found = (int)m.inSrc[a]; break; }
      }
      if (found < 0) { len[k] = -3; return; }
      if (cnt >= cap) { len[k] = -2; return; }
      --r;
      pe[cnt] = m.inEid[a]; pr[cnt] = r; ++cnt;
      i = ni; q = found; layer = 1;
    }
  }
  reverse_path(cnt, pe, pr);
  len[k] = cnt;
}

// Posterior path samples over a materialised SUM lattice (docs/profile_tapes.md, "Posterior path samples"), one lane per (pair slot,
// sample): lane id serves slot id / nSamples, sample id % nSamples, so the lanes of a wavefront walk the same lattice.  From
// W[I][L][S-1] back to N[0][0][0]; at every W cell and every N cell with r > 0 one decision among the terms of the fill, in the
// fill's order and parenthesisation -- the list k_profile_pair_traceback enumerates -- each with probability exp(term - cell).  The
// uniform of decision t of sample j of pair k (pairIdx[slot]: the pair's index in the object, not in the chunk) is
// philox_uniform(t, j, k, seed), so a sample depends on nothing else.  logq: the sum of term - cell over the decisions, the log
// posterior probability of the path.  Edges go into the sample's slot, at (pathBase * nSamples + j * bound) with bound the pair's
// profile_pair_path_bound, backwards and are reversed at the end.  len = -1: a dead pair (logq = -inf), -2: the slot was too small,
// -3: no candidate with p > 0 (a corrupt lattice).  A candidate whose source cell lies outside the geometry is left out.
template <template <bool> class Geom>
__global__ __launch_bounds__(64) void k_profile_pair_sample(DevMachine m, const typename Geom<true>::Desc *__restrict__ descs, typename Geom<true>::Tables t, long long nLanes,
                                                            int nSamples, const long long *__restrict__ pairIdx, unsigned long long seed,
                                                            const int *__restrict__ inTok, const double *__restrict__ logP, const double *__restrict__ pool,
                                                            uint32_t *edges, int32_t *rows, long long *len, double *logq) {
  const long long id = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (id >= nLanes) return;
  const int slot = (int)(id / nSamples), j = (int)(id - (long long)slot * nSamples);
  const auto pd = descs[slot];
  const unsigned long long k = (unsigned long long)pairIdx[slot];
  const uint32_t k0 = (uint32_t)seed, k1 = (uint32_t)(seed >> 32), c2 = (uint32_t)k, c3 = (uint32_t)(k >> 32);
  const int S = m.S, K = m.K, C = m.nOut + 1, I = pd.nIn, L = pd.nRows;
  const int *x = inTok + pd.inBase;
  const double *P = logP + pd.rowBase * C;
  const Geom<true> lat(pd, t, const_cast<double *>(pool) + pd.cellBase, S);
  const long long cap = I + L + (long long)(I + L + 1) * (m.nLevF - 1);
  uint32_t *pe = edges + pd.pathBase * nSamples + (long long)j * cap;
  int32_t *pr = rows + pd.pathBase * nSamples + (long long)j * cap;
  int i = I, r = L, q = S - 1, layer = 1;
  long long cnt = 0;
  uint32_t dec = 0;
  double lq = 0.0;
  if (!(lat.at(i, r, 1)[q] > -INFINITY)) { len[id] = -1; logq[id] = -INFINITY; return; }
  for (;;) {
    const int xRow = i > 0 ? q * K + x[i - 1] * C : 0;
    if (layer == 1) {
      const double *W = lat.at(i, r, 1);
      SampleDraw d(philox_uniform(dec++, (uint32_t)j, c2, c3, k0, k1), W[q]);
      d.offer(lat.at(i, r, 0)[q], 0, 0, q);
      if (i > 0 && lat.inside(i - 1, r)) {
        const double *Wl = lat.at(i - 1, r, 1);
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
      if (r == 0) { if (i != 0 || q != 0) { len[id] = -3; logq[id] = lq; return; } break; }
      const double *Pr = P + (long long)(r - 1) * C;
      SampleDraw d(philox_uniform(dec++, (uint32_t)j, c2, c3, k0, k1), lat.at(i, r, 0)[q]);
      const bool up = lat.inside(i, r - 1);
      if (up) d.offer(lat.at(i, r - 1, 0)[q] + Pr[0], 0, 0, q);
      if (i > 0 && lat.inside(i - 1, r - 1)) {
        const double *Wd = lat.at(i - 1, r - 1, 1);
        const int a1 = m.inOff[xRow + C];
        for (int a = m.inOff[xRow + 1]; a < a1 && !d.done; ++a)
          d.offer((Wd[m.inSrc[a]] + m.inW[a]) + Pr[m.eOutTok[m.inEid[a]]], 1, a, (int)m.inSrc[a]);
      }
      if (up) {
        const double *Wu = lat.at(i, r - 1, 1);
        const int a1 = m.inOff[q * K + C];
        for (int a = m.inOff[q * K + 1]; a < a1 && !d.done; ++a)
          d.offer((Wu[m.inSrc[a]] + m.inW[a]) + Pr[m.eOutTok[m.inEid[a]]], 2, a, (int)m.inSrc[a]);
      }
      if (d.kind < 0) { len[id] = -3; logq[id] = lq; return; }
      lq += d.term - d.cur;
      --r;
      if (d.kind == 0) continue;
      if (cnt >= cap) { len[id] = -2; logq[id] = lq; return; }
      pe[cnt] = m.inEid[d.a]; pr[cnt] = r; ++cnt;
      if (d.kind == 1) --i;
      q = d.src; layer = 1;
    }
  }
  reverse_path(cnt, pe, pr);
  len[id] = cnt;
  logq[id] = lq;
}

// The launchers: each sweep once over a geometry, and the two overloads of the headers that name one.
template <template <bool> class Geom>
static int pair_fwd(const mb_machine *m, int mode, bool mat, const typename Geom<true>::Desc *d, typename Geom<true>::Tables t, int n, size_t lds, long long maxItems,
                    const int *inTok, const double *logP, double *pool, double *scratch, double *loglike, hipStream_t st) {
  constexpr bool ENV = Geom<true>::ENV;
  if (n <= 0) return 0;
  if (mat) lds = 0;
  static size_t ldsAllowed = 64 * 1024;
  if (!allow_sweep_lds(ldsAllowed, lds, {(const void *)&k_profile_pair_fwd<MB_FORWARD, false, Geom>, (const void *)&k_profile_pair_fwd<MB_VITERBI, false, Geom>},
                       ENV ? "k_profile_pair_env_fwd: raising the LDS limit" : "k_profile_pair_fwd: raising the LDS limit")) return 1;
  const dim3 g(n), b(sweep_threads(maxItems));
  if (mode == MB_VITERBI) {
    if (mat) k_profile_pair_fwd<MB_VITERBI, true, Geom><<<g, b, 0, st>>>(m->dev, d, t, inTok, logP, pool, scratch, loglike);
    else k_profile_pair_fwd<MB_VITERBI, false, Geom><<<g, b, lds, st>>>(m->dev, d, t, inTok, logP, pool, scratch, loglike);
  } else {
    if (mat) k_profile_pair_fwd<MB_FORWARD, true, Geom><<<g, b, 0, st>>>(m->dev, d, t, inTok, logP, pool, scratch, loglike);
    else k_profile_pair_fwd<MB_FORWARD, false, Geom><<<g, b, lds, st>>>(m->dev, d, t, inTok, logP, pool, scratch, loglike);
  }
  return hip_ok(hipGetLastError(), ENV ? "k_profile_pair_env_fwd" : "k_profile_pair_fwd") ? 0 : 1;
}
int launch_profile_pair_fwd(const mb_machine *m, int mode, bool mat, const PairProfDesc *d, int n, size_t lds, long long maxItems, const int *inTok,
                            const double *logP, double *pool, double *scratch, double *loglike, hipStream_t st) {
  return pair_fwd<FullGeom>(m, mode, mat, d, {}, n, lds, maxItems, inTok, logP, pool, scratch, loglike, st);
}
int launch_profile_pair_fwd(const mb_machine *m, int mode, bool mat, const PairEnvDesc *d, const PairEnvTables &t, int n, size_t lds, long long maxItems,
                            const int *inTok, const double *logP, double *pool, double *scratch, double *loglike, hipStream_t st) {
  return pair_fwd<EnvGeom>(m, mode, mat, d, t, n, lds, maxItems, inTok, logP, pool, scratch, loglike, st);
}

template <template <bool> class Geom>
static int pair_bwd(const mb_machine *m, const typename Geom<true>::Desc *d, typename Geom<true>::Tables t, int n, long long maxItems, const int *inTok,
                    const double *logP, double *pool, double *loglike, hipStream_t st) {
  if (n <= 0) return 0;
  k_profile_pair_bwd<Geom><<<dim3(n), dim3(sweep_threads(maxItems)), 0, st>>>(m->dev, d, t, inTok, logP, pool, loglike);
  return hip_ok(hipGetLastError(), Geom<true>::ENV ? "k_profile_pair_env_bwd" : "k_profile_pair_bwd") ? 0 : 1;
}
int launch_profile_pair_bwd(const mb_machine *m, const PairProfDesc *d, int n, long long maxItems, const int *inTok, const double *logP, double *pool,
                            double *loglike, hipStream_t st) {
  return pair_bwd<FullGeom>(m, d, {}, n, maxItems, inTok, logP, pool, loglike, st);
}
int launch_profile_pair_bwd(const mb_machine *m, const PairEnvDesc *d, const PairEnvTables &t, int n, long long maxItems, const int *inTok, const double *logP,
                            double *pool, double *loglike, hipStream_t st) {
  return pair_bwd<EnvGeom>(m, d, t, n, maxItems, inTok, logP, pool, loglike, st);
}

template <template <bool> class Geom>
static int pair_counts(const mb_machine *m, const typename Geom<true>::Desc *d, typename Geom<true>::Tables t, int n, int groupsPerPair, const int *inTok,
                       const double *logP, const double *fwdPool, const double *bwdPool, double *counts, hipStream_t st) {
  if (n <= 0 || m->nTrans <= 0) return 0;
  k_profile_pair_counts<Geom><<<dim3((unsigned)((long long)n * groupsPerPair)), dim3(256), 0, st>>>(m->dev, d, t, groupsPerPair, inTok, logP, fwdPool, bwdPool, m->nTrans, counts,
                                                                                                 g_deterministic ? 1 : 0);
  return hip_ok(hipGetLastError(), Geom<true>::ENV ? "k_profile_pair_env_counts" : "k_profile_pair_counts") ? 0 : 1;
}
int launch_profile_pair_counts(const mb_machine *m, const PairProfDesc *d, int n, int groupsPerPair, const int *inTok, const double *logP,
                               const double *fwdPool, const double *bwdPool, double *counts, hipStream_t st) {
  return pair_counts<FullGeom>(m, d, {}, n, groupsPerPair, inTok, logP, fwdPool, bwdPool, counts, st);
}
int launch_profile_pair_counts(const mb_machine *m, const PairEnvDesc *d, const PairEnvTables &t, int n, int groupsPerPair, const int *inTok, const double *logP,
                               const double *fwdPool, const double *bwdPool, double *counts, hipStream_t st) {
  return pair_counts<EnvGeom>(m, d, t, n, groupsPerPair, inTok, logP, fwdPool, bwdPool, counts, st);
}

template <template <bool> class Geom>
static int pair_rowpost(const mb_machine *m, const typename Geom<true>::Desc *d, typename Geom<true>::Tables t, int n, int groupsPerPair, int tabMax, const int *inTok,
                        const double *logP, const double *fwdPool, const double *bwdPool, double *post, hipStream_t st) {
  if (n <= 0) return 0;
  k_profile_pair_rowpost<Geom><<<dim3((unsigned)((long long)n * groupsPerPair)), dim3(ROWPOST_THREADS), 0, st>>>(m->dev, d, t, groupsPerPair, inTok, logP, fwdPool, bwdPool, post, tabMax,
                                                                                                              g_deterministic ? 1 : 0);
  return hip_ok(hipGetLastError(), Geom<true>::ENV ? "k_profile_pair_env_rowpost" : "k_profile_pair_rowpost") ? 0 : 1;
}
int launch_profile_pair_rowpost(const mb_machine *m, const PairProfDesc *d, int n, int groupsPerPair, int tabMax, const int *inTok, const double *logP,
                                const double *fwdPool, const double *bwdPool, double *post, hipStream_t st) {
  return pair_rowpost<FullGeom>(m, d, {}, n, groupsPerPair, tabMax, inTok, logP, fwdPool, bwdPool, post, st);
}
int launch_profile_pair_rowpost(const mb_machine *m, const PairEnvDesc *d, const PairEnvTables &t, int n, int groupsPerPair, int tabMax, const int *inTok,
                                const double *logP, const double *fwdPool, const double *bwdPool, double *post, hipStream_t st) {
  return pair_rowpost<EnvGeom>(m, d, t, n, groupsPerPair, tabMax, inTok, logP, fwdPool, bwdPool, post, st);
}

template <template <bool> class Geom>
static int pair_traceback(const mb_machine *m, const typename Geom<true>::Desc *d, typename Geom<true>::Tables t, int n, const int *inTok, const double *logP,
                          const double *pool, uint32_t *edges, int32_t *rows, long long *len, hipStream_t st) {
  if (n <= 0) return 0;
  k_profile_pair_traceback<Geom><<<(n + 63) / 64, 64, 0, st>>>(m->dev, d, t, n, inTok, logP, pool, edges, rows, len);
  return hip_ok(hipGetLastError(), Geom<true>::ENV ? "k_profile_pair_env_traceback" : "k_profile_pair_traceback") ? 0 : 1;
}
int launch_profile_pair_traceback(const mb_machine *m, const PairProfDesc *d, int n, const int *inTok, const double *logP, const double *pool,
                                  uint32_t *edges, int32_t *rows, long long *len, hipStream_t st) {
  return pair_traceback<FullGeom>(m, d, {}, n, inTok, logP, pool, edges, rows, len, st);
}
int launch_profile_pair_traceback(const mb_machine *m, const PairEnvDesc *d, const PairEnvTables &t, int n, const int *inTok, const double *logP, const double *pool,
                                  uint32_t *edges, int32_t *rows, long long *len, hipStream_t st) {
  return pair_traceback<EnvGeom>(m, d, t, n, inTok, logP, pool, edges, rows, len, st);
}

template <template <bool> class Geom>
static int pair_sample(const mb_machine *m, const typename Geom<true>::Desc *d, typename Geom<true>::Tables t, int n, int nSamples, const long long *pairIdx,
                       unsigned long long seed, const int *inTok, const double *logP, const double *pool, uint32_t *edges, int32_t *rows, long long *len,
                       double *logq, hipStream_t st) {
  if (n <= 0) return 0;
  const long long nLanes = (long long)n * nSamples;      // (the caller keeps it within 2^31 - 1)
  k_profile_pair_sample<Geom><<<(unsigned)((nLanes + 63) / 64), 64, 0, st>>>(m->dev, d, t, nLanes, nSamples, pairIdx, seed, inTok, logP, pool, edges, rows, len, logq);
  return hip_ok(hipGetLastError(), Geom<true>::ENV ? "k_profile_pair_env_sample" : "k_profile_pair_sample") ? 0 : 1;
}
int launch_profile_pair_sample(const mb_machine *m, const PairProfDesc *d, int n, int nSamples, const long long *pairIdx, unsigned long long seed, const int *inTok,
                               const double *logP, const double *pool, uint32_t *edges, int32_t *rows, long long *len, double *logq, hipStream_t st) {
  return pair_sample<FullGeom>(m, d, {}, n, nSamples, pairIdx, seed, inTok, logP, pool, edges, rows, len, logq, st);
}
int launch_profile_pair_sample(const mb_machine *m, const PairEnvDesc *d, const PairEnvTables &t, int n, int nSamples, const long long *pairIdx, unsigned long long seed,
                               const int *inTok, const double *logP, const double *pool, uint32_t *edges, int32_t *rows, long long *len, double *logq,
                               hipStream_t st) {
  return pair_sample<EnvGeom>(m, d, t, n, nSamples, pairIdx, seed, inTok, logP, pool, edges, rows, len, logq, st);
}

}  // namespace mb
