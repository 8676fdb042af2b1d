// mb_profile_two.hip -- Forward / Backward / Viterbi / posterior counts / row posteriors of a machine WITH an input alphabet between two PROFILE tapes:
// an input profile A of K rows (the generator of `--generate-csv`) and an output profile B of L rows (`--recognize-csv`) -- the
// semantics of compose(A.machine(), compose(M, transpose(B.machine()))) with both tapes empty, restated in docs/profile_tapes.md
// ("Pairs of profiles"):
//
//   N[i][r][d] = [i = 0, r = 0, d = 0]
//                (+) N[i][r-1][d] + B[r-1][0]                                                          (output blank; r > 0)
//                (+) sum_{t: s->d, in = a, out = o}   ((Z[i-1][r-1][s] + w_t) + A[i-1][a]) + B[r-1][o]   (match; i > 0, r > 0)
//                (+) sum_{t: s->d, in = eps, out = o} (W[i][r-1][s] + w_t) + B[r-1][o]                   (output-only; r > 0)
//   W[i][r][d] = N[i][r][d]
//                (+) sum_{t: s->d, in = a, out = eps} (Z[i-1][r][s] + w_t) + A[i-1][a]                   (input-only; i > 0)
//                (+) sum_{silent t: s->d, s < d}      W[i][r][s] + w_t                                   (silent levels)
//   Z[i][r][d] = W[i][r][d] (+) Z[i-1][r][d] + A[i-1][0]                                                 (input blank; i > 0)
//   loglike    = Z[K][L][S-1]
//
// The generator moves only while the machine waits, so after an input blank only input-reading edges follow: Z feeds the match and
// the input-only edges alone.  The sweep is the one of mb_profile_pair.hip -- one workgroup per pair along the anti-diagonals i + r,
// the work items of a diagonal (cell, state) -- with the edge loops over ALL input tokens (for a destination q the CSR rows
// q*K + a*C + o, a = 1..nIn: they are contiguous from q*K + C to (q + 1)*K) and a third layer.  Z of a state is written by the item
// that finishes its W: the first phase writes it from the W it has, and the phase of the state's silent level writes it again from
// the finished W -- nothing reads Z before the diagonal's last barrier, so the barriers stay at (K + L + 1) nLevF per pair.  The
// rolling sweeps keep a ring of three diagonals of three layers, 3 * 3 * (min(K, L) + 1) * S doubles, in LDS when that fits 160 KiB,
// else in the pair's slice of a global scratch buffer.  Cells are fp64, the sums the exact log-sum-exp.
//
// Every kernel is written once over a GEOMETRY, which says which cells exist and where they live: TwoGeom, the whole rectangle, or
// TwoEnvGeom, the cells of an envelope (docs/profile_tapes.md, "Pairs of profiles under an envelope").  The index rules of both are
// those of mb_profile_lattice.h; TwoLattice below adds the three layers.  All three layers of a cell outside the envelope are -inf,
// so a neighbour outside is not read -- the input blank Z[i-1][r] -> Z[i][r] is a move along i like any other and is left out when
// (i-1, r) is outside; the recurrence, the candidate order and the sums are the same text for both.
#include "mb_profile_common.h"
#include "mb_profile_two_env.h"

namespace mb {

size_t profile_two_lds_bytes(int S, long long nIn, long long nRows) {
  const double b = (double)profile_two_ring(S, nIn, nRows) * sizeof(double);
  return b <= (double)SWEEP_LDS_MAX ? (size_t)b : 0;
}
size_t profile_two_env_lds_bytes(int S, long long M) {
  const double b = (double)profile_two_env_ring(S, M) * sizeof(double);
  return b <= (double)SWEEP_LDS_MAX ? (size_t)b : 0;
}

// A pair's lattice: the cells of mb_profile_lattice.h, RectCells or EnvCells, with three layers of S doubles in each.  MAT: the
// materialised lattice of mb_profile_two.h (the compact one of mb_profile_two_env.h) at base, else the ring.
template <class Cells, bool MAT>
struct TwoLattice : Cells {
  using Desc = std::conditional_t<Cells::ENV, TwoEnvDesc, PairProfDesc>;
  using Tables = std::conditional_t<Cells::ENV, TwoEnvTables, NoTables>;
  double *base;
  int S;
  __device__ __forceinline__ TwoLattice(const Desc &pd, const Tables &t, double *base, int S) : Cells(lattice_cells(pd, t)), base(base), S(S) {}
  __device__ __forceinline__ double *at(int i, int r, int layer) const { return base + ((MAT ? this->index(i, r) : this->slot(i, r)) * 3 + layer) * S; }
};
template <bool MAT> using TwoGeom = TwoLattice<RectCells, MAT>;
template <bool MAT> using TwoEnvGeom = TwoLattice<EnvCells, MAT>;

// Forward (MODE = MB_FORWARD) or Viterbi (MB_VITERBI) sweep.  MAT: every cell into pool, else rolling.  Viterbi keeps the FIRST
// maximum: N takes the output blank first, then the match edges, then the output-only edges; W takes N (no move) first, then the
// input-only edges, then the silent edges; Z takes W first, then the input blank; edges of a kind in `incoming` order (input token
// ascending, then output token) -- the order k_profile_two_traceback re-enumerates.
template <int MODE, bool MAT, template <bool> class Geom>
__global__ __launch_bounds__(SWEEP_THREADS) void k_profile_two_fwd(DevMachine m, const typename Geom<MAT>::Desc *__restrict__ descs, typename Geom<MAT>::Tables t,
                                                                   const double *__restrict__ logA, const double *__restrict__ logB, double *pool, double *scratch,
                                                                   double *__restrict__ loglike) {
  extern __shared__ double pt_sh[];
  const auto pd = descs[blockIdx.x];
  const int S = m.S, KK = m.K, C = m.nOut + 1, CA = m.nIn + 1, K = pd.nIn, L = pd.nRows;
  const double *A = logA + pd.inBase * CA;
  const double *B = logB + pd.rowBase * C;
  const Geom<MAT> lat(pd, t, MAT ? pool + pd.cellBase : (pd.ringBase < 0 ? pt_sh : scratch + pd.ringBase), S);
  for (int d = 0; d <= K + L; ++d) {
    int ilo, nCells;
    lat.diag(d, ilo, nCells);
    const int nItems = nCells * S;
    for (int it = threadIdx.x; it < nItems; it += blockDim.x) {
      const int c = it / S, q = it - c * S, i = ilo + c, r = d - i;
      const double *Ai = A + (long long)max(i - 1, 0) * CA;      // row i - 1; read when i > 0
      double acc;
      if (r > 0) {
        const double *Br = B + (long long)(r - 1) * C;
        const bool up = lat.inside(i, r - 1);
        acc = up ? lat.at(i, r - 1, 0)[q] + Br[0] : -INFINITY;
        if (i > 0 && lat.inside(i - 1, r - 1)) {
          const double *Zd = lat.at(i - 1, r - 1, 2);
          for (int a = 1; a <= m.nIn; ++a) {
            const int row = q * KK + a * C;
            const double wa = Ai[a];
            const int e1 = m.inOff[row + C];
            for (int e = m.inOff[row + 1]; e < e1; ++e)
              acc = red<MODE>(acc, ((Zd[m.inSrc[e]] + m.inW[e]) + wa) + Br[m.eOutTok[m.inEid[e]]]);
          }
        }
        if (up) {
          const double *Wu = lat.at(i, r - 1, 1);
          const int e1 = m.inOff[q * KK + C];
          for (int e = m.inOff[q * KK + 1]; e < e1; ++e)
            acc = red<MODE>(acc, (Wu[m.inSrc[e]] + m.inW[e]) + Br[m.eOutTok[m.inEid[e]]]);
        }
      } else {
        acc = (i == 0 && q == 0) ? 0.0 : -INFINITY;
      }
      lat.at(i, r, 0)[q] = acc;
      if (i > 0 && lat.inside(i - 1, r)) {
        const double *Zl = lat.at(i - 1, r, 2);
        for (int a = 1; a <= m.nIn; ++a) {
          const int row = q * KK + a * C;
          const double wa = Ai[a];
          const int e1 = m.inOff[row + 1];
          for (int e = m.inOff[row]; e < e1; ++e) acc = red<MODE>(acc, (Zl[m.inSrc[e]] + m.inW[e]) + wa);
        }
        lat.at(i, r, 1)[q] = acc;
        lat.at(i, r, 2)[q] = red<MODE>(acc, Zl[q] + Ai[0]);
      } else {
        lat.at(i, r, 1)[q] = acc;
        lat.at(i, r, 2)[q] = acc;
      }
    }
    __syncthreads();
    for (int lev = 1; lev < m.nLevF; ++lev) {      // (level 0 has no silent edge coming in: its W and Z are complete)
      const int l0 = m.levFOff[lev], ns = m.levFOff[lev + 1] - l0;
      const int nLevItems = nCells * ns;
      for (int it = threadIdx.x; it < nLevItems; it += blockDim.x) {
        const int c = it / ns, q = m.levFState[l0 + (it - c * ns)], i = ilo + c, r = d - i;
        double *Wc = lat.at(i, r, 1);
        double acc = Wc[q];
        const int e1 = m.inOff[q * KK + 1];
        for (int e = m.inOff[q * KK]; e < e1; ++e) {
          const int s = (int)m.inSrc[e];
          if (s >= q) continue;                       // as the token sweeps: a silent self-loop never fires
          acc = red<MODE>(acc, Wc[s] + m.inW[e]);
        }
        Wc[q] = acc;
        lat.at(i, r, 2)[q] = (i > 0 && lat.inside(i - 1, r)) ? red<MODE>(acc, lat.at(i - 1, r, 2)[q] + A[(long long)(i - 1) * CA]) : acc;
      }
      __syncthreads();
    }
  }
  if (threadIdx.x == 0) loglike[blockIdx.x] = lat.at(K, L, 2)[S - 1];      // (an envelope is connected: (0, 0) and (K, L) are inside)
}

// Materialised Backward sweep, layer 0 = NB ("from the arrived stage"), 1 = WB ("from the waiting stage"), 2 = ZB ("from the
// committed stage"):
//   ZB[i][r][s] = [i = K, r = L, s = S-1]
//                 (+) A[i][0] + ZB[i+1][r][s]                                                    (i < K)
//                 (+) sum_{t: s->d, in = a, out = o}   ((w_t + A[i][a]) + B[r][o]) + NB[i+1][r+1][d]   (i < K, r < L)
//                 (+) sum_{t: s->d, in = a, out = eps} (w_t + A[i][a]) + WB[i+1][r][d]                 (i < K)
//   WB[i][r][s] = ZB[i][r][s]
//                 (+) sum_{t: s->d, in = eps, out = o} (w_t + B[r][o]) + NB[i][r+1][d]                 (r < L)
//                 (+) sum_{silent t: s->d, s < d}      w_t + WB[i][r][d]
//   NB[i][r][s] = WB[i][r][s] (+) (B[r][0] + NB[i][r+1][s])   (r < L);   loglike = NB[0][0][0]
// Anti-diagonals from K + L down.  A state's WB is final once its backward level has run; the item that finishes it writes its NB.
// A successor cell outside the geometry contributes nothing.
template <template <bool> class Geom>
__global__ __launch_bounds__(SWEEP_THREADS) void k_profile_two_bwd(DevMachine m, const typename Geom<true>::Desc *__restrict__ descs, typename Geom<true>::Tables t,
                                                                   const double *__restrict__ logA, const double *__restrict__ logB, double *pool,
                                                                   double *__restrict__ loglike) {
  const auto pd = descs[blockIdx.x];
  const int S = m.S, KK = m.K, C = m.nOut + 1, CA = m.nIn + 1, K = pd.nIn, L = pd.nRows;
  const double *A = logA + pd.inBase * CA;
  const double *B = logB + pd.rowBase * C;
  const Geom<true> lat(pd, t, pool + pd.cellBase, S);
  for (int d = K + L; d >= 0; --d) {
    int ilo, nCells;
    lat.diag(d, ilo, nCells);
    const int nItems = nCells * S;
    for (int it = threadIdx.x; it < nItems; it += blockDim.x) {
      const int c = it / S, s = it - c * S, i = ilo + c, r = d - i;
      const double *Ai = A + (long long)i * CA;      // read when i < K
      const double *Br = B + (long long)r * C;       // read when r < L
      const bool right = i < K && lat.inside(i + 1, r), down = r < L && lat.inside(i, r + 1);
      double v = (i == K && r == L && s == S - 1) ? 0.0 : -INFINITY;
      if (i < K) {
        if (right) v = lse2_exact(v, Ai[0] + lat.at(i + 1, r, 2)[s]);
        if (r < L && lat.inside(i + 1, r + 1)) {
          const double *Nd = lat.at(i + 1, r + 1, 0);
          for (int a = 1; a <= m.nIn; ++a) {
            const int row = s * KK + a * C;
            const double wa = Ai[a];
            const int e1 = m.outOff[row + C];
            for (int e = m.outOff[row + 1]; e < e1; ++e)
              v = lse2_exact(v, ((m.outW[e] + wa) + Br[m.eOutTok[m.outEid[e]]]) + Nd[m.outDst[e]]);
          }
        }
        if (right) {
          const double *Wl = lat.at(i + 1, r, 1);
          for (int a = 1; a <= m.nIn; ++a) {
            const int row = s * KK + a * C;
            const double wa = Ai[a];
            const int e1 = m.outOff[row + 1];
            for (int e = m.outOff[row]; e < e1; ++e) v = lse2_exact(v, (m.outW[e] + wa) + Wl[m.outDst[e]]);
          }
        }
      }
      lat.at(i, r, 2)[s] = v;
      if (down) {
        const double *Nu = lat.at(i, r + 1, 0);
        const int e1 = m.outOff[s * KK + C];
        for (int e = m.outOff[s * KK + 1]; e < e1; ++e)
          v = lse2_exact(v, (m.outW[e] + Br[m.eOutTok[m.outEid[e]]]) + Nu[m.outDst[e]]);
      }
      lat.at(i, r, 1)[s] = v;
      lat.at(i, r, 0)[s] = down ? lse2_exact(v, Br[0] + lat.at(i, r + 1, 0)[s]) : v;
    }
    __syncthreads();
    for (int lev = 1; lev < m.nLevB; ++lev) {
      const int l0 = m.levBOff[lev], ns = m.levBOff[lev + 1] - l0;
      const int nLevItems = nCells * ns;
      for (int it = threadIdx.x; it < nLevItems; it += blockDim.x) {
        const int c = it / ns, s = m.levBState[l0 + (it - c * ns)], i = ilo + c, r = d - i;
        double *Wc = lat.at(i, r, 1);
        double v = Wc[s];
        const int e1 = m.outOff[s * KK + 1];
        for (int e = m.outOff[s * KK]; e < e1; ++e) {
          const int t = (int)m.outDst[e];
          if (t <= s) continue;
          v = lse2_exact(v, Wc[t] + m.outW[e]);
        }
        Wc[s] = v;
        lat.at(i, r, 0)[s] = (r < L && lat.inside(i, r + 1)) ? lse2_exact(v, B[(long long)r * C] + lat.at(i, r + 1, 0)[s]) : v;
      }
      __syncthreads();
    }
  }
  if (threadIdx.x == 0) loglike[blockIdx.x] = lat.at(0, 0, 0)[0];
}

// Posterior counts.  With both lattices in memory every (cell, edge) term is independent:
//   count[t] += exp(F[i][r][s] - LL + term_t), term_t the edge's summand of ZB (read from Z_F) or WB (read from W_F) above,
// so the sweep is a flat grid over (pair, group of the pair, (cell, state)), accumulated by CountsAcc (mb_profile_common.h).  A pair
// whose likelihood is -inf adds nothing; the blanks of either tape are not edges.  The cells of an envelope are counted through its
// compact index (a cell finds its row by bisection in off); a term whose destination lies outside is left out.
template <template <bool> class Geom>
__global__ __launch_bounds__(256) void k_profile_two_counts(DevMachine m, const typename Geom<true>::Desc *__restrict__ descs, typename Geom<true>::Tables t, int groupsPerPair,
                                                            const double *__restrict__ logA, const double *__restrict__ logB, const double *__restrict__ fwdPool,
                                                            const double *__restrict__ bwdPool, long long nTrans, double *__restrict__ counts, int det) {
  __shared__ double lcount[COUNTS_LDS_MAX];
  const CountsAcc acc(lcount, counts, nTrans, det);
  const int k = blockIdx.x / groupsPerPair, group = blockIdx.x % groupsPerPair;
  const auto pd = descs[k];
  const int S = m.S, KK = m.K, C = m.nOut + 1, CA = m.nIn + 1, K = pd.nIn, L = pd.nRows;
  const double *A = logA + pd.inBase * CA;
  const double *B = logB + pd.rowBase * C;
  const Geom<true> F(pd, t, const_cast<double *>(fwdPool) + pd.cellBase, S), Bk(pd, t, const_cast<double *>(bwdPool) + pd.cellBase, S);
  const double LL = F.at(K, L, 2)[S - 1];
  if (LL > -INFINITY) {
    const long long nItems = F.cells() * S;
    for (long long idx = (long long)group * blockDim.x + threadIdx.x; idx < nItems; idx += (long long)groupsPerPair * blockDim.x) {
      const long long cell = idx / S;
      const int s = (int)(idx - cell * S);
      int i, r;
      F.cell(cell, i, r);
      const double f = F.at(i, r, 1)[s] - LL, z = F.at(i, r, 2)[s] - LL;
      if (!(z > -INFINITY)) continue;                 // (Z holds W: a dead Z is a dead W)
      const double *Ai = A + (long long)i * CA;
      const double *Br = B + (long long)r * C;
      if (i < K) {
        const bool right = Bk.inside(i + 1, r), across = r < L && Bk.inside(i + 1, r + 1);
        const double *Wl = right ? Bk.at(i + 1, r, 1) : nullptr, *Nd = across ? Bk.at(i + 1, r + 1, 0) : nullptr;
        for (int a = 1; a <= m.nIn; ++a) {
          const int row = s * KK + a * C;
          const double wa = Ai[a];
          if (across) {
            const int e1 = m.outOff[row + C];
            for (int e = m.outOff[row + 1]; e < e1; ++e)
              acc.add(m.outEid[e], exp(z + (((m.outW[e] + wa) + Br[m.eOutTok[m.outEid[e]]]) + Nd[m.outDst[e]])));
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
        const int e1 = m.outOff[s * KK + C];
        for (int e = m.outOff[s * KK + 1]; e < e1; ++e)
          acc.add(m.outEid[e], exp(f + ((m.outW[e] + Br[m.eOutTok[m.outEid[e]]]) + Nu[m.outDst[e]])));
      }
      const double *Wc = Bk.at(i, r, 1);
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

// Row posteriors of both tapes (docs/profile_tapes.md, "Row posteriors of pairs of profiles"): the terms of k_profile_two_counts and
// the two blank masses, binned by (line, column) instead of by transition.  AXIS 0 bins output rows -- post[(rowBase + r) * C + o] is
// the gradient of the log-likelihood in B[r][o]:
//   post[r][0] = sum_i sum_s exp((N_F[i][r][s] - LL) + (B[r][0] + NB[i][r+1][s]))
//   post[r][o] = the match terms (read from Z_F) and the output-only terms (read from W_F) whose edge writes o
// AXIS 1 bins input rows -- post[(inBase + i) * CA + a] is the gradient in A[i][a]:
//   post[i][0] = sum_r sum_s exp((Z_F[i][r][s] - LL) + (A[i][0] + ZB[i+1][r][s]))
//   post[i][a] = the input-only and the match terms (both read from Z_F) whose edge reads a
// The scheme is the one of k_profile_pair_rowpost: the work items are (line, cell of the line, state) in that order -- over the full
// rectangle both orders are a division -- and a workgroup owns whole lines, blocks of profile_pair_rowpost_rows lines dealt round
// robin to the pair's groups.  A lane sums its terms of one column in a register, in CSR order (axis 0, column o: the rows
// s*K + a*C + o for a = 1..nIn, then s*K + o; axis 1, column a: the rows s*K + a*C + o for o = 0..nOut); rowpost_add reduces the lane
// sums of a wavefront that lies in one line and adds to the workgroup's LDS table, which is then stored: every bin has one writing
// workgroup, so there is no global atomic and nothing to clear beforehand.  A line of more than tabMax columns is summed in its
// global bins instead, cleared by the workgroup that owns it.  A pair whose likelihood is -inf gets zeros.  det: post holds 64-bit
// fixed point at 2^-36.
// Under an envelope the lines are those of the geometry (lineFirst / lineCell): on axis 0 the compact index already counts row by
// row; on axis 1 the lines are COLUMNS of the envelope -- by monotonicity the cells of input row i are the run r = colStart[i] ..
// colEnd[i] - 1, an item finds its column by bisection in colOff and its cell through at().  A term whose destination lies outside
// is left out.
template <int AXIS, template <bool> class Geom>
__global__ __launch_bounds__(ROWPOST_THREADS) void k_profile_two_rowpost(DevMachine m, const typename Geom<true>::Desc *__restrict__ descs, typename Geom<true>::Tables t,
                                                                         int groupsPerPair, const double *__restrict__ logA, const double *__restrict__ logB,
                                                                         const double *__restrict__ fwdPool, const double *__restrict__ bwdPool,
                                                                         double *post, int tabMax, int det) {
  __shared__ double ltab[ROWPOST_LDS_MAX];
  const int k = blockIdx.x / groupsPerPair, group = blockIdx.x % groupsPerPair;
  const auto pd = descs[k];
  const int S = m.S, KK = m.K, C = m.nOut + 1, CA = m.nIn + 1, K = pd.nIn, L = pd.nRows;
  const int NL = AXIS ? K : L, NC = AXIS ? CA : C;      // lines, bins of a line
  if (NL == 0) return;
  const double *A = logA + pd.inBase * CA;
  const double *B = logB + pd.rowBase * C;
  const Geom<true> F(pd, t, const_cast<double *>(fwdPool) + pd.cellBase, S), Bk(pd, t, const_cast<double *>(bwdPool) + pd.cellBase, S);
  const double LL = F.at(K, L, 2)[S - 1];
  const int R = profile_pair_rowpost_rows(F.cells(), S, NL, NC, tabMax);
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
      const long long c0 = F.template lineFirst<AXIS>(l0), nItems = (F.template lineFirst<AXIS>(l1) - c0) * S;
      for (long long base = threadIdx.x - lane; base < nItems; base += blockDim.x) {      // (a wavefront stays whole in here)
        const long long idx = base + lane;
        const bool valid = idx < nItems;
        int i = AXIS ? l0 : 0, r = AXIS ? 0 : l0, s = 0;
        if (valid) {
          const long long cell = idx / S;
          s = (int)(idx - cell * S);
          F.template lineCell<AXIS>(c0 + cell, i, r);
        }
        const int line = AXIS ? i : r;
        const double z = valid ? F.at(i, r, 2)[s] - LL : -INFINITY;
        const bool whole = __all(valid && line == __shfl(line, 0));
        // (the line's own coordinate is inside: r < L on axis 0, i < K on axis 1)
        const bool diag = valid && i < K && r < L && Bk.inside(i + 1, r + 1);
        const double *Ai = A + (long long)i * CA;        // read when i < K
        const double *Br = B + (long long)r * C;         // read when r < L
        const double *Nd = diag ? Bk.at(i + 1, r + 1, 0) : nullptr;
        const int sRow = s * KK, bin0 = (line - l0) * NC;
        if (AXIS == 0) {
          const double f = valid ? F.at(i, r, 1)[s] - LL : -INFINITY, n = valid ? F.at(i, r, 0)[s] - LL : -INFINITY;
          const bool up = valid && Bk.inside(i, r + 1);
          const double *Nu = up ? Bk.at(i, r + 1, 0) : nullptr;
          const bool zLive = diag && z > -INFINITY, fLive = up && f > -INFINITY;
          rowpost_add(tab, bin0, (up && n > -INFINITY) ? exp(n + (Br[0] + Nu[s])) : 0.0, whole, lane, det);
          for (int o = 1; o < C; ++o) {      // the out-edges of (s, a) that write o are one CSR row
            double v = 0.0;
            const double po = Br[o];
            if (zLive)
              for (int a = 1; a <= m.nIn; ++a) {
                const int row = sRow + a * C + o;
                const double wa = Ai[a];
                const int e1 = m.outOff[row + 1];
                for (int e = m.outOff[row]; e < e1; ++e) v += exp(z + (((m.outW[e] + wa) + po) + Nd[m.outDst[e]]));
              }
            if (fLive) {
              const int e1 = m.outOff[sRow + o + 1];
              for (int e = m.outOff[sRow + o]; e < e1; ++e) v += exp(f + ((m.outW[e] + po) + Nu[m.outDst[e]]));
            }
            rowpost_add(tab, bin0 + o, v, whole, lane, det);
          }
        } else {
          const bool right = valid && Bk.inside(i + 1, r);
          const double *Zl = right ? Bk.at(i + 1, r, 2) : nullptr, *Wl = right ? Bk.at(i + 1, r, 1) : nullptr;
          const bool zLive = z > -INFINITY;
          rowpost_add(tab, bin0, (right && zLive) ? exp(z + (Ai[0] + Zl[s])) : 0.0, whole, lane, det);
          for (int a = 1; a < CA; ++a) {      // the out-edges of s that read a: the input-only row, then the rows of the output tokens
            double v = 0.0;
            if (zLive) {
              const int row = sRow + a * C;
              const double wa = Ai[a];
              if (right) {
                const int e1 = m.outOff[row + 1];
                for (int e = m.outOff[row]; e < e1; ++e) v += exp(z + ((m.outW[e] + wa) + Wl[m.outDst[e]]));
              }
              if (diag) {
                const int e1 = m.outOff[row + C];
                for (int e = m.outOff[row + 1]; e < e1; ++e)
                  v += exp(z + (((m.outW[e] + wa) + Br[m.eOutTok[m.outEid[e]]]) + Nd[m.outDst[e]]));
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

// Viterbi traceback over a materialised max lattice, one lane per pair: from Z[K][L][S-1] back to N[0][0][0], taking at every cell
// the first candidate (in the fill's order) whose value equals the cell.  Edges go start -> end into the pair's slot
// (profile_pair_path_bound entries) with both coordinates at which each fired: an emitting edge the output row it consumed, an
// output-less edge the number of output rows consumed before it, and the same on the input tape.  len = -1: no finite path, -2: the
// slot was too small, -3: no candidate matched (a corrupt matrix).
// A candidate whose source cell lies outside the geometry is left out: it is -inf, and the cells on the path are finite.
template <template <bool> class Geom>
__global__ void k_profile_two_traceback(DevMachine m, const typename Geom<true>::Desc *__restrict__ descs, typename Geom<true>::Tables t, int n,
                                        const double *__restrict__ logA, const double *__restrict__ logB, const double *__restrict__ pool, uint32_t *edges,
                                        int32_t *rows, int32_t *inRows, long long *len) {
  const int k = blockIdx.x * blockDim.x + threadIdx.x;
  if (k >= n) return;
  const auto pd = descs[k];
  const int S = m.S, KK = m.K, C = m.nOut + 1, CA = m.nIn + 1, K = pd.nIn, L = pd.nRows;
  const double *A = logA + pd.inBase * CA;
  const double *B = logB + pd.rowBase * C;
  const Geom<true> lat(pd, t, const_cast<double *>(pool) + pd.cellBase, S);
  uint32_t *pe = edges + pd.pathBase;
  int32_t *pr = rows + pd.pathBase, *pi = inRows + pd.pathBase;
  int i = K, r = L, q = S - 1, layer = 2;
  const long long cap = K + L + (long long)(K + L + 1) * (m.nLevF - 1);
  long long cnt = 0;
  if (!(lat.at(i, r, 2)[q] > -INFINITY)) { len[k] = -1; return; }
  for (;;) {
    const double *Ai = A + (long long)max(i - 1, 0) * CA;      // row i - 1; read when i > 0
    int e = 0, found = -1;
    if (layer == 2) {
      const double cur = lat.at(i, r, 2)[q];
      if (lat.at(i, r, 1)[q] == cur) { layer = 1; continue; }
      if (i > 0 && lat.inside(i - 1, r) && lat.at(i - 1, r, 2)[q] + Ai[0] == cur) { --i; continue; }
      len[k] = -3; return;
    } else if (layer == 1) {
      const double *W = lat.at(i, r, 1);
      const double cur = W[q];
      if (lat.at(i, r, 0)[q] == cur) { layer = 0; continue; }
      int ni = i, nl = 1;
      if (i > 0 && lat.inside(i - 1, r)) {
        const double *Zl = lat.at(i - 1, r, 2);
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
      if (found < 0) { len[k] = -3; return; }
      if (cnt >= cap) { len[k] = -2; return; }
      pe[cnt] = m.inEid[e]; pr[cnt] = r; pi[cnt] = ni; ++cnt;
      i = ni; q = found; layer = nl;
    } else {
      if (r == 0) { if (i != 0 || q != 0) { len[k] = -3; return; } break; }
      const double *Br = B + (long long)(r - 1) * C;
      const double cur = lat.at(i, r, 0)[q];
      const bool up = lat.inside(i, r - 1);
      if (up && lat.at(i, r - 1, 0)[q] + Br[0] == cur) { --r; continue; }
      int ni = i, nl = 1;
      if (i > 0 && lat.inside(i - 1, r - 1)) {
        const double *Zd = lat.at(i - 1, r - 1, 2);
        for (int a = 1; a <= m.nIn && found < 0; ++a) {
          const int row = q * KK + a * C;
          const double wa = Ai[a];
          e = m.inOff[row + 1];
          for (const int e1 = m.inOff[row + C]; e < e1; ++e)
            if (((Zd[m.inSrc[e]] + m.inW[e]) + wa) + Br[m.eOutTok[m.inEid[e]]] == cur) { found = (int)m.inSrc[e]; ni = i - 1; nl = 2; break; }
        }
      }
      if (found < 0 && up) {
        const double *Wu = lat.at(i, r - 1, 1);
        e = m.inOff[q * KK + 1];
        for (const int e1 = m.inOff[q * KK + C]; e < e1; ++e)
          if ((Wu[m.inSrc[e]] + m.inW[e]) + Br[m.eOutTok[m.inEid[e]]] == cur) { found = (int)m.inSrc[e]; break; }
      }
      if (found < 0) { len[k] = -3; return; }
      if (cnt >= cap) { len[k] = -2; return; }
      --r;
      pe[cnt] = m.inEid[e]; pr[cnt] = r; pi[cnt] = ni; ++cnt;
      i = ni; q = found; layer = nl;
    }
  }
  reverse_path(cnt, pe, pr, pi);
  len[k] = cnt;
}

// Posterior path samples over a materialised SUM lattice (docs/profile_tapes.md, "Posterior path samples of pairs of profiles"), one
// lane per (pair, sample) as k_profile_pair_sample (mb_profile_pair.hip): lane id serves pair id / nSamples of the chunk, sample
// id % nSamples.  From Z[K][L][S-1] back to N[0][0][0]; every Z cell with i > 0, every W cell and every N cell with r > 0 is one
// decision among the terms of the fill, in the fill's order and parenthesisation -- the list k_profile_two_traceback enumerates --
// each with probability exp(term - cell).  A Z cell with i = 0 holds its W and draws nothing; a Z cell whose input blank lies
// outside the geometry has one candidate and still takes a counter value.  The uniform of decision t of sample j of pair k
// (pair0 + the pair's place in the chunk: its index in the object) is philox_uniform(t, j, k, seed).  SampleDraw's kind: 0 the
// candidate without an edge (wait, stay, the output blank; at a Z cell 1 is the input blank), 1 an edge that reads an input row
// (its source is a Z cell), 2 an edge that reads none (its source is a W cell).  Edges and both coordinates go into the sample's
// slot, at (pathBase * nSamples + j * bound), backwards and are reversed at the end; len and logq are k_profile_pair_sample's.
template <template <bool> class Geom>
__global__ __launch_bounds__(64) void k_profile_two_sample(DevMachine m, const typename Geom<true>::Desc *__restrict__ descs, typename Geom<true>::Tables t, long long nLanes,
                                                           int nSamples, long long pair0, unsigned long long seed, const double *__restrict__ logA,
                                                           const double *__restrict__ logB, const double *__restrict__ pool, uint32_t *edges, int32_t *rows,
                                                           int32_t *inRows, long long *len, double *logq) {
  const long long id = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (id >= nLanes) return;
  const int slot = (int)(id / nSamples), j = (int)(id - (long long)slot * nSamples);
  const auto pd = descs[slot];
  const unsigned long long k = (unsigned long long)(pair0 + slot);
  const uint32_t k0 = (uint32_t)seed, k1 = (uint32_t)(seed >> 32), c2 = (uint32_t)k, c3 = (uint32_t)(k >> 32);
  const int S = m.S, KK = m.K, C = m.nOut + 1, CA = m.nIn + 1, K = pd.nIn, L = pd.nRows;
  const double *A = logA + pd.inBase * CA;
  const double *B = logB + pd.rowBase * C;
  const Geom<true> lat(pd, t, const_cast<double *>(pool) + pd.cellBase, S);
  const long long cap = K + L + (long long)(K + L + 1) * (m.nLevF - 1);
  const long long at = pd.pathBase * nSamples + (long long)j * cap;
  uint32_t *pe = edges + at;
  int32_t *pr = rows + at, *pi = inRows + at;
  int i = K, r = L, q = S - 1, layer = 2;
  long long cnt = 0;
  uint32_t dec = 0;
  double lq = 0.0;
  if (!(lat.at(i, r, 2)[q] > -INFINITY)) { len[id] = -1; logq[id] = -INFINITY; return; }
  for (;;) {
    if (layer == 2 && i == 0) layer = 1;      // (Z[0][r] is W[0][r]: nothing to decide)
    if (layer == 0 && r == 0) { if (i != 0 || q != 0) { len[id] = -3; logq[id] = lq; return; } break; }
    const double *Ai = A + (long long)max(i - 1, 0) * CA;      // row i - 1; read when i > 0
    const double *Br = B + (long long)max(r - 1, 0) * C;       // row r - 1; read at an N cell
    SampleDraw d(philox_uniform(dec++, (uint32_t)j, c2, c3, k0, k1), lat.at(i, r, layer)[q]);
    if (layer == 2) {
      d.offer(lat.at(i, r, 1)[q], 0, 0, q);
      if (lat.inside(i - 1, r)) d.offer(lat.at(i - 1, r, 2)[q] + Ai[0], 1, 0, q);
    } else if (layer == 1) {
      const double *W = lat.at(i, r, 1);
      d.offer(lat.at(i, r, 0)[q], 0, 0, q);
      if (i > 0 && lat.inside(i - 1, r)) {
        const double *Zl = lat.at(i - 1, r, 2);
        for (int a = 1; a <= m.nIn && !d.done; ++a) {
          const int row = q * KK + a * C;
          const double wa = Ai[a];
          const int e1 = m.inOff[row + 1];
          for (int e = m.inOff[row]; e < e1 && !d.done; ++e) d.offer((Zl[m.inSrc[e]] + m.inW[e]) + wa, 1, e, (int)m.inSrc[e]);
        }
      }
      const int e1 = m.inOff[q * KK + 1];
      for (int e = m.inOff[q * KK]; e < e1 && !d.done; ++e) {
        const int s = (int)m.inSrc[e];
        if (s < q) d.offer(W[s] + m.inW[e], 2, e, s);
      }
    } else {
      const bool up = lat.inside(i, r - 1);
      if (up) d.offer(lat.at(i, r - 1, 0)[q] + Br[0], 0, 0, q);
      if (i > 0 && lat.inside(i - 1, r - 1)) {
        const double *Zd = lat.at(i - 1, r - 1, 2);
        for (int a = 1; a <= m.nIn && !d.done; ++a) {
          const int row = q * KK + a * C;
          const double wa = Ai[a];
          const int e1 = m.inOff[row + C];
          for (int e = m.inOff[row + 1]; e < e1 && !d.done; ++e)
            d.offer(((Zd[m.inSrc[e]] + m.inW[e]) + wa) + Br[m.eOutTok[m.inEid[e]]], 1, e, (int)m.inSrc[e]);
        }
      }
      if (up) {
        const double *Wu = lat.at(i, r - 1, 1);
        const int e1 = m.inOff[q * KK + C];
        for (int e = m.inOff[q * KK + 1]; e < e1 && !d.done; ++e)
          d.offer((Wu[m.inSrc[e]] + m.inW[e]) + Br[m.eOutTok[m.inEid[e]]], 2, e, (int)m.inSrc[e]);
      }
    }
    if (d.kind < 0) { len[id] = -3; logq[id] = lq; return; }
    lq += d.term - d.cur;
    if (layer == 2) {      // wait, or the input blank: no edge
      if (d.kind == 0) layer = 1; else --i;
      continue;
    }
    if (layer == 0) --r;
    if (d.kind == 0) { layer = 0; continue; }      // (stay: W -> N; the output blank: N -> N)
    if (cnt >= cap) { len[id] = -2; logq[id] = lq; return; }
    if (d.kind == 1) --i;
    pe[cnt] = m.inEid[d.a]; pr[cnt] = r; pi[cnt] = i; ++cnt;
    q = d.src; layer = d.kind == 1 ? 2 : 1;
  }
  reverse_path(cnt, pe, pr, pi);
  len[id] = cnt;
  logq[id] = lq;
}

// The launchers: each sweep once over a geometry, and the two overloads of the headers that name one.
template <template <bool> class Geom>
static int two_fwd(const mb_machine *m, int mode, bool mat, const typename Geom<true>::Desc *d, typename Geom<true>::Tables t, int n, size_t lds, long long maxItems,
                   const double *logA, const double *logB, double *pool, double *scratch, double *loglike, hipStream_t st) {
  constexpr bool ENV = Geom<true>::ENV;
  if (n <= 0) return 0;
  if (mat) lds = 0;
  static size_t ldsAllowed = 64 * 1024;
  if (!allow_sweep_lds(ldsAllowed, lds, {(const void *)&k_profile_two_fwd<MB_FORWARD, false, Geom>, (const void *)&k_profile_two_fwd<MB_VITERBI, false, Geom>},
                       ENV ? "k_profile_two_env_fwd: raising the LDS limit" : "k_profile_two_fwd: raising the LDS limit")) return 1;
  const dim3 g(n), b(sweep_threads(maxItems));
  if (mode == MB_VITERBI) {
    if (mat) k_profile_two_fwd<MB_VITERBI, true, Geom><<<g, b, 0, st>>>(m->dev, d, t, logA, logB, pool, scratch, loglike);
    else k_profile_two_fwd<MB_VITERBI, false, Geom><<<g, b, lds, st>>>(m->dev, d, t, logA, logB, pool, scratch, loglike);
  } else {
    if (mat) k_profile_two_fwd<MB_FORWARD, true, Geom><<<g, b, 0, st>>>(m->dev, d, t, logA, logB, pool, scratch, loglike);
    else k_profile_two_fwd<MB_FORWARD, false, Geom><<<g, b, lds, st>>>(m->dev, d, t, logA, logB, pool, scratch, loglike);
  }
  return hip_ok(hipGetLastError(), ENV ? "k_profile_two_env_fwd" : "k_profile_two_fwd") ? 0 : 1;
}
int launch_profile_two_fwd(const mb_machine *m, int mode, bool mat, const PairProfDesc *d, int n, size_t lds, long long maxItems, const double *logA,
                           const double *logB, double *pool, double *scratch, double *loglike, hipStream_t st) {
  return two_fwd<TwoGeom>(m, mode, mat, d, {}, n, lds, maxItems, logA, logB, pool, scratch, loglike, st);
}
int launch_profile_two_fwd(const mb_machine *m, int mode, bool mat, const TwoEnvDesc *d, const TwoEnvTables &t, int n, size_t lds, long long maxItems,
                           const double *logA, const double *logB, double *pool, double *scratch, double *loglike, hipStream_t st) {
  return two_fwd<TwoEnvGeom>(m, mode, mat, d, t, n, lds, maxItems, logA, logB, pool, scratch, loglike, st);
}

template <template <bool> class Geom>
static int two_bwd(const mb_machine *m, const typename Geom<true>::Desc *d, typename Geom<true>::Tables t, int n, long long maxItems, const double *logA,
                   const double *logB, double *pool, double *loglike, hipStream_t st) {
  if (n <= 0) return 0;
  k_profile_two_bwd<Geom><<<dim3(n), dim3(sweep_threads(maxItems)), 0, st>>>(m->dev, d, t, logA, logB, pool, loglike);
  return hip_ok(hipGetLastError(), Geom<true>::ENV ? "k_profile_two_env_bwd" : "k_profile_two_bwd") ? 0 : 1;
}
int launch_profile_two_bwd(const mb_machine *m, const PairProfDesc *d, int n, long long maxItems, const double *logA, const double *logB, double *pool,
                           double *loglike, hipStream_t st) {
  return two_bwd<TwoGeom>(m, d, {}, n, maxItems, logA, logB, pool, loglike, st);
}
int launch_profile_two_bwd(const mb_machine *m, const TwoEnvDesc *d, const TwoEnvTables &t, int n, long long maxItems, const double *logA, const double *logB,
                           double *pool, double *loglike, hipStream_t st) {
  return two_bwd<TwoEnvGeom>(m, d, t, n, maxItems, logA, logB, pool, loglike, st);
}

template <template <bool> class Geom>
static int two_counts(const mb_machine *m, const typename Geom<true>::Desc *d, typename Geom<true>::Tables t, int n, int groupsPerPair, const double *logA,
                      const double *logB, const double *fwdPool, const double *bwdPool, double *counts, hipStream_t st) {
  if (n <= 0 || m->nTrans <= 0) return 0;
  k_profile_two_counts<Geom><<<dim3((unsigned)((long long)n * groupsPerPair)), dim3(256), 0, st>>>(m->dev, d, t, groupsPerPair, logA, logB, fwdPool, bwdPool, m->nTrans, counts,
                                                                                                g_deterministic ? 1 : 0);
  return hip_ok(hipGetLastError(), Geom<true>::ENV ? "k_profile_two_env_counts" : "k_profile_two_counts") ? 0 : 1;
}
int launch_profile_two_counts(const mb_machine *m, const PairProfDesc *d, int n, int groupsPerPair, const double *logA, const double *logB,
                              const double *fwdPool, const double *bwdPool, double *counts, hipStream_t st) {
  return two_counts<TwoGeom>(m, d, {}, n, groupsPerPair, logA, logB, fwdPool, bwdPool, counts, st);
}
int launch_profile_two_counts(const mb_machine *m, const TwoEnvDesc *d, const TwoEnvTables &t, int n, int groupsPerPair, const double *logA, const double *logB,
                              const double *fwdPool, const double *bwdPool, double *counts, hipStream_t st) {
  return two_counts<TwoEnvGeom>(m, d, t, n, groupsPerPair, logA, logB, fwdPool, bwdPool, counts, st);
}

template <template <bool> class Geom>
static int two_rowpost(const mb_machine *m, int axis, const typename Geom<true>::Desc *d, typename Geom<true>::Tables t, int n, int groupsPerPair, int tabMax,
                       const double *logA, const double *logB, const double *fwdPool, const double *bwdPool, double *post, hipStream_t st) {
  if (n <= 0) return 0;
  const dim3 g((unsigned)((long long)n * groupsPerPair)), b(ROWPOST_THREADS);
  const int det = g_deterministic ? 1 : 0;
  if (axis) k_profile_two_rowpost<1, Geom><<<g, b, 0, st>>>(m->dev, d, t, groupsPerPair, logA, logB, fwdPool, bwdPool, post, tabMax, det);
  else k_profile_two_rowpost<0, Geom><<<g, b, 0, st>>>(m->dev, d, t, groupsPerPair, logA, logB, fwdPool, bwdPool, post, tabMax, det);
  return hip_ok(hipGetLastError(), Geom<true>::ENV ? "k_profile_two_env_rowpost" : "k_profile_two_rowpost") ? 0 : 1;
}
int launch_profile_two_rowpost(const mb_machine *m, int axis, const PairProfDesc *d, int n, int groupsPerPair, int tabMax, const double *logA,
                               const double *logB, const double *fwdPool, const double *bwdPool, double *post, hipStream_t st) {
  return two_rowpost<TwoGeom>(m, axis, d, {}, n, groupsPerPair, tabMax, logA, logB, fwdPool, bwdPool, post, st);
}
int launch_profile_two_rowpost(const mb_machine *m, int axis, const TwoEnvDesc *d, const TwoEnvTables &t, int n, int groupsPerPair, int tabMax, const double *logA,
                               const double *logB, const double *fwdPool, const double *bwdPool, double *post, hipStream_t st) {
  return two_rowpost<TwoEnvGeom>(m, axis, d, t, n, groupsPerPair, tabMax, logA, logB, fwdPool, bwdPool, post, st);
}

template <template <bool> class Geom>
static int two_traceback(const mb_machine *m, const typename Geom<true>::Desc *d, typename Geom<true>::Tables t, int n, const double *logA, const double *logB,
                         const double *pool, uint32_t *edges, int32_t *rows, int32_t *inRows, long long *len, hipStream_t st) {
  if (n <= 0) return 0;
  k_profile_two_traceback<Geom><<<(n + 63) / 64, 64, 0, st>>>(m->dev, d, t, n, logA, logB, pool, edges, rows, inRows, len);
  return hip_ok(hipGetLastError(), Geom<true>::ENV ? "k_profile_two_env_traceback" : "k_profile_two_traceback") ? 0 : 1;
}
int launch_profile_two_traceback(const mb_machine *m, const PairProfDesc *d, int n, const double *logA, const double *logB, const double *pool,
                                 uint32_t *edges, int32_t *rows, int32_t *inRows, long long *len, hipStream_t st) {
  return two_traceback<TwoGeom>(m, d, {}, n, logA, logB, pool, edges, rows, inRows, len, st);
}
int launch_profile_two_traceback(const mb_machine *m, const TwoEnvDesc *d, const TwoEnvTables &t, int n, const double *logA, const double *logB, const double *pool,
                                 uint32_t *edges, int32_t *rows, int32_t *inRows, long long *len, hipStream_t st) {
  return two_traceback<TwoEnvGeom>(m, d, t, n, logA, logB, pool, edges, rows, inRows, len, st);
}

template <template <bool> class Geom>
static int two_sample(const mb_machine *m, const typename Geom<true>::Desc *d, typename Geom<true>::Tables t, int n, int nSamples, long long pair0, unsigned long long seed,
                      const double *logA, const double *logB, const double *pool, uint32_t *edges, int32_t *rows, int32_t *inRows, long long *len, double *logq,
                      hipStream_t st) {
  if (n <= 0) return 0;
  const long long nLanes = (long long)n * nSamples;
  k_profile_two_sample<Geom><<<(unsigned)((nLanes + 63) / 64), 64, 0, st>>>(m->dev, d, t, nLanes, nSamples, pair0, seed, logA, logB, pool, edges, rows, inRows, len, logq);
  return hip_ok(hipGetLastError(), Geom<true>::ENV ? "k_profile_two_env_sample" : "k_profile_two_sample") ? 0 : 1;
}
int launch_profile_two_sample(const mb_machine *m, const PairProfDesc *d, int n, int nSamples, long long pair0, unsigned long long seed, const double *logA,
                              const double *logB, const double *pool, uint32_t *edges, int32_t *rows, int32_t *inRows, long long *len, double *logq, hipStream_t st) {
  return two_sample<TwoGeom>(m, d, {}, n, nSamples, pair0, seed, logA, logB, pool, edges, rows, inRows, len, logq, st);
}
int launch_profile_two_sample(const mb_machine *m, const TwoEnvDesc *d, const TwoEnvTables &t, int n, int nSamples, long long pair0, unsigned long long seed,
                              const double *logA, const double *logB, const double *pool, uint32_t *edges, int32_t *rows, int32_t *inRows, long long *len,
                              double *logq, hipStream_t st) {
  return two_sample<TwoEnvGeom>(m, d, t, n, nSamples, pair0, seed, logA, logB, pool, edges, rows, inRows, len, logq, st);
}

}  // namespace mb
