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
#include <algorithm>

#include "mb_device_math.h"
#include "mb_profile_pair.h"

namespace mb {

template <int MODE>
__device__ __forceinline__ double pp_red(double a, double b) { return MODE == MB_VITERBI ? dmax(a, b) : lse2_exact(a, b); }

static constexpr int PP_THREADS = 1024;
static constexpr size_t PP_LDS_MAX = 160 * 1024;
static constexpr int PP_COUNTS_LDS_MAX = 8192;

size_t profile_pair_lds_bytes(int S, long long nIn, long long nRows) {
  const double b = (double)profile_pair_ring(S, nIn, nRows) * sizeof(double);
  return b <= (double)PP_LDS_MAX ? (size_t)b : 0;
}

// Where the layers of cell (i, r) live: the materialised lattice, or the ring (diagonal (i + r) mod 3, the cell by its coordinate on
// the short side of the lattice).
template <bool MAT>
struct PairLattice {
  double *base;
  int S, L, M, byI;
  __device__ __forceinline__ double *at(int i, int r, int layer) const {
    if (MAT) return base + ((((long long)i * (L + 1)) + r) * 2 + layer) * S;
    return base + ((((long long)((i + r) % 3) * M) + (byI ? i : r)) * 2 + layer) * S;
  }
};

// Forward (MODE = MB_FORWARD) or Viterbi (MB_VITERBI) sweep.  MAT: every cell into pool (layout of mb_profile_pair.h), else rolling.
// Viterbi keeps the FIRST maximum: N takes the blank first, then the match edges in `incoming` order, then the output-only edges in
// `incoming` order; W takes N (no move) first, then the input-only edges, then the silent edges, each in `incoming` order -- the
// order k_profile_pair_traceback re-enumerates.
template <int MODE, bool MAT>
__global__ __launch_bounds__(PP_THREADS) void k_profile_pair_fwd(DevMachine m, const PairProfDesc *__restrict__ descs,
                                                                 const int *__restrict__ inTok, const double *__restrict__ logP,
                                                                 double *pool, double *scratch, double *__restrict__ loglike) {
  extern __shared__ double pp_sh[];
  const PairProfDesc pd = descs[blockIdx.x];
  const int S = m.S, K = m.K, C = m.nOut + 1, I = pd.nIn, L = pd.nRows;
  const int *x = inTok + pd.inBase;
  const double *P = logP + pd.rowBase * C;
  const PairLattice<MAT> lat{MAT ? pool + pd.cellBase : (pd.ringBase < 0 ? pp_sh : scratch + pd.ringBase), S, L, min(I, L) + 1, I <= L};
  for (int d = 0; d <= I + L; ++d) {
    const int ilo = max(0, d - L), nCells = min(I, d) - ilo + 1;
    const int nItems = nCells * S;
    for (int it = threadIdx.x; it < nItems; it += blockDim.x) {
      const int c = it / S, q = it - c * S, i = ilo + c, r = d - i;
      const int xRow = i > 0 ? q * K + x[i - 1] * C : 0;     // CSR rows q*K + key(x_i, o), o = 0..nOut: contiguous
      double acc;
      if (r > 0) {
        const double *Pr = P + (long long)(r - 1) * C;
        acc = lat.at(i, r - 1, 0)[q] + Pr[0];
        if (i > 0) {
          const double *Wd = lat.at(i - 1, r - 1, 1);
          const int a1 = m.inOff[xRow + C];
          for (int a = m.inOff[xRow + 1]; a < a1; ++a)
            acc = pp_red<MODE>(acc, (Wd[m.inSrc[a]] + m.inW[a]) + Pr[m.eOutTok[m.inEid[a]]]);
        }
        const double *Wu = lat.at(i, r - 1, 1);
        const int a1 = m.inOff[q * K + C];
        for (int a = m.inOff[q * K + 1]; a < a1; ++a)
          acc = pp_red<MODE>(acc, (Wu[m.inSrc[a]] + m.inW[a]) + Pr[m.eOutTok[m.inEid[a]]]);
      } else {
        acc = (i == 0 && q == 0) ? 0.0 : -INFINITY;
      }
      lat.at(i, r, 0)[q] = acc;
      if (i > 0) {
        const double *Wl = lat.at(i - 1, r, 1);
        const int a1 = m.inOff[xRow + 1];
        for (int a = m.inOff[xRow]; a < a1; ++a) acc = pp_red<MODE>(acc, Wl[m.inSrc[a]] + m.inW[a]);
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
          acc = pp_red<MODE>(acc, Wc[s] + m.inW[a]);
        }
        Wc[q] = acc;
      }
      __syncthreads();
    }
  }
  if (threadIdx.x == 0) loglike[blockIdx.x] = lat.at(I, L, 1)[S - 1];
}

// Materialised Backward sweep, layer 0 = NB ("from the arrived stage"), layer 1 = WB ("from the waiting stage"):
//   WB[i][r][s] = [i = I, r = L, s = S-1]
//                 (+) sum_{t: s->d, in = x_{i+1}, out = o} (w_t + P[r][o]) + NB[i+1][r+1][d]     (i < I, r < L)
//                 (+) sum_{t: s->d, in = eps, out = o}     (w_t + P[r][o]) + NB[i][r+1][d]       (r < L)
//                 (+) sum_{t: s->d, in = x_{i+1}, out = eps} w_t + WB[i+1][r][d]                 (i < I)
//                 (+) sum_{silent t: s->d, s < d}            w_t + WB[i][r][d]
//   NB[i][r][s] = WB[i][r][s] (+) (P[r][0] + NB[i][r+1][s])   (r < L);   loglike = NB[0][0][0]
// Anti-diagonals from I + L down.  A state's WB is final once its backward level has run; the item that finishes it writes its NB.
__global__ __launch_bounds__(PP_THREADS) void k_profile_pair_bwd(DevMachine m, const PairProfDesc *__restrict__ descs,
                                                                 const int *__restrict__ inTok, const double *__restrict__ logP,
                                                                 double *pool, double *__restrict__ loglike) {
  const PairProfDesc pd = descs[blockIdx.x];
  const int S = m.S, K = m.K, C = m.nOut + 1, I = pd.nIn, L = pd.nRows;
  const int *x = inTok + pd.inBase;
  const double *P = logP + pd.rowBase * C;
  const PairLattice<true> lat{pool + pd.cellBase, S, L, 0, 0};
  for (int d = I + L; d >= 0; --d) {
    const int ilo = max(0, d - L), nCells = min(I, d) - ilo + 1;
    const int nItems = nCells * S;
    for (int it = threadIdx.x; it < nItems; it += blockDim.x) {
      const int c = it / S, s = it - c * S, i = ilo + c, r = d - i;
      const int xRow = i < I ? s * K + x[i] * C : 0;
      const double *Pr = P + (long long)r * C;
      double v = (i == I && r == L && s == S - 1) ? 0.0 : -INFINITY;
      if (r < L) {
        if (i < I) {
          const double *Nd = lat.at(i + 1, r + 1, 0);
          const int a1 = m.outOff[xRow + C];
          for (int a = m.outOff[xRow + 1]; a < a1; ++a)
            v = lse2_exact(v, (m.outW[a] + Pr[m.eOutTok[m.outEid[a]]]) + Nd[m.outDst[a]]);
        }
        const double *Nu = lat.at(i, r + 1, 0);
        const int a1 = m.outOff[s * K + C];
        for (int a = m.outOff[s * K + 1]; a < a1; ++a)
          v = lse2_exact(v, (m.outW[a] + Pr[m.eOutTok[m.outEid[a]]]) + Nu[m.outDst[a]]);
      }
      if (i < I) {
        const double *Wl = lat.at(i + 1, r, 1);
        const int a1 = m.outOff[xRow + 1];
        for (int a = m.outOff[xRow]; a < a1; ++a) v = lse2_exact(v, Wl[m.outDst[a]] + m.outW[a]);
      }
      lat.at(i, r, 1)[s] = v;
      lat.at(i, r, 0)[s] = r < L ? lse2_exact(v, Pr[0] + lat.at(i, r + 1, 0)[s]) : v;
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
        lat.at(i, r, 0)[s] = r < L ? lse2_exact(v, P[(long long)r * C] + lat.at(i, r + 1, 0)[s]) : v;
      }
      __syncthreads();
    }
  }
  if (threadIdx.x == 0) loglike[blockIdx.x] = lat.at(0, 0, 0)[0];
}

// Posterior counts.  With both lattices in memory every (cell, edge) term is independent:
//   count[t] += exp(W_F[i][r][s] - LL + term_t), term_t the edge's summand of WB[i][r][s] above,
// so the sweep is a flat grid over (pair, group of the pair, (cell, state)).  Per-workgroup partial counts are kept in LDS when the
// transition table is small and flushed once with atomics; det: both tables hold 64-bit fixed point at 2^-36 (mb_internal.h) --
// integer adds commute, so the counts are the same bits from call to call.  A pair whose likelihood is -inf adds nothing.
__global__ __launch_bounds__(256) void k_profile_pair_counts(DevMachine m, const PairProfDesc *__restrict__ descs, int groupsPerPair,
                                                             const int *__restrict__ inTok, const double *__restrict__ logP,
                                                             const double *__restrict__ fwdPool, const double *__restrict__ bwdPool,
                                                             long long nTrans, double *__restrict__ counts, int det) {
  __shared__ double lcount[PP_COUNTS_LDS_MAX];
  const bool useLds = nTrans <= PP_COUNTS_LDS_MAX;
  if (useLds) {
    for (int e = threadIdx.x; e < nTrans; e += blockDim.x) lcount[e] = 0.0;
    __syncthreads();
  }
  const int k = blockIdx.x / groupsPerPair, group = blockIdx.x % groupsPerPair;
  const PairProfDesc pd = descs[k];
  const int S = m.S, K = m.K, C = m.nOut + 1, I = pd.nIn, L = pd.nRows;
  const int *x = inTok + pd.inBase;
  const double *P = logP + pd.rowBase * C;
  const PairLattice<true> F{const_cast<double *>(fwdPool) + pd.cellBase, S, L, 0, 0}, B{const_cast<double *>(bwdPool) + pd.cellBase, S, L, 0, 0};
  const double LL = F.at(I, L, 1)[S - 1];
  double *tab = useLds ? lcount : counts;
  auto add = [&](uint32_t e, double c) {
    if (c != 0.0) {
      if (det) atomicAdd((unsigned long long *)tab + e, (unsigned long long)fmin(fmax(c * 68719476736.0 + 0.5, 0.0), 4611686018427387904.0));
      else atomicAdd(&tab[e], c);
    }
  };
  if (LL > -INFINITY) {
    const long long nItems = (long long)(I + 1) * (L + 1) * S;
    for (long long idx = (long long)group * blockDim.x + threadIdx.x; idx < nItems; idx += (long long)groupsPerPair * blockDim.x) {
      const long long cell = idx / S;
      const int s = (int)(idx - cell * S), i = (int)(cell / (L + 1)), r = (int)(cell - (long long)i * (L + 1));
      const double f = F.at(i, r, 1)[s] - LL;
      if (!(f > -INFINITY)) continue;
      const int xRow = i < I ? s * K + x[i] * C : 0;
      const double *Pr = P + (long long)r * C;
      if (r < L) {
        if (i < I) {
          const double *Nd = B.at(i + 1, r + 1, 0);
          const int a1 = m.outOff[xRow + C];
          for (int a = m.outOff[xRow + 1]; a < a1; ++a)
            add(m.outEid[a], exp(f + ((m.outW[a] + Pr[m.eOutTok[m.outEid[a]]]) + Nd[m.outDst[a]])));
        }
        const double *Nu = B.at(i, r + 1, 0);
        const int a1 = m.outOff[s * K + C];
        for (int a = m.outOff[s * K + 1]; a < a1; ++a)
          add(m.outEid[a], exp(f + ((m.outW[a] + Pr[m.eOutTok[m.outEid[a]]]) + Nu[m.outDst[a]])));
      }
      if (i < I) {
        const double *Wl = B.at(i + 1, r, 1);
        const int a1 = m.outOff[xRow + 1];
        for (int a = m.outOff[xRow]; a < a1; ++a) add(m.outEid[a], exp(f + (Wl[m.outDst[a]] + m.outW[a])));
      }
      const double *Wc = B.at(i, r, 1);
      const int a1 = m.outOff[s * K + 1];
      for (int a = m.outOff[s * K]; a < a1; ++a) {
        const int t = (int)m.outDst[a];
        if (t <= s) continue;
        add(m.outEid[a], exp(f + (Wc[t] + m.outW[a])));
      }
    }
  }
  if (useLds) {
    __syncthreads();
    for (int e = threadIdx.x; e < nTrans; e += blockDim.x)
      if (det ? ((const unsigned long long *)lcount)[e] != 0ull : lcount[e] != 0.0) {
        if (det) atomicAdd((unsigned long long *)counts + e, ((const unsigned long long *)lcount)[e]);
        else atomicAdd(&counts[e], lcount[e]);
      }
  }
}

// Viterbi traceback over a materialised max lattice, one lane per pair: from W[I][L][S-1] back to N[0][0][0], taking at every cell
// the first candidate (in the fill's order) whose value equals the cell.  Edges go start -> end into the pair's slot
// (profile_pair_path_bound entries) with the row each fired at: an emitting edge the row it consumed, an output-less edge the number
// of rows consumed before it.  len = -1: no finite path, -2: the slot was too small, -3: no candidate matched (a corrupt matrix).
__global__ void k_profile_pair_traceback(DevMachine m, const PairProfDesc *__restrict__ descs, int n, const int *__restrict__ inTok,
                                         const double *__restrict__ logP, const double *__restrict__ pool, uint32_t *edges,
                                         int32_t *rows, long long *len) {
  const int k = blockIdx.x * blockDim.x + threadIdx.x;
  if (k >= n) return;
  const PairProfDesc pd = descs[k];
  const int S = m.S, K = m.K, C = m.nOut + 1, I = pd.nIn, L = pd.nRows;
  const int *x = inTok + pd.inBase;
  const double *P = logP + pd.rowBase * C;
  const PairLattice<true> lat{const_cast<double *>(pool) + pd.cellBase, S, L, 0, 0};
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
      if (i > 0) {
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
      if (lat.at(i, r - 1, 0)[q] + Pr[0] == cur) { --r; continue; }
      int ni = i;
      if (i > 0) {
        const double *Wd = lat.at(i - 1, r - 1, 1);
        a = m.inOff[xRow + 1];
        for (const int a1 = m.inOff[xRow + C]; a < a1; ++a)
          if ((Wd[m.inSrc[a]] + m.inW[a]) + Pr[m.eOutTok[m.inEid[a]]] == cur) { found = (int)m.inSrc[a]; ni = i - 1; break; }
      }
      if (found < 0) {
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
  for (long long u = 0, v = cnt - 1; u < v; ++u, --v) {
    const uint32_t e = pe[u]; pe[u] = pe[v]; pe[v] = e;
    const int32_t w = pr[u]; pr[u] = pr[v]; pr[v] = w;
  }
  len[k] = cnt;
}

static int pp_threads(long long maxItems) { return (int)std::min<long long>(PP_THREADS, std::max<long long>(64, (maxItems + 63) / 64 * 64)); }

int launch_profile_pair_fwd(const mb_machine *m, int mode, bool mat, const PairProfDesc *d, int n, size_t lds, long long maxItems,
                            const int *inTok, const double *logP, double *pool, double *scratch, double *loglike, hipStream_t st) {
  if (n <= 0) return 0;
  if (mat) lds = 0;
  static size_t ldsAllowed = 64 * 1024;      // beyond the default the kernels must be told; asked for once, and only when a ring needs it
  if (lds > ldsAllowed) {
    if (!hip_ok(hipFuncSetAttribute((const void *)&k_profile_pair_fwd<MB_FORWARD, false>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)PP_LDS_MAX),
                "k_profile_pair_fwd: raising the LDS limit") ||
        !hip_ok(hipFuncSetAttribute((const void *)&k_profile_pair_fwd<MB_VITERBI, false>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)PP_LDS_MAX),
                "k_profile_pair_fwd: raising the LDS limit")) return 1;
    ldsAllowed = PP_LDS_MAX;
  }
  const dim3 g(n), b(pp_threads(maxItems));
  if (mode == MB_VITERBI) {
    if (mat) k_profile_pair_fwd<MB_VITERBI, true><<<g, b, 0, st>>>(m->dev, d, inTok, logP, pool, scratch, loglike);
    else k_profile_pair_fwd<MB_VITERBI, false><<<g, b, lds, st>>>(m->dev, d, inTok, logP, pool, scratch, loglike);
  } else {
    if (mat) k_profile_pair_fwd<MB_FORWARD, true><<<g, b, 0, st>>>(m->dev, d, inTok, logP, pool, scratch, loglike);
    else k_profile_pair_fwd<MB_FORWARD, false><<<g, b, lds, st>>>(m->dev, d, inTok, logP, pool, scratch, loglike);
  }
  return hip_ok(hipGetLastError(), "k_profile_pair_fwd") ? 0 : 1;
}

int launch_profile_pair_bwd(const mb_machine *m, const PairProfDesc *d, int n, long long maxItems, const int *inTok, const double *logP,
                            double *pool, double *loglike, hipStream_t st) {
  if (n <= 0) return 0;
  k_profile_pair_bwd<<<dim3(n), dim3(pp_threads(maxItems)), 0, st>>>(m->dev, d, inTok, logP, pool, loglike);
  return hip_ok(hipGetLastError(), "k_profile_pair_bwd") ? 0 : 1;
}

int launch_profile_pair_counts(const mb_machine *m, const PairProfDesc *d, int n, int groupsPerPair, const int *inTok, const double *logP,
                               const double *fwdPool, const double *bwdPool, double *counts, hipStream_t st) {
  if (n <= 0 || m->nTrans <= 0) return 0;
  k_profile_pair_counts<<<dim3((unsigned)((long long)n * groupsPerPair)), dim3(256), 0, st>>>(m->dev, d, groupsPerPair, inTok, logP, fwdPool, bwdPool,
                                                                                               m->nTrans, counts, g_deterministic ? 1 : 0);
  return hip_ok(hipGetLastError(), "k_profile_pair_counts") ? 0 : 1;
}

int launch_profile_pair_traceback(const mb_machine *m, const PairProfDesc *d, int n, const int *inTok, const double *logP,
                                  const double *pool, uint32_t *edges, int32_t *rows, long long *len, hipStream_t st) {
  if (n <= 0) return 0;
  k_profile_pair_traceback<<<(n + 63) / 64, 64, 0, st>>>(m->dev, d, n, inTok, logP, pool, edges, rows, len);
  return hip_ok(hipGetLastError(), "k_profile_pair_traceback") ? 0 : 1;
}

}  // namespace mb
