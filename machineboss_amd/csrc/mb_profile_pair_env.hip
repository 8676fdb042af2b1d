// mb_profile_pair_env.hip -- the sweeps of mb_profile_pair.hip restricted to an envelope (docs/profile_tapes.md, "Pairs under an
// envelope").  The recurrence is unchanged; both layers of a cell outside the envelope are -inf, so a read of a neighbour outside
// yields -inf without touching memory and the sweeps visit the envelope cells alone.
//
// One workgroup per pair along the anti-diagonals, as the full sweeps.  The envelope bounds never decrease from row to row, so the
// cells of diagonal d are the run i = diagLo[d] .. diagLo[d] + diagCnt[d] - 1 (the host uploads both); the items of a diagonal are
// (envelope cell, state).  The rolling ring holds three diagonals of both layers with M cells each, M the largest diagCnt of the
// pair, and a cell lives at i mod M: the cells of a diagonal have consecutive i and number at most M, so no two share a slot.  The
// ring is in LDS when 3 * 2 * M * S doubles fit 160 KiB, else in the pair's slice of the global scratch buffer.
#include <algorithm>

#include "mb_device_math.h"
#include "mb_profile_pair_env.h"

namespace mb {

template <int MODE>
__device__ __forceinline__ double ppe_red(double a, double b) { return MODE == MB_VITERBI ? dmax(a, b) : lse2_exact(a, b); }

static constexpr int PPE_THREADS = 1024;
static constexpr size_t PPE_LDS_MAX = 160 * 1024;
static constexpr int PPE_COUNTS_LDS_MAX = 8192;

size_t profile_pair_env_lds_bytes(int S, long long M) {
  const double b = (double)profile_pair_env_ring(S, M) * sizeof(double);
  return b <= (double)PPE_LDS_MAX ? (size_t)b : 0;
}

// Where the layers of an envelope cell live: the compact lattice, or the ring (diagonal (i + r) mod 3, the cell at i mod M).
template <bool MAT>
struct EnvLattice {
  double *base;
  const int *st, *en;         // the pair's envelope rows
  const long long *off;       // compact index of the first cell of each row
  int S, L, M;
  // r in -1..L+1, i in -1..I+1
  __device__ __forceinline__ bool inside(int i, int r) const { return r >= 0 && r <= L && i >= st[r] && i < en[r]; }
  __device__ __forceinline__ double *at(int i, int r, int layer) const {
    if (MAT) return base + ((off[r] + (i - st[r])) * 2 + layer) * S;
    return base + ((((long long)((i + r) % 3) * M) + (i % M)) * 2 + layer) * S;
  }
};

// Forward (MODE = MB_FORWARD) or Viterbi (MB_VITERBI) sweep over the envelope.  MAT: every envelope cell into the compact lattice,
// else rolling.  The candidates and their order are those of k_profile_pair_fwd; one whose source cell lies outside the envelope
// is -inf and is not read.
template <int MODE, bool MAT>
__global__ __launch_bounds__(PPE_THREADS) void k_profile_pair_env_fwd(DevMachine m, const PairEnvDesc *__restrict__ descs, PairEnvTables t,
                                                                      const int *__restrict__ inTok, const double *__restrict__ logP,
                                                                      double *pool, double *scratch, double *__restrict__ loglike) {
  extern __shared__ double ppe_sh[];
  const PairEnvDesc pd = descs[blockIdx.x];
  const int S = m.S, K = m.K, C = m.nOut + 1, I = pd.nIn, L = pd.nRows;
  const int *x = inTok + pd.inBase;
  const double *P = logP + pd.rowBase * C;
  const int *dLo = t.diagLo + pd.diagBase, *dCnt = t.diagCnt + pd.diagBase;
  const EnvLattice<MAT> lat{MAT ? pool + pd.cellBase : (pd.ringBase < 0 ? ppe_sh : scratch + pd.ringBase),
                            t.envStart + pd.envBase, t.envEnd + pd.envBase, t.envOff + pd.envBase, S, L, pd.M};
  for (int d = 0; d <= I + L; ++d) {
    const int ilo = dLo[d], nCells = dCnt[d];
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
            acc = ppe_red<MODE>(acc, (Wd[m.inSrc[a]] + m.inW[a]) + Pr[m.eOutTok[m.inEid[a]]]);
        }
        if (up) {
          const double *Wu = lat.at(i, r - 1, 1);
          const int a1 = m.inOff[q * K + C];
          for (int a = m.inOff[q * K + 1]; a < a1; ++a)
            acc = ppe_red<MODE>(acc, (Wu[m.inSrc[a]] + m.inW[a]) + Pr[m.eOutTok[m.inEid[a]]]);
        }
      } else {
        acc = (i == 0 && q == 0) ? 0.0 : -INFINITY;
      }
      lat.at(i, r, 0)[q] = acc;
      if (i > 0 && lat.inside(i - 1, r)) {
        const double *Wl = lat.at(i - 1, r, 1);
        const int a1 = m.inOff[xRow + 1];
        for (int a = m.inOff[xRow]; a < a1; ++a) acc = ppe_red<MODE>(acc, Wl[m.inSrc[a]] + m.inW[a]);
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
          acc = ppe_red<MODE>(acc, Wc[s] + m.inW[a]);
        }
        Wc[q] = acc;
      }
      __syncthreads();
    }
  }
  if (threadIdx.x == 0) loglike[blockIdx.x] = lat.at(I, L, 1)[S - 1];      // (I, L) is inside a connected envelope
}

// Materialised Backward sweep over the envelope into a compact lattice, layer 0 = NB, layer 1 = WB (k_profile_pair_bwd); a
// successor cell outside the envelope contributes nothing.
__global__ __launch_bounds__(PPE_THREADS) void k_profile_pair_env_bwd(DevMachine m, const PairEnvDesc *__restrict__ descs, PairEnvTables t,
                                                                      const int *__restrict__ inTok, const double *__restrict__ logP,
                                                                      double *pool, double *__restrict__ loglike) {
  const PairEnvDesc pd = descs[blockIdx.x];
  const int S = m.S, K = m.K, C = m.nOut + 1, I = pd.nIn, L = pd.nRows;
  const int *x = inTok + pd.inBase;
  const double *P = logP + pd.rowBase * C;
  const int *dLo = t.diagLo + pd.diagBase, *dCnt = t.diagCnt + pd.diagBase;
  const EnvLattice<true> lat{pool + pd.cellBase, t.envStart + pd.envBase, t.envEnd + pd.envBase, t.envOff + pd.envBase, S, L, 0};
  for (int d = I + L; d >= 0; --d) {
    const int ilo = dLo[d], nCells = dCnt[d];
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
          const int u = (int)m.outDst[a];
          if (u <= s) continue;
          v = lse2_exact(v, Wc[u] + m.outW[a]);
        }
        Wc[s] = v;
        lat.at(i, r, 0)[s] = (r < L && lat.inside(i, r + 1)) ? lse2_exact(v, P[(long long)r * C] + lat.at(i, r + 1, 0)[s]) : v;
      }
      __syncthreads();
    }
  }
  if (threadIdx.x == 0) loglike[blockIdx.x] = lat.at(0, 0, 0)[0];          // (0, 0) is inside a connected envelope
}

// Posterior counts over the compact lattices: the scheme of k_profile_pair_counts (flat grid over (pair, group, (cell, state)),
// per-workgroup LDS accumulators up to 8 192 transitions, 64-bit fixed point at 2^-36 under det).  The row of a compact cell is
// found by bisection in the pair's row offsets.
__global__ __launch_bounds__(256) void k_profile_pair_env_counts(DevMachine m, const PairEnvDesc *__restrict__ descs, PairEnvTables t,
                                                                 int groupsPerPair, const int *__restrict__ inTok,
                                                                 const double *__restrict__ logP, const double *__restrict__ fwdPool,
                                                                 const double *__restrict__ bwdPool, long long nTrans,
                                                                 double *__restrict__ counts, int det) {
  __shared__ double lcount[PPE_COUNTS_LDS_MAX];
  const bool useLds = nTrans <= PPE_COUNTS_LDS_MAX;
  if (useLds) {
    for (int e = threadIdx.x; e < nTrans; e += blockDim.x) lcount[e] = 0.0;
    __syncthreads();
  }
  const int k = blockIdx.x / groupsPerPair, group = blockIdx.x % groupsPerPair;
  const PairEnvDesc pd = descs[k];
  const int S = m.S, K = m.K, C = m.nOut + 1, I = pd.nIn, L = pd.nRows;
  const int *x = inTok + pd.inBase;
  const double *P = logP + pd.rowBase * C;
  const int *st = t.envStart + pd.envBase, *en = t.envEnd + pd.envBase;
  const long long *off = t.envOff + pd.envBase;
  const EnvLattice<true> F{const_cast<double *>(fwdPool) + pd.cellBase, st, en, off, S, L, 0}, B{const_cast<double *>(bwdPool) + pd.cellBase, st, en, off, S, L, 0};
  const double LL = F.at(I, L, 1)[S - 1];
  double *tab = useLds ? lcount : counts;
  auto add = [&](uint32_t e, double c) {
    if (c != 0.0) {
      if (det) atomicAdd((unsigned long long *)tab + e, (unsigned long long)fmin(fmax(c * 68719476736.0 + 0.5, 0.0), 4611686018427387904.0));
      else atomicAdd(&tab[e], c);
    }
  };
  if (LL > -INFINITY) {
    const long long nItems = pd.nCells * S;
    for (long long idx = (long long)group * blockDim.x + threadIdx.x; idx < nItems; idx += (long long)groupsPerPair * blockDim.x) {
      const long long cell = idx / S;
      const int s = (int)(idx - cell * S);
      int lo = 0, hi = L;                      // the last row whose offset is <= cell: rows behind it start past the cell
      while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        if (off[mid] <= cell) lo = mid; else hi = mid - 1;
      }
      const int r = lo, i = st[r] + (int)(cell - off[r]);
      const double f = F.at(i, r, 1)[s] - LL;
      if (!(f > -INFINITY)) continue;
      const int xRow = i < I ? s * K + x[i] * C : 0;
      const double *Pr = P + (long long)r * C;
      if (r < L) {
        if (i < I && B.inside(i + 1, r + 1)) {
          const double *Nd = B.at(i + 1, r + 1, 0);
          const int a1 = m.outOff[xRow + C];
          for (int a = m.outOff[xRow + 1]; a < a1; ++a)
            add(m.outEid[a], exp(f + ((m.outW[a] + Pr[m.eOutTok[m.outEid[a]]]) + Nd[m.outDst[a]])));
        }
        if (B.inside(i, r + 1)) {
          const double *Nu = B.at(i, r + 1, 0);
          const int a1 = m.outOff[s * K + C];
          for (int a = m.outOff[s * K + 1]; a < a1; ++a)
            add(m.outEid[a], exp(f + ((m.outW[a] + Pr[m.eOutTok[m.outEid[a]]]) + Nu[m.outDst[a]])));
        }
      }
      if (i < I && B.inside(i + 1, r)) {
        const double *Wl = B.at(i + 1, r, 1);
        const int a1 = m.outOff[xRow + 1];
        for (int a = m.outOff[xRow]; a < a1; ++a) add(m.outEid[a], exp(f + (Wl[m.outDst[a]] + m.outW[a])));
      }
      const double *Wc = B.at(i, r, 1);
      const int a1 = m.outOff[s * K + 1];
      for (int a = m.outOff[s * K]; a < a1; ++a) {
        const int u = (int)m.outDst[a];
        if (u <= s) continue;
        add(m.outEid[a], exp(f + (Wc[u] + m.outW[a])));
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

// Viterbi traceback over a compact max lattice, one lane per pair: k_profile_pair_traceback with the candidates whose source cell
// lies outside the envelope left out (they are -inf and the cells on the path are finite).  Same slots, same lengths, same codes.
__global__ void k_profile_pair_env_traceback(DevMachine m, const PairEnvDesc *__restrict__ descs, PairEnvTables t, int n,
                                             const int *__restrict__ inTok, const double *__restrict__ logP,
                                             const double *__restrict__ pool, uint32_t *edges, int32_t *rows, long long *len) {
  const int k = blockIdx.x * blockDim.x + threadIdx.x;
  if (k >= n) return;
  const PairEnvDesc pd = descs[k];
  const int S = m.S, K = m.K, C = m.nOut + 1, I = pd.nIn, L = pd.nRows;
  const int *x = inTok + pd.inBase;
  const double *P = logP + pd.rowBase * C;
  const EnvLattice<true> lat{const_cast<double *>(pool) + pd.cellBase, t.envStart + pd.envBase, t.envEnd + pd.envBase, t.envOff + pd.envBase, S, L, 0};
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
  for (long long u = 0, v = cnt - 1; u < v; ++u, --v) {
    const uint32_t e = pe[u]; pe[u] = pe[v]; pe[v] = e;
    const int32_t w = pr[u]; pr[u] = pr[v]; pr[v] = w;
  }
  len[k] = cnt;
}

static int ppe_threads(long long maxItems) { return (int)std::min<long long>(PPE_THREADS, std::max<long long>(64, (maxItems + 63) / 64 * 64)); }

int launch_profile_pair_env_fwd(const mb_machine *m, int mode, bool mat, const PairEnvDesc *d, PairEnvTables t, int n, size_t lds,
                                long long maxItems, const int *inTok, const double *logP, double *pool, double *scratch, double *loglike,
                                hipStream_t st) {
  if (n <= 0) return 0;
  if (mat) lds = 0;
  static size_t ldsAllowed = 64 * 1024;      // beyond the default the kernels must be told; asked for once, and only when a ring needs it
  if (lds > ldsAllowed) {
    if (!hip_ok(hipFuncSetAttribute((const void *)&k_profile_pair_env_fwd<MB_FORWARD, false>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)PPE_LDS_MAX),
                "k_profile_pair_env_fwd: raising the LDS limit") ||
        !hip_ok(hipFuncSetAttribute((const void *)&k_profile_pair_env_fwd<MB_VITERBI, false>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)PPE_LDS_MAX),
                "k_profile_pair_env_fwd: raising the LDS limit")) return 1;
    ldsAllowed = PPE_LDS_MAX;
  }
  const dim3 g(n), b(ppe_threads(maxItems));
  if (mode == MB_VITERBI) {
    if (mat) k_profile_pair_env_fwd<MB_VITERBI, true><<<g, b, 0, st>>>(m->dev, d, t, inTok, logP, pool, scratch, loglike);
    else k_profile_pair_env_fwd<MB_VITERBI, false><<<g, b, lds, st>>>(m->dev, d, t, inTok, logP, pool, scratch, loglike);
  } else {
    if (mat) k_profile_pair_env_fwd<MB_FORWARD, true><<<g, b, 0, st>>>(m->dev, d, t, inTok, logP, pool, scratch, loglike);
    else k_profile_pair_env_fwd<MB_FORWARD, false><<<g, b, lds, st>>>(m->dev, d, t, inTok, logP, pool, scratch, loglike);
  }
  return hip_ok(hipGetLastError(), "k_profile_pair_env_fwd") ? 0 : 1;
}

int launch_profile_pair_env_bwd(const mb_machine *m, const PairEnvDesc *d, PairEnvTables t, int n, long long maxItems, const int *inTok,
                                const double *logP, double *pool, double *loglike, hipStream_t st) {
  if (n <= 0) return 0;
  k_profile_pair_env_bwd<<<dim3(n), dim3(ppe_threads(maxItems)), 0, st>>>(m->dev, d, t, inTok, logP, pool, loglike);
  return hip_ok(hipGetLastError(), "k_profile_pair_env_bwd") ? 0 : 1;
}

int launch_profile_pair_env_counts(const mb_machine *m, const PairEnvDesc *d, PairEnvTables t, int n, int groupsPerPair, const int *inTok,
                                   const double *logP, const double *fwdPool, const double *bwdPool, double *counts, hipStream_t st) {
  if (n <= 0 || m->nTrans <= 0) return 0;
  k_profile_pair_env_counts<<<dim3((unsigned)((long long)n * groupsPerPair)), dim3(256), 0, st>>>(m->dev, d, t, groupsPerPair, inTok, logP, fwdPool,
                                                                                                   bwdPool, m->nTrans, counts, g_deterministic ? 1 : 0);
  return hip_ok(hipGetLastError(), "k_profile_pair_env_counts") ? 0 : 1;
}

int launch_profile_pair_env_traceback(const mb_machine *m, const PairEnvDesc *d, PairEnvTables t, int n, const int *inTok,
                                      const double *logP, const double *pool, uint32_t *edges, int32_t *rows, long long *len, hipStream_t st) {
  if (n <= 0) return 0;
  k_profile_pair_env_traceback<<<(n + 63) / 64, 64, 0, st>>>(m->dev, d, t, n, inTok, logP, pool, edges, rows, len);
  return hip_ok(hipGetLastError(), "k_profile_pair_env_traceback") ? 0 : 1;
}

}  // namespace mb
