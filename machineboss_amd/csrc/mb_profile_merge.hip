// mb_profile_merge.hip -- Forward / Backward / Viterbi / posterior counts of a machine with an empty input tape against CTC-MERGED
// profile tapes: a column repeated in consecutive rows is one symbol, and only a blank separates two equal symbols.  The semantics of
// compose(M, transpose(CSVProfile::mergingMachine())) with empty tapes (src/csv.cpp:20-46), restated in docs/profile_tapes.md:
//
//   N[0][0][q]   = [q == 0], every other plane -inf
//   W[r][p][q]   = N[r][p][q] (+) sum_{silent t: s->q, s < q} W[r][p][s] + w_t                          (silent levels, per plane)
//   N[r+1][0][q] = (+)_p (N[r][p][q] + P[r][0])                                                         (blank: M does not move)
//   N[r+1][c][q] = (N[r][c][q] + P[r][c]) (+) sum_{t: s->q, in = eps, out = colTok[c]} (X[r][c][s] + w_t) + P[r][c]
//   X[r][c][s]   = (+)_{k != c} W[r][k][s]                                                              (the exclusion vector)
//   loglike      = (+)_p W[L][p][S-1]
//
// Plane 0 = the last row took the blank (or no row yet), plane c = the last row took column c.  One workgroup per profile; the lanes
// are split into groups, one per plane, and the lanes of a group run over the states (of a silent level).  Per row: one emission
// phase and a barrier, one barrier per silent level -- the barriers of the plain sweep, with nCols + 1 times the work between them --
// and one more phase and barrier for X, so that no edge loop runs over planes.  Cells are fp64, sums the exact log-sum-exp.
#include "mb_profile_common.h"
#include "mb_profile_merge.h"

namespace mb {

static size_t pm_fit(long long doubles) {
  const unsigned long long b = (unsigned long long)doubles * sizeof(double);
  return b <= SWEEP_LDS_MAX ? (size_t)b : 0;
}
size_t profile_merge_fwd_lds(int S, int nCols, bool mat) { return pm_fit(mat ? (long long)nCols * S : profile_merge_ring(S, nCols)); }
size_t profile_merge_bwd_lds(int S, int nCols) { return pm_fit(3LL * (nCols + 1) * S); }

// The lanes of a workgroup as plane groups: G = min(planes, lanes) groups of LPP lanes; a lane serves planes p0, p0 + G, ... and,
// within a plane, items ln, ln + LPP, ...  Lanes beyond G * LPP idle (p0 = planes) but keep the barriers.
struct PmLanes { int G, LPP, p0, ln; };
__device__ __forceinline__ PmLanes pm_lanes(int planes) {
  PmLanes l;
  l.G = min(planes, (int)blockDim.x);
  l.LPP = (int)blockDim.x / l.G;
  l.p0 = (int)threadIdx.x / l.LPP;
  l.ln = (int)threadIdx.x - l.p0 * l.LPP;
  if (l.p0 >= l.G) l.p0 = planes;
  return l;
}

// Forward (MODE = MB_FORWARD) or Viterbi (MB_VITERBI) sweep.  MAT: every N and W cell into pool (layout of mb_profile_merge.h) and
// only X in the ring, else rolling.  Viterbi keeps the FIRST maximum: W takes N (no move) first, then the silent edges in `incoming`
// order; N[.][0] the planes ascending; N[.][c] the repeat first, then the emitting edges of colTok[c] in `incoming` order; X and the
// end the planes ascending -- the order k_profile_merge_traceback re-enumerates.
template <int MODE, bool MAT>
__global__ __launch_bounds__(SWEEP_THREADS) void k_profile_merge_fwd(DevMachine m, MergeMap mm, const ProfDesc *__restrict__ descs,
                                                                     const double *__restrict__ logP, double *pool, double *scratch,
                                                                     int useLds, double *__restrict__ loglike) {
  extern __shared__ double pm_sh[];
  const ProfDesc pd = descs[blockIdx.x];
  const int S = m.S, K = m.K, nC = mm.nCols, PL = nC + 1, L = pd.nRows;
  const long long PS = (long long)PL * S;
  const double *P = logP + pd.rowBase * PL;
  double *ring = useLds ? pm_sh : scratch + (long long)blockIdx.x * profile_merge_ring(S, nC);
  double *X = ring, *roll = ring + (long long)nC * S;      // X[(c-1)*S + s]
  const PmLanes ln = pm_lanes(PL);
  double *Wc = nullptr;
  for (int r = 0; r <= L; ++r) {
    double *Nc;
    const double *Np;
    if (MAT) { Nc = pool + pd.cellBase + (long long)r * 2 * PS; Wc = Nc + PS; Np = Nc - 2 * PS; }
    else { Nc = roll + (r & 1) * PS; Np = roll + ((r + 1) & 1) * PS; Wc = roll + 2 * PS; }
    if (r == 0) {
      for (int p = ln.p0; p < PL; p += ln.G)
        for (int q = ln.ln; q < S; q += ln.LPP) Nc[(long long)p * S + q] = (p == 0 && q == 0) ? 0.0 : -INFINITY;
    } else {
      const double *Pr = P + (long long)(r - 1) * PL;
      for (int p = ln.p0; p < PL; p += ln.G) {
        const double w = Pr[p];
        if (p == 0) {
          for (int q = ln.ln; q < S; q += ln.LPP) {
            double acc = Np[q] + w;
            for (int k = 1; k < PL; ++k) acc = red<MODE>(acc, Np[(long long)k * S + q] + w);
            Nc[q] = acc;
          }
        } else {
          const int tok = mm.colTok[p - 1];               // CSR row q*K + key(0, tok): the emitting edges of the column's token
          const double *Xc = X + (long long)(p - 1) * S;
          for (int q = ln.ln; q < S; q += ln.LPP) {
            double acc = Np[(long long)p * S + q] + w;
            const int a1 = m.inOff[q * K + tok + 1];
            for (int a = m.inOff[q * K + tok]; a < a1; ++a) acc = red<MODE>(acc, (Xc[m.inSrc[a]] + m.inW[a]) + w);
            Nc[(long long)p * S + q] = acc;
          }
        }
      }
    }
    __syncthreads();
    for (int lev = 0; lev < m.nLevF; ++lev) {
      const int l0 = m.levFOff[lev], ns = m.levFOff[lev + 1] - l0;
      for (int p = ln.p0; p < PL; p += ln.G) {
        const double *Nq = Nc + (long long)p * S;
        double *Wq = Wc + (long long)p * S;
        for (int j = ln.ln; j < ns; j += ln.LPP) {
          const int q = m.levFState[l0 + j];
          double acc = Nq[q];
          const int a1 = m.inOff[q * K + 1];
          for (int a = m.inOff[q * K]; a < a1; ++a) {
            const int s = (int)m.inSrc[a];
            if (s >= q) continue;                         // as the plain sweep: a silent self-loop never fires
            acc = red<MODE>(acc, Wq[s] + m.inW[a]);
          }
          Wq[q] = acc;
        }
      }
      __syncthreads();
    }
    if (r < L) {
      for (int c = ln.p0 + 1; c < PL; c += ln.G) {
        double *Xc = X + (long long)(c - 1) * S;
        for (int s = ln.ln; s < S; s += ln.LPP) {
          double acc = Wc[s];                             // plane 0 is never the excluded one
          for (int k = 1; k < PL; ++k)
            if (k != c) acc = red<MODE>(acc, Wc[(long long)k * S + s]);
          Xc[s] = acc;
        }
      }
      __syncthreads();
    }
  }
  if (threadIdx.x == 0) {
    double acc = Wc[S - 1];
    for (int p = 1; p < PL; ++p) acc = red<MODE>(acc, Wc[(long long)p * S + S - 1]);
    loglike[blockIdx.x] = acc;
  }
}

// Backward sweep:
//   WB[r][k][s] = [r == L, s == S-1] (+) sum_{c != k} sum_{t: s->q, out = colTok[c]} (w_t + P[r][c]) + NB[r+1][c][q] (r < L)
//                 (+) sum_{silent t: s->q} WB[r][k][q] + w_t
//   NB[r][k][s] = WB[r][k][s] (+) (P[r][0] + NB[r+1][0][s]) (+) [k >= 1] (P[r][k] + NB[r+1][k][s])   (r < L);   loglike = NB[0][0][0]
// MAT: every cell into pool.  fwdPool != nullptr: posterior counts into part[(blockIdx.x * (nCols+1) + k) * nTrans + edge], the
// posteriors of the terms above with W_F[r][k][s] - LL in front.  An accumulator belongs to one plane and one source state, hence to
// one lane, which sees its rows and columns in a fixed order: the counts are the same bits from run to run.
template <bool MAT>
__global__ __launch_bounds__(SWEEP_THREADS) void k_profile_merge_bwd(DevMachine m, MergeMap mm, const ProfDesc *__restrict__ descs,
                                                                     const double *__restrict__ logP, double *pool,
                                                                     const double *__restrict__ fwdPool, double *scratch, int useLds,
                                                                     double *__restrict__ loglike, double *part, long long nTrans) {
  extern __shared__ double pm_sh[];
  const ProfDesc pd = descs[blockIdx.x];
  const int S = m.S, K = m.K, nC = mm.nCols, PL = nC + 1, L = pd.nRows;
  const long long PS = (long long)PL * S;
  const double *P = logP + pd.rowBase * PL;
  double *ring = MAT ? nullptr : (useLds ? pm_sh : scratch + (long long)blockIdx.x * profile_merge_ring(S, nC));
  const double *F = fwdPool ? fwdPool + pd.cellBase : nullptr;
  double LL = -INFINITY;
  if (F) {
    const double *WL = F + ((long long)L * 2 + 1) * PS;
    LL = WL[S - 1];
    for (int p = 1; p < PL; ++p) LL = lse2_exact(LL, WL[(long long)p * S + S - 1]);
  }
  const bool counting = F && LL > -INFINITY;
  const PmLanes ln = pm_lanes(PL);
  double *Nc = nullptr;
  for (int r = L; r >= 0; --r) {
    double *Wc;
    const double *Nn;
    if (MAT) { Nc = pool + pd.cellBase + (long long)r * 2 * PS; Wc = Nc + PS; Nn = Nc + 2 * PS; }
    else { Nc = ring + (r & 1) * PS; Nn = ring + ((r + 1) & 1) * PS; Wc = ring + 2 * PS; }
    const double *Pr = P + (long long)r * PL;
    const double *WF = counting ? F + ((long long)r * 2 + 1) * PS : nullptr;
    for (int lev = 0; lev < m.nLevB; ++lev) {
      const int l0 = m.levBOff[lev], ns = m.levBOff[lev + 1] - l0;
      for (int k = ln.p0; k < PL; k += ln.G) {
        double *Wk = Wc + (long long)k * S;
        double *acc = counting ? part + ((long long)blockIdx.x * PL + k) * nTrans : nullptr;
        for (int j = ln.ln; j < ns; j += ln.LPP) {
          const int s = m.levBState[l0 + j];
          double v = (r == L && s == S - 1) ? 0.0 : -INFINITY;
          const double f = counting ? WF[(long long)k * S + s] - LL : -INFINITY;
          const bool live = f > -INFINITY;
          if (r < L) {
            for (int c = 1; c < PL; ++c) {
              if (c == k) continue;
              const int tok = mm.colTok[c - 1];
              const double pc = Pr[c];
              const double *Nq = Nn + (long long)c * S;
              const int a1 = m.outOff[s * K + tok + 1];
              for (int a = m.outOff[s * K + tok]; a < a1; ++a) {
                const double t = (m.outW[a] + pc) + Nq[m.outDst[a]];
                v = lse2_exact(v, t);
                if (live) acc[m.outEid[a]] += exp(f + t);
              }
            }
          }
          const int a1 = m.outOff[s * K + 1];
          for (int a = m.outOff[s * K]; a < a1; ++a) {
            const int d = (int)m.outDst[a];
            if (d <= s) continue;
            const double t = Wk[d] + m.outW[a];
            v = lse2_exact(v, t);
            if (live) acc[m.outEid[a]] += exp(f + t);
          }
          Wk[s] = v;
        }
      }
      __syncthreads();
    }
    for (int k = ln.p0; k < PL; k += ln.G)
      for (int s = ln.ln; s < S; s += ln.LPP) {
        double v = Wc[(long long)k * S + s];
        if (r < L) {
          v = lse2_exact(v, Pr[0] + Nn[s]);
          if (k) v = lse2_exact(v, Pr[k] + Nn[(long long)k * S + s]);
        }
        Nc[(long long)k * S + s] = v;
      }
    __syncthreads();
  }
  if (threadIdx.x == 0) loglike[blockIdx.x] = Nc[0];
}

// Viterbi traceback over a materialised max lattice, one lane per profile: from the first plane that attains the score at
// W[L][.][S-1] back to N[0][0][0], taking at every cell the first candidate (in the fill's order) whose value equals the cell; an
// emitting edge comes from the lowest plane k != c whose W equals the edge's X.  Blank and repeat rows are not edges.  len as
// k_profile_traceback: -1 no finite path, -2 the slot was too small, -3 no candidate matched (a corrupt matrix).
__global__ void k_profile_merge_traceback(DevMachine m, MergeMap mm, const ProfDesc *__restrict__ descs, int n,
                                          const double *__restrict__ logP, const double *__restrict__ pool, uint32_t *edges,
                                          int32_t *rows, long long *len) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const ProfDesc pd = descs[i];
  const int S = m.S, K = m.K, nC = mm.nCols, PL = nC + 1;
  const long long PS = (long long)PL * S;
  const double *P = logP + pd.rowBase * PL, *cells = pool + pd.cellBase;
  uint32_t *pe = edges + pd.pathBase;
  int32_t *pr = rows + pd.pathBase;
  int r = pd.nRows, q = S - 1, layer = 1, p = 0;
  const long long cap = pd.nRows + (long long)(pd.nRows + 1) * (m.nLevF - 1);
  long long cnt = 0;
  {
    const double *WL = cells + ((long long)r * 2 + 1) * PS;
    double best = WL[q];
    for (int k = 1; k < PL; ++k)
      if (best < WL[(long long)k * S + q]) { best = WL[(long long)k * S + q]; p = k; }
    if (!(best > -INFINITY)) { len[i] = -1; return; }
  }
  for (;;) {
    const double *N = cells + (long long)r * 2 * PS, *W = N + PS;
    if (layer == 1) {
      const double *Wp = W + (long long)p * S;
      const double cur = Wp[q];
      if (N[(long long)p * S + q] == cur) { layer = 0; continue; }
      int a = m.inOff[q * K], found = -1;
      for (const int a1 = m.inOff[q * K + 1]; a < a1; ++a) {
        const int s = (int)m.inSrc[a];
        if (s < q && Wp[s] + m.inW[a] == cur) { found = s; break; }
      }
      if (found < 0) { len[i] = -3; return; }
      if (cnt >= cap) { len[i] = -2; return; }
      pe[cnt] = m.inEid[a]; pr[cnt] = r; ++cnt;
      q = found;
    } else {
      if (r == 0) { if (q != 0 || p != 0) { len[i] = -3; return; } break; }
      const double *Np = N - 2 * PS, *Wv = N - PS, *Pr = P + (long long)(r - 1) * PL;
      const double cur = N[(long long)p * S + q], w = Pr[p];
      if (p == 0) {
        int k = 0;
        while (k < PL && !(Np[(long long)k * S + q] + w == cur)) ++k;
        if (k == PL) { len[i] = -3; return; }
        p = k; --r;
        continue;
      }
      if (Np[(long long)p * S + q] + w == cur) { --r; continue; }
      const int tok = mm.colTok[p - 1];
      int a = m.inOff[q * K + tok], found = -1, from = -1;
      for (const int a1 = m.inOff[q * K + tok + 1]; a < a1; ++a) {
        const int s = (int)m.inSrc[a];
        double x = Wv[s];
        int kx = 0;
        for (int k = 1; k < PL; ++k)
          if (k != p && x < Wv[(long long)k * S + s]) { x = Wv[(long long)k * S + s]; kx = k; }
        if ((x + m.inW[a]) + w == cur) { found = s; from = kx; break; }
      }
      if (found < 0) { len[i] = -3; return; }
      if (cnt >= cap) { len[i] = -2; return; }
      --r;
      pe[cnt] = m.inEid[a]; pr[cnt] = r; ++cnt;
      q = found; p = from; layer = 1;
    }
  }
  for (long long a = 0, b = cnt - 1; a < b; ++a, --b) {
    const uint32_t e = pe[a]; pe[a] = pe[b]; pe[b] = e;
    const int32_t w = pr[a]; pr[a] = pr[b]; pr[b] = w;
  }
  len[i] = cnt;
}

static void pm_set_lds_attr() {
  static bool done = false;
  if (done) return;
  done = true;
  (void)hipFuncSetAttribute((const void *)&k_profile_merge_fwd<MB_FORWARD, false>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)SWEEP_LDS_MAX);
  (void)hipFuncSetAttribute((const void *)&k_profile_merge_fwd<MB_VITERBI, false>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)SWEEP_LDS_MAX);
  (void)hipFuncSetAttribute((const void *)&k_profile_merge_fwd<MB_FORWARD, true>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)SWEEP_LDS_MAX);
  (void)hipFuncSetAttribute((const void *)&k_profile_merge_fwd<MB_VITERBI, true>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)SWEEP_LDS_MAX);
  (void)hipFuncSetAttribute((const void *)&k_profile_merge_bwd<false>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)SWEEP_LDS_MAX);
}

// one lane per (plane, state) pair up to the workgroup's 1 024
static int pm_threads(int S, int nCols) { return sweep_threads((long long)(nCols + 1) * S); }

int launch_profile_merge_fwd(const mb_machine *m, MergeMap mm, int mode, bool mat, const ProfDesc *d, int n, const double *logP,
                             double *pool, double *scratch, double *loglike, hipStream_t st) {
  if (n <= 0) return 0;
  pm_set_lds_attr();
  const size_t lds = profile_merge_fwd_lds(m->S, mm.nCols, mat);
  const int useLds = lds > 0;
  const dim3 g(n), b(pm_threads(m->S, mm.nCols));
  if (mode == MB_VITERBI) {
    if (mat) k_profile_merge_fwd<MB_VITERBI, true><<<g, b, lds, st>>>(m->dev, mm, d, logP, pool, scratch, useLds, loglike);
    else k_profile_merge_fwd<MB_VITERBI, false><<<g, b, lds, st>>>(m->dev, mm, d, logP, pool, scratch, useLds, loglike);
  } else {
    if (mat) k_profile_merge_fwd<MB_FORWARD, true><<<g, b, lds, st>>>(m->dev, mm, d, logP, pool, scratch, useLds, loglike);
    else k_profile_merge_fwd<MB_FORWARD, false><<<g, b, lds, st>>>(m->dev, mm, d, logP, pool, scratch, useLds, loglike);
  }
  return hip_ok(hipGetLastError(), "k_profile_merge_fwd") ? 0 : 1;
}

int launch_profile_merge_bwd(const mb_machine *m, MergeMap mm, bool mat, const ProfDesc *d, int n, const double *logP, double *pool,
                             const double *fwdPool, double *scratch, double *loglike, double *part, long long nTrans, hipStream_t st) {
  if (n <= 0) return 0;
  pm_set_lds_attr();
  const size_t lds = mat ? 0 : profile_merge_bwd_lds(m->S, mm.nCols);
  const dim3 g(n), b(pm_threads(m->S, mm.nCols));
  if (mat) k_profile_merge_bwd<true><<<g, b, 0, st>>>(m->dev, mm, d, logP, pool, fwdPool, scratch, 0, loglike, part, nTrans);
  else k_profile_merge_bwd<false><<<g, b, lds, st>>>(m->dev, mm, d, logP, pool, fwdPool, scratch, lds > 0, loglike, part, nTrans);
  return hip_ok(hipGetLastError(), "k_profile_merge_bwd") ? 0 : 1;
}

int launch_profile_merge_traceback(const mb_machine *m, MergeMap mm, const ProfDesc *d, int n, const double *logP, const double *pool,
                                   uint32_t *edges, int32_t *rows, long long *len, hipStream_t st) {
  if (n <= 0) return 0;
  k_profile_merge_traceback<<<(n + 63) / 64, 64, 0, st>>>(m->dev, mm, d, n, logP, pool, edges, rows, len);
  return hip_ok(hipGetLastError(), "k_profile_merge_traceback") ? 0 : 1;
}

}  // namespace mb
