// mb_profile.hip -- Forward / Backward / Viterbi / posterior counts of a machine with an empty input tape against PROFILE tapes
// (rows of output-symbol log weights plus a blank), the semantics of compose(M, transpose(CSVProfile::machine())) with empty
// tapes (src/csv.cpp:8-18, src/machine.cpp:794-850, 1053-1085), restated in docs/profile_tapes.md:
//
//   N[0][q]   = 0 if q == 0 else -inf
//   W[r][q]   = N[r][q] (+) sum_{silent t: s->q, s < q} W[r][s] + w_t                          (silent levels, r = 0..L)
//   N[r+1][q] = (N[r][q] + P[r][0]) (+) sum_{t: s->q, in = eps, out = o != eps} (W[r][s] + w_t) + P[r][o]
//   loglike   = W[L][S-1]
//
// One workgroup per profile, lanes over states.  Per row: one emission phase (every emitting incoming edge of a destination and
// the blank term) and one barrier, then one barrier per silent level.  The rolling sweeps keep three state vectors (two N rows and
// W) in LDS when they fit (24 S bytes: about 6 800 states in 160 KiB), else in a per-workgroup slice of a global scratch buffer.
// Cells are fp64 and the sums use the exact log-sum-exp (the counts of long profiles need it).  Transitions that read input never
// fire: the input tape is empty.
#include "mb_profile.h"
#include "mb_profile_common.h"

namespace mb {

size_t profile_lds_bytes(int S) {
  const size_t b = (size_t)3 * S * sizeof(double);
  return b <= SWEEP_LDS_MAX ? b : 0;
}

// Forward (MODE = MB_FORWARD) or Viterbi (MB_VITERBI) sweep.  MAT: every cell into pool (layout of mb_profile.h), else rolling.
// Viterbi keeps the FIRST maximum: N takes the blank candidate first, then the emitting edges in `incoming` order; W takes N
// (no move) first, then the silent edges in `incoming` order -- the order k_profile_traceback re-enumerates.
template <int MODE, bool MAT>
__global__ __launch_bounds__(SWEEP_THREADS) void k_profile_fwd(DevMachine m, const ProfDesc *__restrict__ descs,
                                                               const double *__restrict__ logP, double *pool, double *scratch,
                                                               int useLds, double *__restrict__ loglike) {
  extern __shared__ double pf_sh[];
  const ProfDesc pd = descs[blockIdx.x];
  const int S = m.S, K = m.K, C = m.nOut + 1, L = pd.nRows;
  const double *P = logP + pd.rowBase * C;
  double *ring = MAT ? nullptr : (useLds ? pf_sh : scratch + (long long)blockIdx.x * 3 * S);
  double *Wc = nullptr;
  for (int r = 0; r <= L; ++r) {
    double *Nc;
    const double *Np, *Wp;
    if (MAT) { Nc = pool + pd.cellBase + (long long)r * 2 * S; Wc = Nc + S; Np = Nc - 2 * S; Wp = Nc - S; }
    else { Nc = ring + (r & 1) * S; Np = ring + ((r + 1) & 1) * S; Wc = ring + 2 * S; Wp = Wc; }
    if (r == 0) {
      for (int q = threadIdx.x; q < S; q += blockDim.x) Nc[q] = q == 0 ? 0.0 : -INFINITY;
    } else {
      const double *Pr = P + (long long)(r - 1) * C;
      const double blank = Pr[0];
      for (int q = threadIdx.x; q < S; q += blockDim.x) {
        double acc = Np[q] + blank;
        const int a1 = m.inOff[q * K + C];            // CSR rows q*K + key(0, o), o = 1..nOut: contiguous
        for (int a = m.inOff[q * K + 1]; a < a1; ++a)
          acc = red<MODE>(acc, (Wp[m.inSrc[a]] + m.inW[a]) + Pr[m.eOutTok[m.inEid[a]]]);
        Nc[q] = acc;
      }
    }
    __syncthreads();
    for (int lev = 0; lev < m.nLevF; ++lev) {
      const int l0 = m.levFOff[lev], ns = m.levFOff[lev + 1] - l0;
      for (int j = threadIdx.x; j < ns; j += blockDim.x) {
        const int q = m.levFState[l0 + j];
        double acc = Nc[q];
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
  if (threadIdx.x == 0) loglike[blockIdx.x] = Wc[S - 1];
}

// Backward sweep:
//   WB[r][s] = [r == L, s == S-1] (+) sum_{emitting t: s->q} (w_t + P[r][o]) + NB[r+1][q] (r < L) (+) sum_{silent t: s->q} WB[r][q] + w_t
//   NB[r][s] = WB[r][s] (+) (P[r][0] + NB[r+1][s])   (r < L);   loglike = NB[0][0]
// MAT: every cell into pool.  fwdPool != nullptr: posterior counts of the profile into part[blockIdx.x * nTrans + edge]:
//   emitting edge at row r: exp(W_F[r][s] + w_t + P[r][o] + NB[r+1][q] - LL),  silent edge at row r: exp(W_F[r][s] + w_t + WB[r][q] - LL)
// with LL the Forward likelihood.  An edge belongs to one source state and a state to one lane (its place in its level), so each
// accumulator has one writer and sees its rows in a fixed order: the counts are the same bits from run to run.
template <bool MAT>
__global__ __launch_bounds__(SWEEP_THREADS) void k_profile_bwd(DevMachine m, const ProfDesc *__restrict__ descs,
                                                               const double *__restrict__ logP, double *pool,
                                                               const double *__restrict__ fwdPool, double *scratch, int useLds,
                                                               double *__restrict__ loglike, double *part, long long nTrans) {
  extern __shared__ double pf_sh[];
  const ProfDesc pd = descs[blockIdx.x];
  const int S = m.S, K = m.K, C = m.nOut + 1, L = pd.nRows;
  const double *P = logP + pd.rowBase * C;
  double *ring = MAT ? nullptr : (useLds ? pf_sh : scratch + (long long)blockIdx.x * 3 * S);
  const double *F = fwdPool ? fwdPool + pd.cellBase : nullptr;
  const double LL = F ? F[(long long)L * 2 * S + S + S - 1] : -INFINITY;
  const bool counting = F && LL > -INFINITY;
  double *acc = counting ? part + (long long)blockIdx.x * nTrans : nullptr;
  double *Nc = nullptr;
  for (int r = L; r >= 0; --r) {
    double *Wc;
    const double *Nn;
    if (MAT) { Nc = pool + pd.cellBase + (long long)r * 2 * S; Wc = Nc + S; Nn = Nc + 2 * S; }
    else { Nc = ring + (r & 1) * S; Nn = ring + ((r + 1) & 1) * S; Wc = ring + 2 * S; }
    const double *Pr = P + (long long)r * C;
    const double *WF = counting ? F + (long long)r * 2 * S + S : nullptr;
    for (int lev = 0; lev < m.nLevB; ++lev) {
      const int l0 = m.levBOff[lev], ns = m.levBOff[lev + 1] - l0;
      for (int j = threadIdx.x; j < ns; j += blockDim.x) {
        const int s = m.levBState[l0 + j];
        double v = (r == L && s == S - 1) ? 0.0 : -INFINITY;
        const double f = counting ? WF[s] - LL : -INFINITY;
        const bool live = f > -INFINITY;
        if (r < L) {
          const int a1 = m.outOff[s * K + C];
          for (int a = m.outOff[s * K + 1]; a < a1; ++a) {
            const double t = (m.outW[a] + Pr[m.eOutTok[m.outEid[a]]]) + Nn[m.outDst[a]];
            v = lse2_exact(v, t);
            if (live) acc[m.outEid[a]] += exp(f + t);
          }
        }
        const int a1 = m.outOff[s * K + 1];
        for (int a = m.outOff[s * K]; a < a1; ++a) {
          const int d = (int)m.outDst[a];
          if (d <= s) continue;
          const double t = Wc[d] + m.outW[a];
          v = lse2_exact(v, t);
          if (live) acc[m.outEid[a]] += exp(f + t);
        }
        Wc[s] = v;
      }
      __syncthreads();
    }
    for (int s = threadIdx.x; s < S; s += blockDim.x) Nc[s] = r < L ? lse2_exact(Wc[s], Pr[0] + Nn[s]) : Wc[s];
    __syncthreads();
  }
  if (threadIdx.x == 0) loglike[blockIdx.x] = Nc[0];
}

// Viterbi traceback over a materialised max lattice, one lane per profile: from W[L][S-1] back to N[0][0], taking at every cell the
// first candidate (in the fill's order) whose value equals the cell.  Edges and the rows they fired at go start -> end into the
// profile's slot (mb_profile_path_bound entries); len = -1: no finite path, -2: the slot was too small, -3: no candidate matched (a corrupt matrix).
__global__ void k_profile_traceback(DevMachine m, const ProfDesc *__restrict__ descs, int n, const double *__restrict__ logP,
                                    const double *__restrict__ pool, uint32_t *edges, int32_t *rows, long long *len) {
  const int k = blockIdx.x * blockDim.x + threadIdx.x;
  if (k >= n) return;
  const ProfDesc pd = descs[k];
  const int S = m.S, K = m.K, C = m.nOut + 1;
  const double *P = logP + pd.rowBase * C, *cells = pool + pd.cellBase;
  uint32_t *pe = edges + pd.pathBase;
  int32_t *pr = rows + pd.pathBase;
  int r = pd.nRows, q = S - 1, layer = 1;
  const long long cap = pd.nRows + (long long)(pd.nRows + 1) * (m.nLevF - 1);
  long long cnt = 0;
  if (!(cells[((long long)r * 2 + 1) * S + q] > -INFINITY)) { len[k] = -1; return; }
  for (;;) {
    const double *N = cells + (long long)r * 2 * S, *W = N + S;
    if (layer == 1) {
      const double cur = W[q];
      if (N[q] == cur) { layer = 0; continue; }
      int a = m.inOff[q * K], found = -1;
      for (const int a1 = m.inOff[q * K + 1]; a < a1; ++a) {
        const int s = (int)m.inSrc[a];
        if (s < q && W[s] + m.inW[a] == cur) { found = s; break; }
      }
      if (found < 0) { len[k] = -3; return; }
      if (cnt >= cap) { len[k] = -2; return; }
      pe[cnt] = m.inEid[a]; pr[cnt] = r; ++cnt;
      q = found;
    } else {
      if (r == 0) { if (q != 0) { len[k] = -3; return; } break; }
      const double *Np = N - 2 * S, *Wp = N - S, *Pr = P + (long long)(r - 1) * C;
      const double cur = N[q];
      if (Np[q] + Pr[0] == cur) { --r; continue; }
      int a = m.inOff[q * K + 1], found = -1;
      for (const int a1 = m.inOff[q * K + C]; a < a1; ++a) {
        const int s = (int)m.inSrc[a];
        if ((Wp[s] + m.inW[a]) + Pr[m.eOutTok[m.inEid[a]]] == cur) { found = s; break; }
      }
      if (found < 0) { len[k] = -3; return; }
      if (cnt >= cap) { len[k] = -2; return; }
      --r;
      pe[cnt] = m.inEid[a]; pr[cnt] = r; ++cnt;
      q = found; layer = 1;
    }
  }
  for (long long i = 0, j = cnt - 1; i < j; ++i, --j) {
    const uint32_t e = pe[i]; pe[i] = pe[j]; pe[j] = e;
    const int32_t w = pr[i]; pr[i] = pr[j]; pr[j] = w;
  }
  len[k] = cnt;
}

// out[e] = sum over the chunk's profiles, in profile order, of part[k * nTrans + e]
__global__ void k_profile_sum_counts(const double *__restrict__ part, int n, long long nTrans, double *__restrict__ out) {
  const long long e = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (e >= nTrans) return;
  double s = 0.0;
  for (int k = 0; k < n; ++k) s += part[(long long)k * nTrans + e];
  out[e] = s;
}

static void pf_set_lds_attr() {
  static bool done = false;
  if (done) return;
  done = true;
  (void)hipFuncSetAttribute((const void *)&k_profile_fwd<MB_FORWARD, false>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)SWEEP_LDS_MAX);
  (void)hipFuncSetAttribute((const void *)&k_profile_fwd<MB_VITERBI, false>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)SWEEP_LDS_MAX);
  (void)hipFuncSetAttribute((const void *)&k_profile_bwd<false>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)SWEEP_LDS_MAX);
}

int launch_profile_fwd(const mb_machine *m, int mode, bool mat, const ProfDesc *d, int n, const double *logP, double *pool,
                       double *scratch, double *loglike, hipStream_t st) {
  if (n <= 0) return 0;
  pf_set_lds_attr();
  const size_t lds = mat ? 0 : profile_lds_bytes(m->S);
  const int useLds = lds > 0;
  const dim3 g(n), b(sweep_threads(m->S));
  if (mode == MB_VITERBI) {
    if (mat) k_profile_fwd<MB_VITERBI, true><<<g, b, 0, st>>>(m->dev, d, logP, pool, scratch, 0, loglike);
    else k_profile_fwd<MB_VITERBI, false><<<g, b, lds, st>>>(m->dev, d, logP, pool, scratch, useLds, loglike);
  } else {
    if (mat) k_profile_fwd<MB_FORWARD, true><<<g, b, 0, st>>>(m->dev, d, logP, pool, scratch, 0, loglike);
    else k_profile_fwd<MB_FORWARD, false><<<g, b, lds, st>>>(m->dev, d, logP, pool, scratch, useLds, loglike);
  }
  return hip_ok(hipGetLastError(), "k_profile_fwd") ? 0 : 1;
}

int launch_profile_bwd(const mb_machine *m, bool mat, const ProfDesc *d, int n, const double *logP, double *pool,
                       const double *fwdPool, double *scratch, double *loglike, double *part, long long nTrans, hipStream_t st) {
  if (n <= 0) return 0;
  pf_set_lds_attr();
  const size_t lds = mat ? 0 : profile_lds_bytes(m->S);
  const dim3 g(n), b(sweep_threads(m->S));
  if (mat) k_profile_bwd<true><<<g, b, 0, st>>>(m->dev, d, logP, pool, fwdPool, scratch, 0, loglike, part, nTrans);
  else k_profile_bwd<false><<<g, b, lds, st>>>(m->dev, d, logP, pool, fwdPool, scratch, lds > 0, loglike, part, nTrans);
  return hip_ok(hipGetLastError(), "k_profile_bwd") ? 0 : 1;
}

int launch_profile_traceback(const mb_machine *m, const ProfDesc *d, int n, const double *logP, const double *pool,
                             uint32_t *edges, int32_t *rows, long long *len, hipStream_t st) {
  if (n <= 0) return 0;
  k_profile_traceback<<<(n + 63) / 64, 64, 0, st>>>(m->dev, d, n, logP, pool, edges, rows, len);
  return hip_ok(hipGetLastError(), "k_profile_traceback") ? 0 : 1;
}

int launch_profile_sum_counts(const double *part, int n, long long nTrans, double *out, hipStream_t st) {
  if (nTrans <= 0) return 0;
  k_profile_sum_counts<<<(unsigned)((nTrans + 255) / 256), 256, 0, st>>>(part, n, nTrans, out);
  return hip_ok(hipGetLastError(), "k_profile_sum_counts") ? 0 : 1;
}

}  // namespace mb
