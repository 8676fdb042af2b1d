// mb_profile_two_env.h -- the two-profile sweeps of mb_profile_two.h under an ENVELOPE (docs/profile_tapes.md, "Pairs of profiles
// under an envelope"): per output row r = 0..L the half-open interval [inStart[r], inEnd[r]) of input-row positions whose cells
// exist; all three layers of every other cell are -inf.  The orientation, the checks and the diagLo / diagCnt / off tables are those
// of mb_profile_pair_env.h with K for I.  The input-row posteriors walk the envelope by COLUMNS: by monotonicity the cells of input
// row i are the run r = colStart[i] .. colEnd[i] - 1, and colOff[i] counts the cells of the columns before i.
//
// Materialised lattices are COMPACT: cells[((off[r] + i - inStart[r]) * 3 + layer) * S + q], off[r] = the cells of the rows < r.
#pragma once
#include "mb_profile_pair_env.h"
#include "mb_profile_two.h"

namespace mb {

struct TwoEnvDesc : PairEnvDesc {
  long long colBase;           // first of this pair's nIn + 1 entries in colStart / colEnd / colOff
};

struct TwoEnvTables : PairEnvTables {
  const int *colStart, *colEnd;   // [input rows] the output rows of each input row's cells
  const long long *colOff;        // [input rows] cells of the input rows before, per pair from 0
};

MB_LATTICE_FN EnvCells lattice_cells(const TwoEnvDesc &pd, const TwoEnvTables &t) {
  return EnvCells(pd.nIn, pd.nRows, t.envStart + pd.envBase, t.envEnd + pd.envBase, t.envOff + pd.envBase, t.diagLo + pd.diagBase, t.diagCnt + pd.diagBase, pd.nCells, pd.M,
                  t.colStart + pd.colBase, t.colOff + pd.colBase);
}

// the rolling ring: three anti-diagonals of three layers, each of M cells; a cell lives at i mod M
inline long long profile_two_env_ring(int S, long long M) { return 3 * 3 * M * (long long)S; }
// dynamic LDS of the ring when it fits (0: a slice of the global scratch buffer)
size_t profile_two_env_lds_bytes(int S, long long M);

// the launchers of mb_profile_two.h over pairs under an envelope (lds, maxItems: of the envelope rings)
int launch_profile_two_fwd(const mb_machine *m, int mode, bool mat, const TwoEnvDesc *d, const TwoEnvTables &t, int n, size_t lds, long long maxItems,
                           const double *logA, const double *logB, double *pool, double *scratch, double *loglike, hipStream_t st);
int launch_profile_two_bwd(const mb_machine *m, const TwoEnvDesc *d, const TwoEnvTables &t, int n, long long maxItems, const double *logA, const double *logB,
                           double *pool, double *loglike, hipStream_t st);
int launch_profile_two_counts(const mb_machine *m, const TwoEnvDesc *d, const TwoEnvTables &t, int n, int groupsPerPair, const double *logA, const double *logB,
                              const double *fwdPool, const double *bwdPool, double *counts, hipStream_t st);
int launch_profile_two_rowpost(const mb_machine *m, int axis, const TwoEnvDesc *d, const TwoEnvTables &t, int n, int groupsPerPair, int tabMax, const double *logA,
                               const double *logB, const double *fwdPool, const double *bwdPool, double *post, hipStream_t st);
int launch_profile_two_traceback(const mb_machine *m, const TwoEnvDesc *d, const TwoEnvTables &t, int n, const double *logA, const double *logB, const double *pool,
                                 uint32_t *edges, int32_t *rows, int32_t *inRows, long long *len, hipStream_t st);
int launch_profile_two_sample(const mb_machine *m, const TwoEnvDesc *d, const TwoEnvTables &t, int n, int nSamples, long long pair0, unsigned long long seed,
                              const double *logA, const double *logB, const double *pool, uint32_t *edges, int32_t *rows, int32_t *inRows, long long *len,
                              double *logq, hipStream_t st);

}  // namespace mb
