// mb_profile_pair_env.h -- the two-tape profile sweeps of mb_profile_pair.h under an ENVELOPE (docs/profile_tapes.md, "Pairs under
// an envelope"): per row r = 0..L the half-open interval [inStart[r], inEnd[r]) of input positions whose cells exist; both layers of
// every other cell are -inf.  inStart and inEnd never decrease from one row to the next, so the envelope cells of an anti-diagonal
// are a run of consecutive i.
//
// Materialised lattices are COMPACT: cells[((off[r] + i - inStart[r]) * 2 + layer) * S + q], off[r] = the cells of the rows < r.
// The pairs against CTC-merged profiles take the same envelopes, descriptors and tables (mb_profile_pair_merge.h), with nCols + 1
// planes in every cell.
#pragma once
#include "mb_profile_pair.h"

namespace mb {

// a pair's descriptor and what its envelope adds
struct PairEnvDesc : PairProfDesc {      // cellBase: of this pair's compact lattice
  long long envBase;           // first of this pair's nRows + 1 entries in envStart / envEnd / envOff
  long long diagBase;          // first of this pair's nIn + nRows + 1 entries in diagLo / diagCnt
  long long nCells;            // envelope cells of the pair (off[nRows + 1])
  int M;                       // the largest cell count of any anti-diagonal of the pair
};

// device arrays of a batch's envelopes (rows of the pairs that have one, packed)
struct PairEnvTables {
  const int *envStart, *envEnd;   // [rows]
  const long long *envOff;        // [rows] compact index of the first cell of each row, per pair from 0
  const int *diagLo, *diagCnt;    // [diagonals] first i and cell count of each anti-diagonal
};

MB_LATTICE_FN EnvCells lattice_cells(const PairEnvDesc &pd, const PairEnvTables &t) {
  return EnvCells(pd.nIn, pd.nRows, t.envStart + pd.envBase, t.envEnd + pd.envBase, t.envOff + pd.envBase, t.diagLo + pd.diagBase, t.diagCnt + pd.diagBase, pd.nCells, pd.M);
}

// the rolling ring: three anti-diagonals of both layers, each of M cells; a cell lives at i mod M
inline long long profile_pair_env_ring(int S, long long M) { return 3 * 2 * M * (long long)S; }
// dynamic LDS of the ring when it fits (0: a slice of the global scratch buffer)
size_t profile_pair_env_lds_bytes(int S, long long M);


// the launchers of mb_profile_pair.h over pairs under an envelope (lds, maxItems: of the envelope rings)
int launch_profile_pair_fwd(const mb_machine *m, int mode, bool mat, const PairEnvDesc *d, const PairEnvTables &t, int n, size_t lds, long long maxItems,
                            const int *inTok, const double *logP, double *pool, double *scratch, double *loglike, hipStream_t st);
int launch_profile_pair_bwd(const mb_machine *m, const PairEnvDesc *d, const PairEnvTables &t, int n, long long maxItems, const int *inTok, const double *logP,
                            double *pool, double *loglike, hipStream_t st);
int launch_profile_pair_counts(const mb_machine *m, const PairEnvDesc *d, const PairEnvTables &t, int n, int groupsPerPair, const int *inTok, const double *logP,
                               const double *fwdPool, const double *bwdPool, double *counts, hipStream_t st);
int launch_profile_pair_rowpost(const mb_machine *m, const PairEnvDesc *d, const PairEnvTables &t, int n, int groupsPerPair, int tabMax, const int *inTok,
                                const double *logP, const double *fwdPool, const double *bwdPool, double *post, hipStream_t st);
int launch_profile_pair_traceback(const mb_machine *m, const PairEnvDesc *d, const PairEnvTables &t, int n, const int *inTok, const double *logP, const double *pool,
                                  uint32_t *edges, int32_t *rows, long long *len, hipStream_t st);
int launch_profile_pair_sample(const mb_machine *m, const PairEnvDesc *d, const PairEnvTables &t, int n, int nSamples, const long long *pairIdx, unsigned long long seed,
                               const int *inTok, const double *logP, const double *pool, uint32_t *edges, int32_t *rows, long long *len, double *logq,
                               hipStream_t st);

}  // namespace mb
