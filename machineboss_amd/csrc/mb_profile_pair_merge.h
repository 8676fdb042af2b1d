// mb_profile_pair_merge.h -- two-tape sweeps against CTC-merged profiles: a machine with an input alphabet, a known input sequence
// x[1..I] and a merged profile of L rows as the soft output (docs/profile_tapes.md, "Pairs against a merged profile").  The lattice
// of mb_profile_pair.h with the plane axis of mb_profile_merge.h.
//
// Rows of the batch's table hold nCols + 1 doubles (column 0 the blank, column c the CSV column whose output token is
// colTok[c - 1]).  Lattice of one pair: (I+1) input positions x (L+1) rows x 2 layers x (nCols+1) planes x S states, materialised
// at cells[((((i*(L+1)) + r)*2 + layer)*(nCols+1) + p)*S + q]; layer 0 (N) = "arrived at (i, r)", layer 1 (W) = "after the machine's
// output-less moves there"; plane 0 = "the last row took the blank, or no row yet", plane c = "the last row took column c".
// PairProfDesc is shared with the plain pair sweeps: rowBase counts rows of nCols + 1 doubles, cellBase doubles of this layout,
// ringBase the pair's slice of the global scratch buffer (-1: its ring is in LDS).
//
// Under an ENVELOPE (mb_profile_pair_env.h; docs/profile_tapes.md, "Pairs against a merged profile under an envelope") cell (i, r)
// exists iff inStart[r] <= i < inEnd[r], in every plane; everything else is -inf.  Materialised lattices are then COMPACT:
// cells[(((off[r] + i - inStart[r]) * 2 + layer) * (nCols + 1) + p) * S + q], off[r] = the cells of the rows < r.  The descriptor
// and the tables are those of the plain pairs under an envelope, PairEnvDesc and PairEnvTables.
#pragma once
#include "mb_profile_merge.h"
#include "mb_profile_pair_env.h"

namespace mb {

inline long long profile_pair_merge_cells(int S, int nCols, long long nIn, long long nRows) {
  return profile_pair_cells(S, nIn, nRows) * (nCols + 1);
}
// The ring of a sweep: three anti-diagonals of min(I, L) + 1 cells.  A rolling Forward / Viterbi keeps N, W (nCols + 1 planes each)
// and the exclusion vectors X (nCols planes) of every cell: 3 (3 nCols + 2) (min(I, L) + 1) S doubles.  The materialised Forward /
// Viterbi keeps X alone, the Backward the per-column sums T of one diagonal (held in a ring of the same shape as X).
inline long long profile_pair_merge_ring(int S, int nCols, long long nIn, long long nRows, bool mat) {
  return 3 * (mat ? (long long)nCols : 3LL * nCols + 2) * (std::min(nIn, nRows) + 1) * (long long)S;
}
// dynamic LDS of a pair's ring when it fits 160 KiB (0: a slice of the global scratch buffer)
size_t profile_pair_merge_lds_bytes(int S, int nCols, long long nIn, long long nRows, bool mat);
// the same under an envelope: three anti-diagonals of M cells, M the largest cell count of a diagonal; a cell lives at i mod M
inline long long profile_pair_merge_env_ring(int S, int nCols, long long M, bool mat) {
  return 3 * (mat ? (long long)nCols : 3LL * nCols + 2) * M * (long long)S;
}
size_t profile_pair_merge_env_lds_bytes(int S, int nCols, long long M, bool mat);

// lds: the dynamic LDS of the launch (the largest ring among the pairs whose ringBase is -1); maxItems: the most (cell, plane,
// state) items on one diagonal of the batch
int launch_profile_pair_merge_fwd(const mb_machine *m, MergeMap mm, int mode, bool mat, const PairProfDesc *d, int n, size_t lds,
                                  long long maxItems, const int *inTok, const double *logP, double *pool, double *scratch,
                                  double *loglike, hipStream_t st);
int launch_profile_pair_merge_bwd(const mb_machine *m, MergeMap mm, const PairProfDesc *d, int n, size_t lds, long long maxItems,
                                  const int *inTok, const double *logP, double *pool, double *scratch, double *loglike, hipStream_t st);
// counts[nTrans] += posteriors of the n pairs (fwdPool / bwdPool: their materialised lattices); det: 64-bit fixed point at 2^-36
int launch_profile_pair_merge_counts(const mb_machine *m, MergeMap mm, const PairProfDesc *d, int n, int groupsPerPair, const int *inTok,
                                     const double *logP, const double *fwdPool, const double *bwdPool, double *counts, hipStream_t st);
// post[(rowBase + r) * (nCols + 1) + c] = the row posteriors of the n pairs, every bin of every row written (nothing to clear);
// groupsPerPair: at least the row blocks (profile_pair_rowpost_rows over rows of (I + 1)(nCols + 1) S items) of the pair that has
// most, 1 024 at the most; loglike: the Forward's, per pair; det: post holds 64-bit fixed point at 2^-36
int launch_profile_pair_merge_rowpost(const mb_machine *m, MergeMap mm, const PairProfDesc *d, int n, int groupsPerPair, int tabMax,
                                      const int *inTok, const double *logP, const double *fwdPool, const double *bwdPool,
                                      const double *loglike, double *post, hipStream_t st);
int launch_profile_pair_merge_traceback(const mb_machine *m, MergeMap mm, const PairProfDesc *d, int n, const int *inTok,
                                        const double *logP, const double *pool, uint32_t *edges, int32_t *rows, long long *len,
                                        hipStream_t st);

// Posterior path samples over the n pairs' materialised sum lattices (k_profile_pair_merge_sample): nSamples lanes per pair, n *
// nSamples <= 2^31 - 1.  pairIdx[n]: each pair's index in the object, the `k` of the generator's counter.  Sample j of the pair at
// d[s] writes len / logq at s * nSamples + j, its path at (d[s].pathBase * nSamples + j * bound), bound = profile_pair_path_bound of
// the pair, and the column every row took at rowCol[(d[s].rowBase - rowBase0) * nSamples + j * nRows + r].
int launch_profile_pair_merge_sample(const mb_machine *m, MergeMap mm, const PairProfDesc *d, int n, int nSamples, const long long *pairIdx, unsigned long long seed,
                                     const int *inTok, const double *logP, const double *pool, long long rowBase0, uint32_t *edges, int32_t *rows, int32_t *rowCol,
                                     long long *len, double *logq, hipStream_t st);

// the launchers above over pairs under an envelope (lds, maxItems: of the envelope rings and diagonals)
int launch_profile_pair_merge_fwd(const mb_machine *m, MergeMap mm, int mode, bool mat, const PairEnvDesc *d, const PairEnvTables &t, int n, size_t lds,
                                  long long maxItems, const int *inTok, const double *logP, double *pool, double *scratch,
                                  double *loglike, hipStream_t st);
int launch_profile_pair_merge_bwd(const mb_machine *m, MergeMap mm, const PairEnvDesc *d, const PairEnvTables &t, int n, size_t lds, long long maxItems,
                                  const int *inTok, const double *logP, double *pool, double *scratch, double *loglike, hipStream_t st);
int launch_profile_pair_merge_counts(const mb_machine *m, MergeMap mm, const PairEnvDesc *d, const PairEnvTables &t, int n, int groupsPerPair, const int *inTok,
                                     const double *logP, const double *fwdPool, const double *bwdPool, double *counts, hipStream_t st);
int launch_profile_pair_merge_rowpost(const mb_machine *m, MergeMap mm, const PairEnvDesc *d, const PairEnvTables &t, int n, int groupsPerPair, int tabMax,
                                      const int *inTok, const double *logP, const double *fwdPool, const double *bwdPool,
                                      const double *loglike, double *post, hipStream_t st);
int launch_profile_pair_merge_traceback(const mb_machine *m, MergeMap mm, const PairEnvDesc *d, const PairEnvTables &t, int n, const int *inTok,
                                        const double *logP, const double *pool, uint32_t *edges, int32_t *rows, long long *len,
                                        hipStream_t st);
int launch_profile_pair_merge_sample(const mb_machine *m, MergeMap mm, const PairEnvDesc *d, const PairEnvTables &t, int n, int nSamples, const long long *pairIdx,
                                     unsigned long long seed, const int *inTok, const double *logP, const double *pool, long long rowBase0, uint32_t *edges,
                                     int32_t *rows, int32_t *rowCol, long long *len, double *logq, hipStream_t st);

}  // namespace mb
