// mb_profile_two_merge.h -- two-profile sweeps against CTC-merged output profiles: a machine with an input alphabet between an input
// profile of K rows and a merged output profile of L rows (docs/profile_tapes.md, "Pairs of profiles against a merged profile").
// The lattice of mb_profile_two.h with the plane axis of mb_profile_merge.h.
//
// Output rows of the batch's table hold nCols + 1 doubles (column 0 the blank, column c the CSV column whose output token is
// colTok[c - 1]); input rows nIn + 1 doubles as in mb_profile_two.h.  Lattice of one pair: (K+1) input rows x (L+1) output rows x 3
// layers x (nCols+1) planes x S states, materialised at cells[((((i*(L+1)) + r)*3 + layer)*(nCols+1) + p)*S + q]; layer 0 (N) =
// "arrived at (i, r)", 1 (W) = "after the machine's output-less moves there", 2 (Z) = "committed to wait for the next input row";
// plane 0 = "the last row took the blank, or no row yet", plane c = "the last row took column c".  PairProfDesc is shared with the
// plain sweeps: rowBase counts rows of nCols + 1 doubles, cellBase doubles of this layout, ringBase the pair's slice of the global
// scratch buffer (-1: its ring is in LDS).
//
// Under an ENVELOPE (mb_profile_two_env.h; docs/profile_tapes.md, "Pairs of profiles against a merged profile under an envelope")
// cell (i, r) exists iff inStart[r] <= i < inEnd[r], in every plane of every layer; everything else is -inf.  Materialised lattices
// are then COMPACT: cells[(((off[r] + i - inStart[r]) * 3 + layer) * (nCols + 1) + p) * S + q], off[r] = the cells of the rows < r.
// The descriptor and the tables are those of the plain two-profile pairs under an envelope, TwoEnvDesc and TwoEnvTables.
#pragma once
#include "mb_profile_merge.h"
#include "mb_profile_two_env.h"

namespace mb {

inline long long profile_two_merge_cells(int S, int nCols, long long nIn, long long nRows) {
  return profile_two_cells(S, nIn, nRows) * (nCols + 1);
}
// The ring of a sweep: three anti-diagonals of min(K, L) + 1 cells.  A rolling Forward / Viterbi keeps N, W, Z (nCols + 1 planes
// each) and the two exclusion vectors XW, XZ (nCols planes each) of every cell: 3 (5 nCols + 3)(min(K, L) + 1) S doubles.  The
// materialised Forward / Viterbi keeps XW and XZ alone, the Backward the per-column sums TZ and TW of one diagonal (held in a ring
// of the same shape).
inline long long profile_two_merge_ring(int S, int nCols, long long nIn, long long nRows, bool mat) {
  return 3 * (mat ? 2LL * nCols : 5LL * nCols + 3) * (std::min(nIn, nRows) + 1) * (long long)S;
}
// dynamic LDS of a pair's ring when it fits 160 KiB (0: a slice of the global scratch buffer)
size_t profile_two_merge_lds_bytes(int S, int nCols, long long nIn, long long nRows, bool mat);
// the same under an envelope: three anti-diagonals of M cells, M the largest cell count of a diagonal; a cell lives at i mod M
// (the Backward's TZ and TW: the cell by its place on the diagonal, at most M places)
inline long long profile_two_merge_env_ring(int S, int nCols, long long M, bool mat) {
  return 3 * (mat ? 2LL * nCols : 5LL * nCols + 3) * M * (long long)S;
}
size_t profile_two_merge_env_lds_bytes(int S, int nCols, long long M, bool mat);

// lds: the dynamic LDS of the launch (the largest ring among the pairs whose ringBase is -1); maxItems: the most (cell, plane,
// state) items on one diagonal of the batch
int launch_profile_two_merge_fwd(const mb_machine *m, MergeMap mm, int mode, bool mat, const PairProfDesc *d, int n, size_t lds,
                                 long long maxItems, const double *logA, const double *logB, double *pool, double *scratch,
                                 double *loglike, hipStream_t st);
int launch_profile_two_merge_bwd(const mb_machine *m, MergeMap mm, const PairProfDesc *d, int n, size_t lds, long long maxItems,
                                 const double *logA, const double *logB, double *pool, double *scratch, double *loglike, hipStream_t st);
// counts[nTrans] += posteriors of the n pairs (fwdPool / bwdPool: their materialised lattices); det: 64-bit fixed point at 2^-36
int launch_profile_two_merge_counts(const mb_machine *m, MergeMap mm, const PairProfDesc *d, int n, int groupsPerPair, const double *logA,
                                    const double *logB, const double *fwdPool, const double *bwdPool, double *counts, hipStream_t st);
// post = the row posteriors of the n pairs on one axis (0: post[(rowBase + r) * (nCols + 1) + c], 1: post[(inBase + i) * (nIn + 1) + a]),
// every bin of every line written (nothing to clear); groupsPerPair: at least the line blocks (profile_pair_rowpost_rows over lines
// of (K + 1)(nCols + 1) S items on axis 0, (L + 1)(nCols + 1) S on axis 1) of the pair that has most, 1 024 at the most; loglike: the
// Forward sweep's, per pair of the launch; det: post holds 64-bit fixed point at 2^-36
int launch_profile_two_merge_rowpost(const mb_machine *m, MergeMap mm, int axis, const PairProfDesc *d, int n, int groupsPerPair, int tabMax,
                                     const double *logA, const double *logB, const double *fwdPool, const double *bwdPool,
                                     const double *loglike, double *post, hipStream_t st);
int launch_profile_two_merge_traceback(const mb_machine *m, MergeMap mm, const PairProfDesc *d, int n, const double *logA,
                                       const double *logB, const double *pool, uint32_t *edges, int32_t *rows, int32_t *inRows,
                                       long long *len, hipStream_t st);

// the launchers above over pairs under an envelope (lds, maxItems: of the envelope rings and diagonals)
int launch_profile_two_merge_fwd(const mb_machine *m, MergeMap mm, int mode, bool mat, const TwoEnvDesc *d, const TwoEnvTables &t, int n, size_t lds,
                                 long long maxItems, const double *logA, const double *logB, double *pool, double *scratch,
                                 double *loglike, hipStream_t st);
int launch_profile_two_merge_bwd(const mb_machine *m, MergeMap mm, const TwoEnvDesc *d, const TwoEnvTables &t, int n, size_t lds, long long maxItems,
                                 const double *logA, const double *logB, double *pool, double *scratch, double *loglike, hipStream_t st);
int launch_profile_two_merge_counts(const mb_machine *m, MergeMap mm, const TwoEnvDesc *d, const TwoEnvTables &t, int n, int groupsPerPair, const double *logA,
                                    const double *logB, const double *fwdPool, const double *bwdPool, double *counts, hipStream_t st);
int launch_profile_two_merge_rowpost(const mb_machine *m, MergeMap mm, int axis, const TwoEnvDesc *d, const TwoEnvTables &t, int n, int groupsPerPair, int tabMax,
                                     const double *logA, const double *logB, const double *fwdPool, const double *bwdPool,
                                     const double *loglike, double *post, hipStream_t st);
int launch_profile_two_merge_traceback(const mb_machine *m, MergeMap mm, const TwoEnvDesc *d, const TwoEnvTables &t, int n, const double *logA,
                                       const double *logB, const double *pool, uint32_t *edges, int32_t *rows, int32_t *inRows,
                                       long long *len, hipStream_t st);

}  // namespace mb
