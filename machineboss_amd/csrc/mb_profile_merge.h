// mb_profile_merge.h -- CTC-merged profile tapes (`--recognize-merge-csv`, src/csv.cpp:20-46): the profile sweeps of mb_profile.h with
// a "last column seen" axis of nCols + 1 planes beside the S states (docs/profile_tapes.md, "Merged (CTC) profiles").
//
// Rows of the batch's table hold nCols + 1 doubles: column 0 the blank, column c the log weight of CSV column c, whose output
// token is colTok[c - 1].  Lattice of one profile of L rows: (L+1) rows x 2 layers x (nCols+1) planes x S states, materialised at
// cells[(((r*2) + layer)*(nCols+1) + p)*S + q]; plane 0 = "the last row took the blank, or no row yet", plane c = "the last row took
// column c".  ProfDesc is shared with the plain sweeps: rowBase counts rows of nCols + 1 doubles, cellBase doubles of this layout.
#pragma once
#include "mb_profile.h"

namespace mb {

struct MergeMap {
  int nCols;
  const int *colTok;   // [nCols] device: output token (1..nOut) of column c at colTok[c - 1]
};

inline long long profile_merge_cells(int S, int nCols, long long nRows) { return profile_cells(S, nRows) * (nCols + 1); }
// doubles of one workgroup's rolling state: the exclusion vectors X (nCols planes), two N rows and W (nCols + 1 planes each)
__host__ __device__ inline long long profile_merge_ring(int S, int nCols) { return (3LL * (nCols + 1) + nCols) * S; }
// dynamic LDS of a sweep when its rolling state fits (0: the workgroup's slice of a global scratch buffer of profile_merge_ring
// doubles).  Forward / Viterbi: the whole ring rolling, X alone when materialised; Backward: three vectors rolling, none materialised.
size_t profile_merge_fwd_lds(int S, int nCols, bool mat);
size_t profile_merge_bwd_lds(int S, int nCols);
int launch_profile_merge_fwd(const mb_machine *m, MergeMap mm, int mode, bool mat, const ProfDesc *d, int n, const double *logP,
                             double *pool, double *scratch, double *loglike, hipStream_t st);
// part: [n * (nCols + 1) * nTrans], one accumulator vector per profile and plane (launch_profile_sum_counts over n * (nCols + 1))
int launch_profile_merge_bwd(const mb_machine *m, MergeMap mm, bool mat, const ProfDesc *d, int n, const double *logP, double *pool,
                             const double *fwdPool, double *scratch, double *loglike, double *part, long long nTrans, hipStream_t st);
int launch_profile_merge_traceback(const mb_machine *m, MergeMap mm, const ProfDesc *d, int n, const double *logP, const double *pool,
                                   uint32_t *edges, int32_t *rows, long long *len, hipStream_t st);

}  // namespace mb
