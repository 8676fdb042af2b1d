// mb_profile.h -- profile tapes: a machine with an empty input tape scored against a table of per-row output-symbol
// weights (a "soft sequence", target/boss.cpp:606-611 --recognize-csv), docs/profile_tapes.md.
//
// Lattice of one profile of L rows: (L+1) rows x 2 layers x S states.  Layer 0 (N) = "arrived at row r", layer 1 (W) = "after
// the machine's silent moves at row r"; materialised cells live at cells[((r*2)+layer)*S + q].
#pragma once
#include <vector>

#include "mb_internal.h"

namespace mb {

struct ProfDesc {
  long long rowBase;    // first row of this profile in the batch's row table (rows of nOut+1 doubles, column 0 = blank)
  long long cellBase;   // offset (doubles) of this profile's lattice in a matrix pool
  long long pathBase;   // offset of this profile's slot in the traceback buffers
  int nRows;
  int pad;
};

inline long long profile_cells(int S, long long nRows) { return (nRows + 1) * 2 * (long long)S; }
// traceback slot of one profile: one emitting edge per row, at most nLevF - 1 silent edges at each of the nRows + 1 rows
inline long long profile_path_bound(int nLevF, long long nRows) { return nRows + (nRows + 1) * (long long)(nLevF - 1); }

// dynamic LDS of the sweeps when the three rolling state vectors fit (0: per-workgroup slices of a global scratch buffer)
size_t profile_lds_bytes(int S);
int launch_profile_fwd(const mb_machine *m, int mode, bool mat, const ProfDesc *d, int n, const double *logP, double *pool,
                       double *scratch, double *loglike, hipStream_t st);
int launch_profile_bwd(const mb_machine *m, bool mat, const ProfDesc *d, int n, const double *logP, double *pool,
                       const double *fwdPool, double *scratch, double *loglike, double *part, long long nTrans, hipStream_t st);
int launch_profile_traceback(const mb_machine *m, const ProfDesc *d, int n, const double *logP, const double *pool,
                             uint32_t *edges, int32_t *rows, long long *len, hipStream_t st);
int launch_profile_sum_counts(const double *part, int n, long long nTrans, double *out, hipStream_t st);

}  // namespace mb

struct mb_profiles {
  mb_machine *m = nullptr;
  long long n = 0, totalRows = 0;
  std::vector<long long> rowOff;   // [n+1], rebased to 0
  double *d_logP = nullptr;        // [totalRows * (nOut+1)]; merged: [totalRows * (nCols+1)]
  int nCols = 0;                   // > 0: CTC-merged profiles (mb_profile_merge.h), rows of nCols + 1 doubles
  int *d_colTok = nullptr;         // [nCols] output token of each column
};
