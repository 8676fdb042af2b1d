// mb_profile_two.h -- two-profile sweeps: a machine with an input alphabet between an input profile of K rows (the generator of
// `--generate-csv`) and an output profile of L rows (docs/profile_tapes.md, "Pairs of profiles").
//
// Lattice of one pair: (K+1) input rows x (L+1) output rows x 3 layers x S states.  Layer 0 (N) = "arrived at (i, r)", layer 1 (W) =
// "after the machine's output-less moves there", layer 2 (Z) = "committed to wait for the next input row"; materialised cells live
// at cells[(((i*(L+1)) + r)*3 + layer)*S + q].  A pair is described by a PairProfDesc whose inBase is the first row of its input
// profile in the batch's input row table (rows of nIn+1 doubles, column 0 = blank) and nIn the number of those rows.  These are the
// launchers over full rectangles; mb_profile_two_env.h declares their overloads for pairs under an envelope.
#pragma once
#include <algorithm>
#include <vector>

#include "mb_profile_pair.h"

namespace mb {

inline long long profile_two_cells(int S, long long nIn, long long nRows) { return (nIn + 1) * (nRows + 1) * 3 * (long long)S; }
// the rolling ring: three anti-diagonals of three layers, each of min(K, L) + 1 cells
inline long long profile_two_ring(int S, long long nIn, long long nRows) { return 3 * 3 * (std::min(nIn, nRows) + 1) * (long long)S; }
// dynamic LDS of a pair's ring when it fits (0: a slice of the global scratch buffer)
size_t profile_two_lds_bytes(int S, long long nIn, long long nRows);

// lds: the dynamic LDS of the launch (the largest ring among the pairs whose ringBase is -1)
int launch_profile_two_fwd(const mb_machine *m, int mode, bool mat, const PairProfDesc *d, int n, size_t lds, long long maxItems, const double *logA,
                           const double *logB, double *pool, double *scratch, double *loglike, hipStream_t st);
int launch_profile_two_bwd(const mb_machine *m, const PairProfDesc *d, int n, long long maxItems, const double *logA, const double *logB, double *pool,
                           double *loglike, hipStream_t st);
// counts[nTrans] += posteriors of the n pairs (fwdPool / bwdPool: their materialised lattices); det: 64-bit fixed point at 2^-36
int launch_profile_two_counts(const mb_machine *m, const PairProfDesc *d, int n, int groupsPerPair, const double *logA, const double *logB,
                              const double *fwdPool, const double *bwdPool, double *counts, hipStream_t st);
// post = the row posteriors of the n pairs on one tape, every bin of every line written (nothing to clear).  axis 0: the output rows,
// post[(rowBase + r) * (nOut+1) + o]; axis 1: the input rows, post[(inBase + i) * (nIn+1) + a].  groupsPerPair: at least the line blocks
// (profile_pair_rowpost_rows over the axis) of the pair that has most, 1 024 at the most; det: post holds 64-bit fixed point at 2^-36
int launch_profile_two_rowpost(const mb_machine *m, int axis, const PairProfDesc *d, int n, int groupsPerPair, int tabMax, const double *logA,
                               const double *logB, const double *fwdPool, const double *bwdPool, double *post, hipStream_t st);
int launch_profile_two_traceback(const mb_machine *m, const PairProfDesc *d, int n, const double *logA, const double *logB, const double *pool,
                                 uint32_t *edges, int32_t *rows, int32_t *inRows, long long *len, hipStream_t st);
// Posterior path samples over the n pairs' materialised sum lattices (k_profile_two_sample): nSamples lanes per pair, n * nSamples
// at most 2^31 - 1.  pair0: the index in the object of the chunk's first pair (the counter of the uniforms).  The slot of sample j of
// a pair is at (pathBase * nSamples + j * bound) of edges / rows / inRows; len and logq are [n * nSamples], pair-major.
int launch_profile_two_sample(const mb_machine *m, const PairProfDesc *d, int n, int nSamples, long long pair0, unsigned long long seed, const double *logA,
                              const double *logB, const double *pool, uint32_t *edges, int32_t *rows, int32_t *inRows, long long *len, double *logq, hipStream_t st);

}  // namespace mb

struct mb_profile_twos {
  mb_machine *m = nullptr;
  long long n = 0, totalRows = 0, totalIn = 0;
  std::vector<long long> rowOff, inOff;   // [n+1], rebased to 0: rows of the output / the input profiles
  double *d_logB = nullptr;               // [totalRows * (nOut+1)]; merged: [totalRows * (nCols+1)]
  double *d_logA = nullptr;               // [totalIn * (nIn+1)]
  int nCols = 0;                          // > 0: CTC-merged output profiles (mb_profile_two_merge.h); they take no envelopes
  int *d_colTok = nullptr;                // [nCols] output token of column c at [c - 1]
  // envelopes (mb_profile_twos_set_envelopes, mb_profile_two_env.h): with hasEnv EVERY pair runs the envelope geometry, a pair
  // that was given none under the full envelope
  bool hasEnv = false;
  std::vector<long long> envBase, diagBase, colBase, envCells;   // [n]: first envelope row / diagonal entry / input-row entry, envelope cells
  std::vector<int> envM;                                         // [n]: the largest cell count of a diagonal
  int *d_envStart = nullptr, *d_envEnd = nullptr, *d_diagLo = nullptr, *d_diagCnt = nullptr, *d_colStart = nullptr, *d_colEnd = nullptr;
  long long *d_envOff = nullptr, *d_colOff = nullptr;
};
