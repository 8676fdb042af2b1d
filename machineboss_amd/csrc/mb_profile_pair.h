// mb_profile_pair.h -- two-tape profile sweeps: a machine with an input alphabet, a known input sequence x[1..I] and a profile of L
// rows as the soft output (docs/profile_tapes.md, "Pairs: an input sequence against a profile").
//
// Lattice of one pair: (I+1) input positions x (L+1) rows x 2 layers x S states.  Layer 0 (N) = "arrived at (i, r)", layer 1 (W) =
// "after the machine's output-less moves there"; materialised cells live at cells[(((i*(L+1)) + r)*2 + layer)*S + q].
#pragma once
#include <algorithm>
#include <vector>

#include "mb_internal.h"
#include "mb_profile_lattice.h"

namespace mb {

struct PairProfDesc {
  long long inBase;     // first input token of this pair in the batch's token array
  long long rowBase;    // first row of this pair's profile in the batch's row table (rows of nOut+1 doubles, column 0 = blank)
  long long cellBase;   // offset (doubles) of this pair's lattice in a matrix pool
  long long pathBase;   // offset of this pair's slot in the traceback buffers
  long long ringBase;   // rolling sweeps: offset (doubles) of this pair's ring in the global scratch buffer, -1 = the ring is in LDS
  int nIn, nRows;
};

// which cells of the pair's lattice exist and where they live (mb_profile_lattice.h)
MB_LATTICE_FN RectCells lattice_cells(const PairProfDesc &pd, NoTables) { return RectCells(pd.nIn, pd.nRows); }

inline long long profile_pair_cells(int S, long long nIn, long long nRows) { return (nIn + 1) * (nRows + 1) * 2 * (long long)S; }
// traceback slot: at most nIn input-consuming and nRows output-only edges, and nLevF - 1 silent edges at each of the at most
// nIn + nRows + 1 cells a path visits
inline long long profile_pair_path_bound(int nLevF, long long nIn, long long nRows) {
  return nIn + nRows + (nIn + nRows + 1) * (long long)(nLevF - 1);
}
// the rolling ring: three anti-diagonals of both layers, each of min(I, L) + 1 cells
inline long long profile_pair_ring(int S, long long nIn, long long nRows) { return 3 * 2 * (std::min(nIn, nRows) + 1) * (long long)S; }
// dynamic LDS of a pair's ring when it fits (0: a slice of the global scratch buffer)
size_t profile_pair_lds_bytes(int S, long long nIn, long long nRows);

// Row posteriors (k_profile_pair_rowpost): a workgroup of ROWPOST_THREADS lanes owns blocks of whole rows and keeps their bins, rows of
// the block x C doubles, in an LDS table of at most tabMax <= ROWPOST_LDS_MAX doubles.  The rows of a block: enough for about
// ROWPOST_ITEMS (cell, state) items, as many as the table holds at the most; 1 where a single row does not fit it (its bins are then
// summed in global memory).  cells: of the pair's lattice, the rectangle or its envelope.
static constexpr int ROWPOST_THREADS = 256;
static constexpr int ROWPOST_LDS_MAX = 4096;
static constexpr int ROWPOST_ITEMS = 8192;
__host__ __device__ inline int profile_pair_rowpost_rows(long long cells, int S, int L, int C, int tabMax) {
  if (L <= 0 || C > tabMax) return 1;
  const long long perRow = cells * S / (L + 1) > 1 ? cells * S / (L + 1) : 1, want = (ROWPOST_ITEMS + perRow - 1) / perRow;
  const long long rows = want < tabMax / C ? want : tabMax / C;
  return (int)(rows < L ? rows : L);
}

// The launchers, one per sweep, over full rectangles; mb_profile_pair_env.h declares their overloads for pairs under an envelope.
// lds: the dynamic LDS of the launch (the largest ring among the pairs whose ringBase is -1)
int launch_profile_pair_fwd(const mb_machine *m, int mode, bool mat, const PairProfDesc *d, int n, size_t lds, long long maxItems, const int *inTok,
                            const double *logP, double *pool, double *scratch, double *loglike, hipStream_t st);
int launch_profile_pair_bwd(const mb_machine *m, const PairProfDesc *d, int n, long long maxItems, const int *inTok, const double *logP, double *pool,
                            double *loglike, hipStream_t st);
// counts[nTrans] += posteriors of the n pairs (fwdPool / bwdPool: their materialised lattices); det: 64-bit fixed point at 2^-36
int launch_profile_pair_counts(const mb_machine *m, const PairProfDesc *d, int n, int groupsPerPair, const int *inTok, const double *logP,
                               const double *fwdPool, const double *bwdPool, double *counts, hipStream_t st);
int launch_profile_pair_traceback(const mb_machine *m, const PairProfDesc *d, int n, const int *inTok, const double *logP, const double *pool,
                                  uint32_t *edges, int32_t *rows, long long *len, hipStream_t st);
// Posterior path samples over the n pairs' materialised sum lattices (k_profile_pair_sample): nSamples lanes per pair, n * nSamples
// <= 2^31 - 1.  pairIdx[n]: each pair's index in the object, the `k` of the generator's counter.  Sample j of the pair at d[s] writes
// len / logq at s * nSamples + j and its path at (d[s].pathBase * nSamples + j * bound), bound = profile_pair_path_bound of the pair.
int launch_profile_pair_sample(const mb_machine *m, const PairProfDesc *d, int n, int nSamples, const long long *pairIdx, unsigned long long seed, const int *inTok,
                               const double *logP, const double *pool, uint32_t *edges, int32_t *rows, long long *len, double *logq, hipStream_t st);
// post[(rowBase + r) * C + o] = the row posteriors of the n pairs, every bin of every row written (nothing to clear); groupsPerPair:
// at least the row blocks of the pair that has most; det: post holds 64-bit fixed point at 2^-36
int launch_profile_pair_rowpost(const mb_machine *m, const PairProfDesc *d, int n, int groupsPerPair, int tabMax, const int *inTok, const double *logP,
                                const double *fwdPool, const double *bwdPool, double *post, hipStream_t st);

}  // namespace mb

struct mb_profile_pairs {
  mb_machine *m = nullptr;
  long long n = 0, totalRows = 0, totalIn = 0;
  std::vector<long long> rowOff, inOff;   // [n+1], rebased to 0
  double *d_logP = nullptr;               // [totalRows * (nOut+1)]; merged: [totalRows * (nCols+1)]
  int *d_in = nullptr;                    // [totalIn]
  int nCols = 0;                          // > 0: CTC-merged profiles (mb_profile_pair_merge.h)
  int *d_colTok = nullptr;                // [nCols] output token of column c at [c - 1]
  // envelopes (mb_profile_pairs_set_envelopes, mb_profile_pair_env.h): the pairs with envBase >= 0 run the envelope kernels
  bool hasEnv = false;
  std::vector<long long> envBase, diagBase, envCells;   // [n]: first envelope row / first diagonal entry (-1: full), envelope cells
  std::vector<int> envM;                                // [n]: the largest cell count of a diagonal
  std::vector<int> h_envStart, h_envEnd;                // the rows of the pairs that have an envelope, packed
  int *d_envStart = nullptr, *d_envEnd = nullptr, *d_diagLo = nullptr, *d_diagCnt = nullptr;
  long long *d_envOff = nullptr;
};
