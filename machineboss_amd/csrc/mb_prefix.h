// mb_prefix.h -- prefix-tree node fills (src/ctc.cpp:25-88 PrefixTree::Node::fill), docs/decoding.md.
//
// A node is an input prefix x[1..n] of one search (one output sequence y[1..L]); its lattice is (L+1) rows x 2 layers x S states:
// layer 0 (seq) = Forward likelihood of the pair (x, y[1..j]) ending in the state, layer 1 (prefix) = likelihood of y[1..j] given
// any input that starts with x.  Cells live at cells[((j*2)+layer)*S + d] inside the node's slot of the pool.  The device owns the
// lattices; the tree (who is whose parent, which slots are live, the heap) is the host's.
#pragma once
#include <vector>

#include "mb_internal.h"

namespace mb {

struct PrefixDesc {
  long long parentBase;   // offset (doubles) of the parent's slot in the pool, -1: this node is a root
  long long childBase;    // offset of the slot to fill
  long long outBase;      // first output token of the node's search in the token array (profile searches: its first row)
  int outLen;             // number of output tokens (rows)
  int inTok;              // the node's own input token (1..nIn), 0 for a root
};

// R = log((I - N)^-1) by COLUMN: entries rOff[s]..rOff[s+1] are the finite R[p][s], p ascending (rIdx = p, rVal = R[p][s])
struct PrefixR {
  const long long *rOff;
  const int *rIdx;
  const double *rVal;
};

inline long long prefix_slot_doubles(int S, long long maxOutLen) { return 2 * (maxOutLen + 1) * (long long)S; }
// the V row of a workgroup lives in LDS: S doubles
constexpr int PREFIX_MAX_STATES = 160 * 1024 / 8;
// against profiles N[r-1], Xn[r-1] and the row's nOut + 1 weights sit beside it: 3 S + nOut + 1 doubles
constexpr size_t PREFIX_PROFILE_MAX_LDS = 160 * 1024;
// against CTC-merged profiles (mb_prefix_merge.hip) a node has nCols + 1 planes of the plain lattice, and a workgroup keeps in LDS
// Y[r-1], N[r-1] and Xn[r-1] (nCols + 1 planes of S each), the three exclusion vectors (nCols planes of S each), the two blank sums
// (S each) and the row's nCols + 1 weights: (6 nCols + 5) S + nCols + 1 doubles, at most PREFIX_PROFILE_MAX_LDS bytes
inline long long merged_prefix_lds_doubles(int S, int nCols) { return (6LL * nCols + 5) * S + nCols + 1; }
inline bool merged_prefix_lds_fits(int S, int nCols) { return (unsigned long long)merged_prefix_lds_doubles(S, nCols) * sizeof(double) <= PREFIX_PROFILE_MAX_LDS; }
inline long long merged_prefix_slot_doubles(int S, int nCols, long long maxOutLen) { return prefix_slot_doubles(S, maxOutLen) * (nCols + 1); }

int launch_prefix_fill(const mb_machine *m, const PrefixR &R, const PrefixDesc *d, int n, const int *outTok, double *pool,
                       double *result /* [2n]: logSeqProb, logPrefixProb per entry */, hipStream_t st);
// the same against profiles: logP holds rows of nOut + 1 log weights (column 0 the blank), outBase / outLen of a descriptor count rows
int launch_prefix_fill_profile(const mb_machine *m, const PrefixR &R, const PrefixDesc *d, int n, const double *logP, double *pool,
                               double *result, hipStream_t st);
// the same against CTC-merged profiles: rows of nCols + 1 log weights (column 0 the blank, column c of output token colTok[c - 1], a
// device array), slots of merged_prefix_slot_doubles laid out as cells[(((r*2) + layer)*(nCols+1) + p)*S + q]
int launch_prefix_fill_merged(const mb_machine *m, const PrefixR &R, int nCols, const int *colTok, const PrefixDesc *d, int n,
                              const double *logP, double *pool, double *result, hipStream_t st);

}  // namespace mb

struct mb_prefix {
  mb_machine *m = nullptr;
  long long nSeq = 0, maxNodes = 0, slotDoubles = 0, maxOutLen = 0;
  std::vector<long long> outOff;     // [nSeq+1], rebased to 0
  int *d_out = nullptr;              // output tokens of every search
  bool profile = false;              // the searches decode profiles: outOff counts rows of d_logP, d_out is unused
  double *d_logP = nullptr;          // [rows][nOut + 1] log weights of every search's profile, column 0 the blank
  int nCols = 0;                     // > 0: the profiles are CTC-merged (mb_prefix_merge.hip): rows of nCols + 1 doubles, nCols + 1 planes per slot
  int *d_colTok = nullptr;           // [nCols] output token of each column
  long long *d_rOff = nullptr;       // R by column (PrefixR)
  int *d_rIdx = nullptr;
  double *d_rVal = nullptr;
  double *pool = nullptr;            // maxNodes slots of slotDoubles
  bool poolIsWorkspace = false;      // the pool is the library's cached node-pool workspace (else an allocation of this object)
  std::vector<long long> freeSlots;  // stack of free slots
  std::vector<long long> slotSeq;    // [maxNodes]: search of a live slot, -1 = free
};
