// mb_profile_post.h -- row posteriors of the one-tape profile sweeps (mb_profile_post.hip; docs/profile_tapes.md, "Row posteriors of
// one-tape profiles"): the gradient of a profile's log-likelihood in its rows, for plain and for CTC-merged profiles.
#pragma once
#include "mb_profile_merge.h"
#include "mb_profile_pair.h"

namespace mb {

// rows of one block of k_profile_rowpost: the rule of k_profile_pair_rowpost over rows of planes x S items
inline int profile_rowpost_rows(int S, int planes, long long nRows, int C, int tabMax) {
  return profile_pair_rowpost_rows((nRows + 1) * planes, S, (int)nRows, C, tabMax);
}

// post[(rowBase + r) * C + x] = the row posteriors of the n profiles, every bin of every row written (nothing to clear); C = nOut + 1,
// or mm.nCols + 1 for merged profiles (mm.nCols > 0).  fwdPool / bwdPool: their materialised lattices, loglike[n] their Forward
// likelihoods (device).  groupsPerProf: at least 1, at most the row blocks of the profile that has most; det (g_deterministic): post
// holds 64-bit fixed point at 2^-36.
int launch_profile_rowpost(const mb_machine *m, MergeMap mm, const ProfDesc *d, int n, int groupsPerProf, int tabMax, const double *logP,
                           const double *fwdPool, const double *bwdPool, const double *loglike, double *post, hipStream_t st);

}  // namespace mb
