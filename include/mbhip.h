/* mbhip.h -- C-ABI of the MI355X (gfx950) Forward / Backward / Viterbi DP engine for Machine Boss.
 *
 * This is the drop-in boundary for the reference's DP hot path.  The reference has no FFI layer: its
 * boundary is the C++ class interface of src/{dpmatrix,forward,backward,viterbi,counts,logsumexp}.h
 * ("construction is computation").  Each entry point below names the reference interface it replaces
 * (paths relative to the reference repository root).  INTEGRATION.md shows the C++ shim that re-implements
 * those classes on top of this header.
 *
 * Conventions
 *  - plain pointers and sizes only; all buffers are caller-owned host memory unless stated otherwise;
 *    the library owns device memory.  Calls are synchronous.
 *  - threading: the reference has no threads on this path.  Every entry point below takes one
 *    process-wide lock (ApiGuard, mb_api.hip), so calls from several host threads are safe and are serialised -- the
 *    device workspaces and compiled programs are process-wide; scale out with one process per GPU, not with threads.
 *    mb_last_error() is thread-local.  A filled matrix handed back to the caller is plain host memory.
 *  - every function returning int returns 0 on success, non-zero on error; mb_last_error() then gives the
 *    message the reference would have put into its runtime_error (src/util.cpp:39-48).
 *  - tokens are int32, token 0 = epsilon, tokens 1..N index the sorted alphabet (src/eval.h:13-22).
 *  - transitions ("edges") are identified by their GLOBAL id e = transOffset[src] + transIndex, the order in
 *    which EvaluatedMachine::init visits them (src/eval.cpp:47-69).  counts[] and Viterbi paths use these ids.
 *  - matrices use the reference's IdentityIndexMapper layout with a full envelope (src/dpmatrix.h:34-44,90-96):
 *        cell(inPos,outPos,state) = cells[((outPos*(inLen+1)) + inPos)*nStates + state]      (double)
 *  - envelopes (src/seqpair.h:75-97) restrict the cells that exist: mb_batch_set_envelopes / mb_fill_env.  The matrix
 *    handed back is still the full rectangle; cells outside the envelope hold -inf, which is what the reference's
 *    const cell() accessor returns for them (src/dpmatrix.h:142-144).  Note the reference's 3-argument DPMatrix
 *    constructor ignores its Envelope argument and uses Envelope(seqPair): the alignment's path envelope if the pair
 *    carries an alignment, else the full one (src/dpmatrix.defs.h:16-17, src/seqpair.cpp:104-110) -- the host shims
 *    (mb_dp.hpp, dp.py) reproduce that choice.
 */
#ifndef MBHIP_H_INCLUDED
#define MBHIP_H_INCLUDED

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct mb_machine mb_machine; /* device-resident flattened EvaluatedMachine (src/eval.h:59-98) */
typedef struct mb_batch mb_batch;     /* device-resident tokenised SeqPairList (src/seqpair.h:56-121)   */

/* fill modes for mb_fill / mb_batch_fill */
enum { MB_FORWARD = 0, MB_VITERBI = 1, MB_BACKWARD = 2 };

/* mb_batch_forward flags */
enum {
  MB_MATERIALISE = 0, /* ForwardMatrix: full (inLen+1)(outLen+1)nStates matrix kept in HBM (src/forward.h:19-27)  */
  MB_ROLLING = 1      /* RollingOutputForwardMatrix: log-likelihood only (src/dpmatrix.h:46-58, target/boss.cpp:799) */
};

/* ---- process / device ------------------------------------------------------------------------------------ */
int mb_device_count(void);        /* number of visible HIP devices (0 if none)                                 */
int mb_set_device(int device);    /* one process drives one GPU (rank-local device)                            */
int mb_synchronize(void);         /* wait for everything the library queued on its device (every compute entry point returns with its
                                     results on the host already; this is the timing bracket of a multi-rank host, bench.py)   */
const char *mb_last_error(void);  /* thread-local message of the last failing call                             */
double mb_last_device_ms(void);   /* device time (HIP events on the library's stream) of the last batch call   */
const char *mb_last_kernel_name(void); /* name of the dominant kernel of the last batch call (for profiles)     */
int64_t mb_last_launch_count(void);    /* launches of that kernel in the last batch call                            */

/* ---- machine ----------------------------------------------------------------------------------------------
 * Replaces the per-state incoming/outgoing maps built by EvaluatedMachine::init (src/eval.cpp:40-70).
 * Edges are passed in global-id order (ascending src, then transIndex).  The library derives
 *   - the `incoming` iteration order (dst, inTok, outTok, src, insertion order)   src/eval.h:66-68, eval.cpp:60-61
 *   - the `outgoing` iteration order (src, inTok, outTok, dst, insertion order)
 *   - silent-transition levels (the reference relies on state order; src/eval.cpp:44, machine.cpp:758-764)
 * Returns NULL on error (e.g. "Machine is not topologically sorted").  nInTok/nOutTok exclude epsilon. */
mb_machine *mb_machine_create(int32_t nStates, int32_t nInTok, int32_t nOutTok, int64_t nTrans,
                              const uint32_t *src, const uint32_t *dst, const uint16_t *inTok,
                              const uint16_t *outTok, const double *logWeight);
/* New log-weights for the same topology: one call per EM iteration (src/fitter.cpp:28-29). */
int mb_machine_set_weights(mb_machine *m, const double *logWeight);
void mb_machine_destroy(mb_machine *m);
int32_t mb_machine_n_states(const mb_machine *m);
int64_t mb_machine_n_trans(const mb_machine *m);
int32_t mb_machine_n_levels(const mb_machine *m); /* depth of the silent-transition DAG + 1 */
/* Edge ids in the reference's iteration order, for tests: which = 0 incoming, 1 outgoing. out[nTrans]. */
int mb_machine_edge_order(const mb_machine *m, int which, uint32_t *out);

/* ---- batch of sequence pairs ------------------------------------------------------------------------------
 * Replaces the `for (const auto& seqPair: data.seqPairs)` loops of target/boss.cpp:796,826 and
 * src/counts.cpp:40-42: the whole list is tokenised by the caller (Tokenizer::tokenize, src/eval.h:29-41),
 * handed over once, and kept resident in HBM.  Pair p has input tokens inTok[inOff[p]..inOff[p+1]) and output
 * tokens outTok[outOff[p]..outOff[p+1]).  Tokens outside [1,nInTok] / [1,nOutTok] are rejected with the
 * reference's "Can't tokenize symbol" condition (src/eval.h:33-37). */
mb_batch *mb_batch_create(mb_machine *m, int64_t nPairs, const int32_t *inTok, const int64_t *inOff,
                          const int32_t *outTok, const int64_t *outOff);
void mb_batch_destroy(mb_batch *b);
int64_t mb_batch_cells(const mb_batch *b); /* sum over pairs of (inLen+1)(outLen+1)nStates */
/* ONE-TAPE machines (generators / recognisers of >= 256 states), every call below: a batch of fewer sequences than the device has CUs,
 * whose longest sequence has >= MB_ONETAPE_PARTS_MIN_LEN (4 096) symbols, is swept with k workgroups per sequence (the machine cut along
 * its strongly connected components).  Viterbi matrices, scores and paths are the same bits as with one workgroup; sums
 * move in the last digits.  A workgroup waits for another part's value at most MB_ONETAPE_PART_TIMEOUT_S (20) seconds: past that the
 * CALL FAILS (non-zero return, mb_last_error names the wait) -- it neither hangs nor returns partial results.  MB_ONETAPE_PARTS=1: off. */
/* Envelopes of the pairs (Envelope::inStart / inEnd, src/seqpair.h:75-97): pair p owns rows envOff[p]..envOff[p+1] of
 * inStart[] / inEnd[] -- either outLen+1 rows (cell (x,y) exists <=> inStart[y] <= x < inEnd[y]) or none (full).
 * Rejected like DPMatrix::alloc does (src/dpmatrix.defs.h:31-32): "Envelope/sequence mismatch", "Envelope is not
 * connected".  Restricted envelopes run on the fast families too (the JENV variants of the small-machine and tiled
 * kernels clip every cell outside its row's [inStart, inEnd) to -inf and do not launch tiles that hold no cell of any
 * envelope); one-tape machines and the ahead-of-time fallback take the generic family. */
int mb_batch_set_envelopes(mb_batch *b, const int64_t *envOff, const int32_t *inStart, const int32_t *inEnd);

/* Forward log-likelihoods, loglike[nPairs] (-inf allowed).
 * MB_MATERIALISE = ForwardMatrix(eval, sp).logLike()             src/forward.defs.h:23-55, src/api.cpp:32-35
 * MB_ROLLING     = RollingOutputForwardMatrix(eval, sp).logLike() target/boss.cpp:799-800               */
int mb_batch_forward(mb_batch *b, int flags, double *loglike);

/* ViterbiMatrix(eval, sp): logLike() and path()                   src/viterbi.cpp:18-51, dpmatrix.defs.h:61-110
 * loglike[nPairs]; pathOff[nPairs+1] (output) delimits each pair's start->end list of global edge ids in
 * pathEdges[pathCap].  A pair whose end cell is -inf gets an empty path (the reference refuses to trace it,
 * src/dpmatrix.defs.h:84, target/boss.cpp:831).  pathEdges may be NULL to skip tracebacks.
 * mb_viterbi_path_bound gives a sufficient pathCap contribution for one pair.
 * With paths the fill keeps ONE traceback byte per cell instead of the fp64 cell wherever the machine's family can (small and
 * tiled families always; one-tape family when the fp64 matrices would take a quarter of the memory budget, option MB_ONETAPE_TB);
 * scores and paths are the reference's either way (first maximum in its enumeration order, src/dpmatrix.defs.h:93-103,171-174). */
int64_t mb_viterbi_path_bound(const mb_machine *m, int64_t inLen, int64_t outLen);
int mb_batch_viterbi(mb_batch *b, double *loglike, int64_t *pathOff, uint32_t *pathEdges, int64_t pathCap);

/* MachineCounts(eval, seqPairList): E-step                        src/counts.cpp:37-64, src/backward.cpp:58-87
 * counts[nTrans] += posterior expected usage of every transition, summed over the batch;
 * *loglikeSum += sum of forward.logLike() (MachineCounts::loglike); loglike[nPairs] optional (may be NULL).
 * Pairs with a -inf likelihood contribute nothing to counts (the reference would produce NaN there).
 * The reference's loop is serial and reproduces bit for bit; here the order of some additions follows the scheduling (counts agree
 * to ~1e-10 from run to run).  Option MB_DETERMINISTIC=1 (mb_set_option or the environment, read when the call begins) puts every
 * such accumulator into 64-bit fixed point: repeated calls return identical counts, below 6.7e7 per transition and call.  A count in [6.7e7, 2.7e8) makes the call FAIL (every conversion saturates at 2^62, the host
 * checks the accumulators); the check is NOT airtight beyond that -- a 64-bit accumulator that several saturated terms push past 2^64
 * wraps, and a true count of 2.7e8 or more per transition and call may come back small with rc = 0: keep a call's batch below 2.7e8
 * expected uses of any one transition (2.7e8 emitted symbols), or use the floating-point mode. */
int mb_batch_counts(mb_batch *b, double *counts, double *loglikeSum, double *loglike);

/* One full matrix back to the host, for DPMatrix::cell()/writeJson() (src/dpmatrix.defs.h:39-53), the golden
 * matrix tests (t/src/testforward.cpp, testbackward.cpp) and Machine::downsample (src/machine.cpp:2053-2076).
 * mode MB_FORWARD uses startState (ForwardMatrix 4-argument ctor, src/forward.h:24); Viterbi seeds state 0
 * (src/viterbi.cpp:30); Backward seeds the last state (src/backward.cpp:33).
 * cellsOut[(inLen+1)*(outLen+1)*nStates]. */
int mb_fill(mb_machine *m, int mode, const int32_t *in, int64_t inLen, const int32_t *out, int64_t outLen,
            int32_t startState, double *cellsOut);

/* mb_fill with an envelope (envStart/envEnd: outLen+1 entries each, or both NULL for the full envelope). */
int mb_fill_env(mb_machine *m, int mode, const int32_t *in, int64_t inLen, const int32_t *out, int64_t outLen,
                int32_t startState, const int32_t *envStart, const int32_t *envEnd, double *cellsOut);

/* ---- profile tapes: a machine with an empty input tape against soft output sequences -------------------------------------
 * `--recognize-csv` (target/boss.cpp:606-611, src/csv.cpp:8-18): the semantics of compose(M, transpose(CSVProfile::machine()))
 * scored with empty tapes (src/machine.cpp:794-850, 1053-1085), swept natively over the (rows + 1) x 2 x nStates lattice
 * (docs/profile_tapes.md).  Profile k = rows rowOff[k]..rowOff[k+1); row r = logP[r*(nOutTok+1) ...], column 0 = the blank (the
 * row is consumed, the machine does not move), column t = the log weight of output token t; -inf allowed, NaN / +inf rejected.
 * Transitions that read input never fire.  Viterbi keeps the first maximum: the blank first, then emitting edges in `incoming`
 * order; after the silent moves, "no move" first, then silent edges in `incoming` order.  Paths are the machine's global edge
 * ids, start -> end, with the row at which each edge fired (pathRow may be NULL); a profile whose score is -inf gets an empty
 * path.  Counts follow mb_batch_counts (a -inf profile adds nothing) and are the same bits from call to call in either mode of
 * MB_DETERMINISTIC.  Materialised lattices: cells[((row*2) + layer)*nStates + state], layer 0 = arrived at the row, layer 1 =
 * after the silent moves; mb_profile_fill: cellsOut[(nRows+1)*2*nStates], mode MB_FORWARD / MB_VITERBI / MB_BACKWARD. */
typedef struct mb_profiles mb_profiles;
mb_profiles *mb_profiles_create(mb_machine *m, int64_t nProfiles, const double *logP, const int64_t *rowOff);
void mb_profiles_destroy(mb_profiles *p);
int mb_profiles_forward(mb_profiles *p, int flags /* MB_ROLLING | MB_MATERIALISE */, double *loglike);
int64_t mb_profile_path_bound(const mb_machine *m, int64_t nRows);
int mb_profiles_viterbi(mb_profiles *p, double *loglike, int64_t *pathOff, uint32_t *pathEdges,
                        int32_t *pathRow /* row at which each edge fired */, int64_t pathCap);
int mb_profiles_counts(mb_profiles *p, double *counts, double *loglikeSum, double *loglike);
int mb_profile_fill(mb_machine *m, int mode, const double *logP, int64_t nRows, double *cellsOut);

/* CTC-merged profiles (`--recognize-merge-csv`, src/csv.cpp:20-46): the semantics of compose(M, transpose(CSVProfile::mergingMachine()))
 * with empty tapes -- a column repeated in consecutive rows is one symbol, and only a blank separates two equal symbols -- swept
 * natively over (rows + 1) x 2 x (nCols + 1) planes x nStates (docs/profile_tapes.md, "Merged (CTC) profiles").  Row r =
 * logP[r*(nCols+1) ...]: column 0 the blank, column c = 1..nCols the log weight of a CSV column whose output token is colTok[c-1]
 * (1..nOutTok; two columns may share a token and stay two columns).  One column map per batch.  Plane 0 = the last row took the
 * blank (or no row yet), plane c = the last row took column c.  mb_profiles_forward / _viterbi / _counts / _destroy and
 * mb_profile_path_bound work on the returned object unchanged; blank and repeat rows are not path edges.  Viterbi keeps the first
 * maximum: after the silent moves "no move", then silent edges in `incoming` order; into plane 0 the planes ascending; into plane c
 * the repeat, then the emitting edges of colTok[c-1] in `incoming` order, each from the lowest plane k != c attaining its maximum; at
 * the end the planes ascending.  Materialised lattices: cells[(((row*2) + layer)*(nCols+1) + plane)*nStates + state];
 * mb_profile_fill_merged: cellsOut[(nRows+1)*2*(nCols+1)*nStates].  nCols < 1, a token outside 1..nOutTok, NaN / +inf: an error. */
mb_profiles *mb_profiles_create_merged(mb_machine *m, int64_t nProfiles, const double *logP, const int64_t *rowOff,
                                       int32_t nCols, const int32_t *colTok);
int mb_profile_fill_merged(mb_machine *m, int mode, const double *logP, int64_t nRows, int32_t nCols, const int32_t *colTok,
                           double *cellsOut);

/* Row posteriors of one-tape profiles, plain and merged (docs/profile_tapes.md, "Row posteriors of one-tape profiles"):
 * post[(rowOff[k] - rowOff[0] + r)*width + x], width = nOutTok + 1 (plain) or nCols + 1 (merged), = the posterior probability that
 * row r of profile k was consumed as column x (0: the blank), which is the gradient of the profile's log-likelihood in logP at that
 * entry.  For merged profiles column c holds both ways a row takes it: repeating the previous row's column and a fresh emission of
 * colTok[c-1]; with a linear-chain generator the likelihood is minus the CTC loss and post its gradient in the frames.  post has the
 * layout of the row table and is overwritten.  Every row of a profile with a finite likelihood sums to 1; a profile whose likelihood
 * is -inf gets zeros, an entry whose weight is -inf is exactly 0, and the column sums of a plain profile are the mb_profiles_counts
 * of the transitions that write the column's token, added up.  The call runs the materialised Forward and Backward sweeps and one
 * flat kernel over all rows (k_profile_rowpost); it chunks under the memory budget by two lattices per profile, and one profile whose
 * two lattices exceed the budget is an error before anything is launched.  With MB_DETERMINISTIC=1 the sums go through 64-bit fixed
 * point at 2^-36 and are the same bits from call to call, alone or in a batch, chunked or not.  mb_profiles_set_rows replaces the
 * whole row table (same shapes, checked as mb_profiles_create / _create_merged check it; a refused table leaves the old one in
 * effect) and launches nothing: a training loop re-uses the object. */
int mb_profiles_row_posteriors(mb_profiles *p, double *post /* [sum rows][width], overwritten */, double *loglike /* [nProfiles] or NULL */);
int mb_profiles_set_rows(mb_profiles *p, const double *logP);

/* Pairs: a known input sequence against a profile (`--recognize-csv` beside --input-chars / --input-fasta / --input-json): the
 * semantics of compose(M, transpose(CSVProfile::machine())) on input x[1..I] with an empty output, for a machine WITH an input
 * alphabet, swept natively over (I + 1) x (rows + 1) x 2 x nStates along anti-diagonals (docs/profile_tapes.md, "Pairs: an input
 * sequence against a profile").  Pair k = input tokens inTok[inOff[k]..inOff[k+1]) (1..nInTok) and rows rowOff[k]..rowOff[k+1) of
 * logP (rows as mb_profiles_create).  Layer 0 (N) = arrived at (i, row), where alone the blank may fire; layer 1 (W) = after the
 * machine's output-less moves there (input-only edges from (i-1, row), then the silent levels).  Viterbi keeps the first maximum:
 * into N the blank, then the match edges (in = x_i, an output) in `incoming` order, then the output-only edges in `incoming` order;
 * into W "no move", then the input-only edges, then the silent edges, each in `incoming` order.  Paths are the machine's global edge
 * ids, start -> end; pathRow (may be NULL) is the row an emitting edge consumed, for an output-less edge the number of rows consumed
 * before it; the input position follows by counting the input-consuming edges.  A pair whose score is -inf gets an empty path and
 * adds nothing to the counts; blank rows are not edges.  pathCap must hold the sum of mb_profile_pair_path_bound over the pairs
 * (I + L + (I + L + 1) * (silent levels)).  Counts with MB_DETERMINISTIC=1 go through 64-bit fixed point and are the same bits from
 * call to call.  Materialised lattices: cells[(((i*(nRows+1)) + row)*2 + layer)*nStates + state]; mb_profile_pair_fill:
 * cellsOut[(nIn+1)*(nRows+1)*2*nStates], mode MB_FORWARD / MB_VITERBI / MB_BACKWARD (Backward: layer 0 = from the arrived stage).
 * Errors, before anything is launched: a token outside 1..nInTok (any token, for a machine without inputs), NaN / +inf weights, a
 * pathCap below the bound, a lattice beyond the memory budget on its own.  An input the machine cannot read scores -inf. */
typedef struct mb_profile_pairs mb_profile_pairs;
mb_profile_pairs *mb_profile_pairs_create(mb_machine *m, int64_t nPairs, const int32_t *inTok, const int64_t *inOff,
                                          const double *logP, const int64_t *rowOff);
void mb_profile_pairs_destroy(mb_profile_pairs *p);
int mb_profile_pairs_forward(mb_profile_pairs *p, int flags /* MB_ROLLING | MB_MATERIALISE */, double *loglike);
int64_t mb_profile_pair_path_bound(const mb_machine *m, int64_t nIn, int64_t nRows);
int mb_profile_pairs_viterbi(mb_profile_pairs *p, double *loglike, int64_t *pathOff, uint32_t *pathEdges, int32_t *pathRow,
                             int64_t pathCap);
int mb_profile_pairs_counts(mb_profile_pairs *p, double *counts, double *loglikeSum, double *loglike);
int mb_profile_pair_fill(mb_machine *m, int mode, const int32_t *inTok, int64_t nIn, const double *logP, int64_t nRows,
                         double *cellsOut);

/* Pairs under an envelope (docs/profile_tapes.md, "Pairs under an envelope"): per row r = 0..rows the half-open interval
 * [inStart[r], inEnd[r]) of input positions whose cells exist, both layers of every other cell -inf -- Envelope::inStart / inEnd in
 * the orientation of mb_batch_set_envelopes.  Pair k owns rows envOff[k]..envOff[k+1]: rows_k + 1 of them, or none (full: the pair
 * runs the sweeps above, in a launch of their own when the batch holds both kinds).  envOff == NULL clears every envelope.  The
 * sweeps visit the envelope cells alone; materialised lattices are compact, cells[((off[r] + i - inStart[r])*2 + layer)*nStates +
 * state] with off[r] the cells of the rows before r, and mb_profile_pairs_cells is the doubles of all of them (the memory budget
 * chunks by it).  mb_profile_pair_fill_env hands back the full rectangle of mb_profile_pair_fill with -inf outside; both pointers
 * NULL = no envelope.  Errors, before anything is launched (the pairs are then left without envelopes): "Envelope/sequence mismatch"
 * (a row count other than rows + 1, inEnd > nIn + 1, inStart < 0 or > inEnd), "Envelope is not connected" (the rule of
 * Envelope::connected; (0, 0) and (nIn, rows) lie inside), "Envelope is not monotone" (inStart or inEnd decreases from a row to the
 * next), "envelopes take plain profiles" (a merged pairs object: its entry is mb_profile_pairs_set_envelopes_merged, below). */
int mb_profile_pairs_set_envelopes(mb_profile_pairs *p, const int64_t *envOff, const int32_t *inStart, const int32_t *inEnd);
int mb_profile_pair_fill_env(mb_machine *m, int mode, const int32_t *inTok, int64_t nIn, const double *logP, int64_t nRows,
                             const int32_t *envStart, const int32_t *envEnd, double *cellsOut);
int64_t mb_profile_pairs_cells(const mb_profile_pairs *p);   /* doubles of all materialised lattices under the current envelopes */

/* Row posteriors of the pairs (docs/profile_tapes.md, "Row posteriors"): post[(rowOff[k] - rowOff[0] + r)*(nOutTok+1) + o] = the
 * posterior probability that row r of pair k's profile was consumed as output token o (column 0: as the blank), which is the
 * gradient of the pair's log-likelihood in logP at that entry.  post has the layout of the row table and is overwritten.  Every row
 * of a pair with a finite likelihood sums to 1; a pair whose likelihood is -inf gets zeros, an entry whose weight is -inf is exactly
 * 0, and the column sums of a pair are the mb_profile_pairs_counts of the transitions that write the column's token, added up.
 * Pairs under an envelope are summed over its cells.  With MB_DETERMINISTIC=1 the sums go through 64-bit fixed point at 2^-36 and
 * are the same bits from call to call, alone or in a batch, chunked or not.  mb_profile_pairs_set_rows replaces the whole row table
 * (same shapes, checked as mb_profile_pairs_create checks it; a refused table leaves the old one in effect), launches nothing and
 * leaves the envelopes in place: a training loop re-uses the object.  Both refuse a merged pairs object before anything is launched:
 * "row posteriors take plain profiles". */
int mb_profile_pairs_row_posteriors(mb_profile_pairs *p, double *post /* [sum rows][nOutTok+1], overwritten */,
                                    double *loglike /* [nPairs] or NULL */);
int mb_profile_pairs_set_rows(mb_profile_pairs *p, const double *logP);

/* Posterior path samples of the pairs (docs/profile_tapes.md, "Posterior path samples"): nSamples alignments per pair, each drawn with
 * its posterior probability by a stochastic traceback over the pair's materialised Forward lattice, on the device -- the reference's
 * ForwardMatrix::samplePath, without the lattice crossing to the host.  Path k * nSamples + j is sample j of pair k, in the format of
 * mb_profile_pairs_viterbi (global edge ids start -> end, pathRow as there, may be NULL; blank rows are not edges);
 * pathLogProb[k * nSamples + j] (may be NULL) is the log posterior probability of that path: its own log weight minus loglike[k].  From
 * W[I][L][S-1] back to N[0][0][0] every visit of a W cell, or of an N cell with row > 0, is one decision among the terms of the fill in
 * the fill's order (the Viterbi candidate order above): p_c = exp(term_c - cell), the first c whose running sum exceeds u, else the
 * last c with p_c > 0.  The uniform u of decision t of sample j of pair k is Philox4x32-10 with key (seed & 0xffffffff, seed >> 32)
 * and counter (t, j, k & 0xffffffff, k >> 32), u = ((x0 >> 5) * 2^26 + (x1 >> 6)) * 2^-53: a sample depends on nothing but (seed,
 * k, j), not on chunking, the pairs beside it or nSamples.  A pair whose likelihood is -inf gets empty paths and -inf.  Pairs under
 * an envelope are sampled over its cells.  The call runs one materialised Forward sweep and one sample launch per kind of pair and
 * chunk; it chunks under the memory budget by a pair's lattice plus nSamples * (8 * bound + 16) bytes.  Errors, before anything is
 * launched: nSamples < 1, NULL pathOff or pathEdges, a pathCap below nSamples times the sum of mb_profile_pair_path_bound over the
 * pairs, a merged pairs object ("sampling takes plain profiles"), more than 2^31 - 1 (pair, sample) lanes in one chunk, a pair beyond
 * the memory budget on its own. */
int mb_profile_pairs_sample(mb_profile_pairs *p, int64_t nSamples, uint64_t seed, double *loglike /* [nPairs] or NULL */,
                            int64_t *pathOff /* [nPairs*nSamples + 1] */, uint32_t *pathEdges, int32_t *pathRow,
                            double *pathLogProb /* [nPairs*nSamples] or NULL */, int64_t pathCap);

/* Pairs against CTC-merged profiles: a known input sequence against the rows of `--recognize-merge-csv` -- the semantics of
 * compose(M, transpose(CSVProfile::mergingMachine())) on input x[1..I] with an empty output, swept natively over
 * (I + 1) x (rows + 1) x 2 x (nCols + 1) x nStates along anti-diagonals (mb_profile_pair_merge.hip; docs/profile_tapes.md, "Pairs
 * against a merged profile").  Rows hold nCols + 1 doubles and the batch has one column map, as mb_profiles_create_merged; plane 0 =
 * the last row took the blank (or no row yet), plane c = the last row took column c.  mb_profile_pairs_forward / _viterbi / _counts /
 * _destroy and mb_profile_pair_path_bound work on the merged object unchanged.  Viterbi keeps the first maximum: into N[..][0] the
 * planes ascending; into N[..][c] the repeat, then the match edges, then the output-only edges of colTok[c] in `incoming` order, each
 * from the lowest plane other than c that attains its exclusion vector; into W "no move", then the input-only edges, then the silent
 * edges; at the end the planes ascending.  Blank and repeat rows are not edges.  Materialised lattices:
 * cells[((((i*(nRows+1)) + row)*2 + layer)*(nCols+1) + plane)*nStates + state]; mb_profile_pair_fill_merged:
 * cellsOut[(nIn+1)*(nRows+1)*2*(nCols+1)*nStates].  Errors, before anything is launched: nCols < 1, a colTok outside 1..nOutTok, an
 * input token outside 1..nInTok, NaN / +inf weights, a pathCap below the bound, a lattice beyond the memory budget on its own. */
mb_profile_pairs *mb_profile_pairs_create_merged(mb_machine *m, int64_t nPairs, const int32_t *inTok, const int64_t *inOff,
                                                 const double *logP, const int64_t *rowOff, int32_t nCols, const int32_t *colTok);
int mb_profile_pair_fill_merged(mb_machine *m, int mode, const int32_t *inTok, int64_t nIn, const double *logP, int64_t nRows,
                                int32_t nCols, const int32_t *colTok, double *cellsOut);

/* Row posteriors of pairs against merged profiles (k_profile_pair_merge_rowpost; docs/profile_tapes.md, "Row posteriors of pairs
 * against a merged profile"): post[(rowOff[k] - rowOff[0] + r)*(nCols+1) + c] = the posterior probability that row r of pair k was
 * consumed as column c (column 0: as the blank) -- the blank out of every plane, the repeat of column c, and the match and
 * output-only edges that write colTok[c] out of every plane other than c -- which is the gradient of the pair's log-likelihood in
 * logP at that entry.  Every row of a pair with a finite likelihood sums to 1; a pair whose likelihood is -inf gets zeros and an
 * entry whose weight is -inf is exactly 0; post less the repeats, summed over rows and over the columns of a token, is the
 * mb_profile_pairs_counts of the transitions that write that token.  MB_DETERMINISTIC=1 as mb_profile_pairs_row_posteriors.
 * mb_profile_pairs_set_rows_merged replaces the whole row table (same shapes, checked as create checks it; a refused table leaves
 * the old one in effect) and launches nothing.  Both refuse a plain pairs object before anything is launched: "merged row
 * posteriors take merged profiles"; a pair whose lattices exceed the memory budget on its own is the error of
 * mb_profile_pairs_counts. */
int mb_profile_pairs_row_posteriors_merged(mb_profile_pairs *p, double *post /* [sum rows][nCols+1], overwritten */,
                                           double *loglike /* [nPairs] or NULL */);
int mb_profile_pairs_set_rows_merged(mb_profile_pairs *p, const double *logP);

/* Pairs against merged profiles under an envelope (docs/profile_tapes.md, "Pairs against a merged profile under an envelope"): the
 * envelopes of mb_profile_pairs_set_envelopes -- same arguments, same checks, same three messages -- on a merged pairs object.  Cell
 * (i, r) exists iff inStart[r] <= i < inEnd[r], in every plane; N, W and the exclusion vectors of every other cell are -inf.  A pair
 * without an envelope runs the kernels of the rectangle, in a launch of their own when the batch holds both kinds.  Materialised
 * lattices are compact, cells[(((off[r] + i - inStart[r])*2 + layer)*(nCols+1) + plane)*nStates + state], and
 * mb_profile_pairs_cells counts them.  mb_profile_pairs_forward / _viterbi / _counts / _row_posteriors_merged then sweep the envelope
 * cells alone; mb_profile_pairs_set_rows_merged leaves the envelopes in place.  envOff == NULL clears.  A plain pairs object is
 * refused with "merged envelopes take merged profiles"; a rejected call leaves the pairs without envelopes and launches nothing.
 * (mb_profile_pairs_set_envelopes keeps refusing a merged object.)  mb_profile_pair_fill_merged_env hands back the full rectangle of
 * mb_profile_pair_fill_merged with -inf outside; both envelope pointers NULL = no envelope. */
int mb_profile_pairs_set_envelopes_merged(mb_profile_pairs *p, const int64_t *envOff, const int32_t *inStart, const int32_t *inEnd);
int mb_profile_pair_fill_merged_env(mb_machine *m, int mode, const int32_t *inTok, int64_t nIn, const double *logP, int64_t nRows,
                                    int32_t nCols, const int32_t *colTok, const int32_t *envStart, const int32_t *envEnd,
                                    double *cellsOut);

/* Posterior path samples of pairs against merged profiles (docs/profile_tapes.md, "Posterior path samples of pairs against a merged
 * profile"): mb_profile_pairs_sample for a merged pairs object, with or without envelopes.  A sample is a LATTICE path: its edges in
 * the format of mb_profile_pairs_viterbi and the column every row took, rowCol[(rowOff[k] - rowOff[0]) * nSamples + j * L_k + r] for
 * row r of sample j of pair k (0: the blank; c: column c, fresh or repeated; may be NULL) -- the edge list alone does not say whether
 * a row no edge consumed was a blank or a repeat.  pathLogProb is the log weight of that lattice path (its edges plus P[r][rowCol[r]]
 * of every row) minus loglike[k].  Decision 0 picks the end plane among W[I][L][.][S-1], planes ascending, against loglike; then at a
 * W cell: N ("stay"), the input-only edges, the silent edges, on the cell's plane; at N[.][r][0]: the blank out of every plane
 * ascending; at N[.][r][c]: the repeat, then the match and then the output-only edges of colTok[c] in `incoming` order, every edge
 * once per source plane k != c ascending.  The draw rule and the uniforms are those of mb_profile_pairs_sample: a sample depends on
 * nothing but (seed, k, j).  A pair whose likelihood is -inf gets empty paths, -inf and rowCol = -1 in every row.  The call runs one
 * materialised Forward sweep and one sample launch per kind of pair and chunk; it chunks under the memory budget by a pair's lattice
 * (and the ring of its fill, where that lives in global memory) plus nSamples * (8 * bound + 16 + 4 * rows) bytes.  Errors, before
 * anything is launched: nSamples < 1, NULL pathOff or pathEdges, a pathCap below nSamples times the sum of
 * mb_profile_pair_path_bound over the pairs, a plain pairs object ("merged sampling takes merged profiles"), more than 2^31 - 1
 * (pair, sample) lanes in one chunk, a pair beyond the memory budget on its own.  (mb_profile_pairs_sample keeps refusing a merged
 * object.) */
int mb_profile_pairs_sample_merged(mb_profile_pairs *p, int64_t nSamples, uint64_t seed, double *loglike /* [nPairs] or NULL */,
                                   int64_t *pathOff /* [nPairs*nSamples + 1] */, uint32_t *pathEdges, int32_t *pathRow /* or NULL */,
                                   int32_t *rowCol /* [nSamples * sum rows] or NULL */, double *pathLogProb /* [nPairs*nSamples] or NULL */,
                                   int64_t pathCap);

/* Pairs of profiles (`--generate-csv A.csv` beside `--recognize-csv B.csv`): a machine WITH an input alphabet between an input
 * profile and an output profile -- the semantics of compose(A.machine(), compose(M, transpose(B.machine()))) with both tapes empty,
 * swept natively over (K + 1) x (rows + 1) x 3 x nStates along anti-diagonals (mb_profile_two.hip; docs/profile_tapes.md, "Pairs
 * of profiles").  Pair k = rows inOff[k]..inOff[k+1) of logA (rows of nInTok + 1 doubles, column 0 = the blank, column a = input
 * token a) and rows rowOff[k]..rowOff[k+1) of logB (rows as mb_profiles_create).  Layer 0 (N) = arrived at (i, row), where alone
 * the output blank may fire; layer 1 (W) = after the machine's output-less moves there; layer 2 (Z) = committed to wait for the next
 * input row, where alone the input blank may fire and from which alone the input-reading edges leave.  Viterbi keeps the first
 * maximum: into N the output blank, then the match edges, then the output-only edges; into W "no move", then the input-only edges,
 * then the silent edges; into Z "W", then the input blank; edges of a kind in `incoming` order (input token ascending, then output
 * token).  Paths are the machine's global edge ids, start -> end; pathRow (may be NULL) is the output row an emitting edge
 * consumed, for an output-less edge the number of output rows consumed before it; pathInRow (may be NULL) is the same on the input
 * tape -- input blanks advance it without an edge.  A pair whose score is -inf gets an empty path and adds nothing to the counts;
 * blanks on either tape are not edges.  pathCap must hold the sum of mb_profile_pair_path_bound(m, K, rows) over the pairs.  Counts
 * with MB_DETERMINISTIC=1 go through 64-bit fixed point and are the same bits from call to call.  Materialised lattices:
 * cells[(((i*(nRows+1)) + row)*3 + layer)*nStates + state]; mb_profile_two_fill: cellsOut[(nIn+1)*(nRows+1)*3*nStates], mode
 * MB_FORWARD / MB_VITERBI / MB_BACKWARD (Backward: layer 0 = from the arrived stage, 2 = from the committed stage).  Envelopes and
 * the CTC-merged form are below.  Errors, before anything is launched: "two-profile sweeps need a machine with an input
 * alphabet", NaN / +inf weights in either table, a pathCap below the bound, a lattice beyond the memory budget on its own. */
typedef struct mb_profile_twos mb_profile_twos;
mb_profile_twos *mb_profile_twos_create(mb_machine *m, int64_t nPairs, const double *logA, const int64_t *inOff, const double *logB,
                                        const int64_t *rowOff);
void mb_profile_twos_destroy(mb_profile_twos *p);
int mb_profile_twos_forward(mb_profile_twos *p, int flags /* MB_ROLLING | MB_MATERIALISE */, double *loglike);
int mb_profile_twos_viterbi(mb_profile_twos *p, double *loglike, int64_t *pathOff, uint32_t *pathEdges, int32_t *pathRow,
                            int32_t *pathInRow, int64_t pathCap);
int mb_profile_twos_counts(mb_profile_twos *p, double *counts, double *loglikeSum, double *loglike);
int mb_profile_two_fill(mb_machine *m, int mode, const double *logA, int64_t nIn, const double *logB, int64_t nRows, double *cellsOut);

/* Row posteriors of the pairs of profiles (docs/profile_tapes.md, "Row posteriors of pairs of profiles"):
 * postB[(rowOff[k] - rowOff[0] + r)*(nOutTok+1) + o] = the posterior probability that output row r of pair k was consumed as output
 * token o, postA[(inOff[k] - inOff[0] + i)*(nInTok+1) + a] = that input row i was consumed as input token a (column 0 of either: as
 * its blank) -- the gradients of the pair's log-likelihood in logB and in logA at those entries.  Either table has the layout of its
 * row table and is overwritten; either may be NULL, and its kernel is then not launched.  Every row of a pair with a finite
 * likelihood sums to 1; a pair whose likelihood is -inf gets zeros in both tables, an entry whose weight is -inf is exactly 0, and
 * the column sums of a pair are the mb_profile_twos_counts of the transitions that write (postB) or read (postA) the column's token,
 * added up.  With MB_DETERMINISTIC=1 the sums go through 64-bit fixed point at 2^-36 and are the same bits from call to call, alone
 * or in a batch, chunked or not.  mb_profile_twos_set_rows replaces the input row table, the output row table or both (NULL: keep;
 * same shapes, checked as mb_profile_twos_create checks them; a refused table leaves both old tables in effect) and launches
 * nothing: a training loop re-uses the object. */
int mb_profile_twos_row_posteriors(mb_profile_twos *p, double *postA /* [sum K][nInTok+1], may be NULL */,
                                   double *postB /* [sum rows][nOutTok+1], may be NULL */, double *loglike /* [nPairs], may be NULL */);
int mb_profile_twos_set_rows(mb_profile_twos *p, const double *logA /* NULL: keep */, const double *logB /* NULL: keep */);

/* Pairs of profiles under an envelope (docs/profile_tapes.md, "Pairs of profiles under an envelope"): per output row r = 0..rows the
 * half-open interval [inStart[r], inEnd[r]) of INPUT-ROW positions i = 0..K whose cells exist -- the orientation and the contract of
 * mb_profile_pairs_set_envelopes with K for nIn; all three layers (N, W, Z; NB, WB, ZB) of every other cell are -inf, and the input
 * blank Z[i-1][r] -> Z[i][r] is left out when (i-1, r) lies outside.  Pair k owns rows envOff[k]..envOff[k+1]: rows_k + 1 of them, or
 * none; envOff == NULL clears every envelope.  No call mixes geometries: if any pair has an envelope EVERY pair of the object runs
 * through the envelope kernels, a pair that was given none under the full envelope [0, K + 1), whose results are the bits of no
 * envelope; one launch per kernel and chunk, as for a plain object.  Forward (both flags), Viterbi, counts and both tables of the row
 * posteriors visit the envelope cells alone; the tie order, the path format and the path bound are unchanged.  Materialised lattices
 * are compact, cells[((off[r] + i - inStart[r])*3 + layer)*nStates + state] with off[r] the cells of the rows before r;
 * mb_profile_twos_cells is the doubles of all of them (3 nStates sum(inEnd - inStart) per pair; the memory budget chunks by it).
 * mb_profile_two_fill_env hands back the full rectangle of mb_profile_two_fill with -inf outside; both pointers NULL = no envelope.
 * mb_profile_twos_set_rows keeps the envelopes.  Errors, before anything is launched (the pairs are then left without envelopes):
 * "Envelope/sequence mismatch", "Envelope is not connected", "Envelope is not monotone", as mb_profile_pairs_set_envelopes. */
int mb_profile_twos_set_envelopes(mb_profile_twos *p, const int64_t *envOff, const int32_t *inStart, const int32_t *inEnd);
int mb_profile_two_fill_env(mb_machine *m, int mode, const double *logA, int64_t nIn, const double *logB, int64_t nRows,
                            const int32_t *envStart, const int32_t *envEnd, double *cellsOut);
int64_t mb_profile_twos_cells(const mb_profile_twos *p);   /* doubles of all materialised lattices under the current envelopes */

/* Posterior path samples of the pairs of profiles (docs/profile_tapes.md, "Posterior path samples of pairs of profiles"): nSamples
 * alignments per pair, each drawn with its posterior probability by a stochastic traceback over the pair's materialised Forward
 * lattice, on the device.  Path k * nSamples + j is sample j of pair k, in the format of mb_profile_twos_viterbi (global edge ids
 * start -> end, pathRow and pathInRow as there, either may be NULL; blanks on either tape are not edges);
 * pathLogProb[k * nSamples + j] (may be NULL) is the log posterior probability of that path: its own log weight, the blank of every
 * row of either tape that no edge consumed included, minus loglike[k].  From Z[K][rows][S-1] back to N[0][0][0] every visit of a Z
 * cell with i > 0, of a W cell, or of an N cell with row > 0 is one decision among the terms of the fill in the fill's order (the
 * Viterbi candidate order above; a Z cell with i = 0 holds its W and is none): p_c = exp(term_c - cell), the first c whose running
 * sum exceeds u, else the last c with p_c > 0.  A decision takes one counter value however many of its candidates exist.  The
 * uniforms are those of mb_profile_pairs_sample -- Philox4x32-10 under (seed; t, j, k) with k the pair's index in the object --, so
 * a sample depends on nothing but (seed, k, j), not on chunking, the pairs beside it or nSamples.  A pair whose likelihood is -inf
 * gets empty paths and -inf.  Under envelopes the samples are drawn over their cells.  The call runs one materialised Forward sweep
 * and one sample launch per chunk; it chunks under the memory budget by a pair's lattice plus nSamples * (12 * bound + 16) bytes.
 * Errors, before anything is launched: nSamples < 1, NULL pathOff or pathEdges, a pathCap below nSamples times the sum of
 * mb_profile_pair_path_bound over the pairs, a merged object ("sampling takes plain profiles"), more than 2^31 - 1 (pair, sample)
 * lanes in one chunk, a pair beyond the memory budget on its own. */
int mb_profile_twos_sample(mb_profile_twos *p, int64_t nSamples, uint64_t seed, double *loglike /* [nPairs] or NULL */,
                           int64_t *pathOff /* [nPairs*nSamples + 1] */, uint32_t *pathEdges, int32_t *pathRow /* or NULL */,
                           int32_t *pathInRow /* or NULL */, double *pathLogProb /* [nPairs*nSamples] or NULL */, int64_t pathCap);

/* Pairs of profiles against a CTC-merged output profile (mb_profile_two_merge.hip; docs/profile_tapes.md, "Pairs of profiles
 * against a merged profile"): the input profile as above, the output rows those of mb_profiles_create_merged -- logB rows of
 * nCols + 1 doubles, column 0 the blank, column c the CSV column whose output token is colTok[c - 1], one column map per batch
 * (checked as mb_profiles_create_merged checks it).  The semantics are those of
 * compose(A.machine(), compose(M, transpose(mergingMachine()))) with both tapes empty.  mb_profile_twos_forward / _viterbi / _counts
 * / _cells / _destroy and the path cap work on the object unchanged (paths in the two-profile format: edge, output row, input
 * row; blanks of either tape and repeat rows are not edges); mb_profile_twos_set_rows takes logB rows of nCols + 1 doubles.  The
 * lattice of a pair has nCols + 1 planes of the plain one -- cells[((((i*(nRows+1)) + row)*3 + layer)*(nCols+1) + plane)*nStates +
 * state], plane 0 = the last row took the blank (or no row yet), plane c = it took column c; mb_profile_two_fill_merged:
 * cellsOut[(nIn+1)*(nRows+1)*3*(nCols+1)*nStates], mode MB_FORWARD, MB_VITERBI or MB_BACKWARD.  The memory budget chunks by the
 * lattices, the scratch rings of the pairs whose ring does not fit LDS, and the path slots; an anti-diagonal of more than 2^31
 * (cell, plane, state) items is an error at create.  mb_profile_twos_set_envelopes fails on the object with "envelopes take plain
 * profiles" (its entry is mb_profile_twos_set_envelopes_merged, below), mb_profile_twos_row_posteriors with "row posteriors take
 * plain profiles". */
mb_profile_twos *mb_profile_twos_create_merged(mb_machine *m, int64_t nPairs, const double *logA, const int64_t *inOff, const double *logB,
                                               const int64_t *rowOff, int32_t nCols, const int32_t *colTok);
int mb_profile_two_fill_merged(mb_machine *m, int mode, const double *logA, int64_t nIn, const double *logB, int64_t nRows, int32_t nCols,
                               const int32_t *colTok, double *cellsOut);

/* Row posteriors of pairs of profiles against merged profiles (k_profile_two_merge_rowpost; docs/profile_tapes.md, "Row posteriors
 * of pairs of profiles against a merged profile"): postB[(rowOff[k] - rowOff[0] + r)*(nCols+1) + c] = the posterior probability
 * that output row r of pair k was consumed as column c (column 0: as the blank) -- the blank out of every plane, the repeat of
 * column c, and the match and output-only edges that write colTok[c] out of every plane other than c;
 * postA[(inOff[k] - inOff[0] + i)*(nInTok+1) + a] = that input row i was consumed as input token a (column 0: as the input blank)
 * -- the gradients of the pair's log-likelihood in logB and in logA at those entries.  Either table has the layout of its row
 * table and is overwritten; either may be NULL, and its kernel is then not launched.  Every row of a pair with a finite likelihood
 * sums to 1; a pair whose likelihood is -inf gets zeros in both tables and an entry whose weight is -inf is exactly 0; postB less
 * the repeats, summed over rows and over the columns of a token, is the mb_profile_twos_counts of the transitions that write that
 * token, the column sums of postA those of the transitions that read the column's token.  MB_DETERMINISTIC=1 as
 * mb_profile_twos_row_posteriors; mb_profile_twos_set_rows replaces the row tables between calls.  A plain object is refused before
 * anything is launched: "merged row posteriors take merged profiles"; a pair whose lattices exceed the memory budget on its own is
 * the error of mb_profile_twos_counts. */
int mb_profile_twos_row_posteriors_merged(mb_profile_twos *p, double *postA /* [sum K][nInTok+1], may be NULL */,
                                          double *postB /* [sum rows][nCols+1], may be NULL */, double *loglike /* may be NULL */);

/* Pairs of profiles against merged profiles under an envelope (docs/profile_tapes.md, "Pairs of profiles against a merged profile
 * under an envelope"): the envelopes of mb_profile_twos_set_envelopes -- same arguments, same checks, same three messages -- on a
 * merged two-profile object.  Cell (i, r) exists iff inStart[r] <= i < inEnd[r], in every plane; N, W, Z, the exclusion vectors XW
 * and XZ and, in the Backward, NB, WB, ZB, TZ and TW of every other cell are -inf.  No call mixes geometries, as for the plain
 * object: if any pair has an envelope EVERY pair runs the envelope kernels, a pair that was given none under the full envelope,
 * whose results are the bits of no envelope; one launch per kernel and chunk.  Materialised lattices are compact,
 * cells[(((off[r] + i - inStart[r])*3 + layer)*(nCols+1) + plane)*nStates + state], and mb_profile_twos_cells counts them
 * (3 nStates (nCols+1) sum(inEnd - inStart) doubles per pair; the memory budget chunks by it).  mb_profile_twos_forward / _viterbi /
 * _counts / _row_posteriors_merged then sweep the envelope cells alone, with the tie order, the path format and the path bound of
 * the rectangle; mb_profile_twos_set_rows leaves the envelopes in place.  envOff == NULL clears.  A plain object is refused with
 * "merged envelopes take merged profiles"; a rejected call leaves the pairs without envelopes and launches nothing.
 * (mb_profile_twos_set_envelopes keeps refusing a merged object.)  mb_profile_two_fill_merged_env hands back the full rectangle of
 * mb_profile_two_fill_merged with -inf outside in all layers and planes; both envelope pointers NULL = no envelope. */
int mb_profile_twos_set_envelopes_merged(mb_profile_twos *p, const int64_t *envOff, const int32_t *inStart, const int32_t *inEnd);
int mb_profile_two_fill_merged_env(mb_machine *m, int mode, const double *logA, int64_t nIn, const double *logB, int64_t nRows,
                                   int32_t nCols, const int32_t *colTok, const int32_t *envStart, const int32_t *envEnd,
                                   double *cellsOut);

/* ---- prefix search: imputing the input tape (--prefix-decode / --prefix-encode / --random-encode) -------------------------------
 * The node fill of the reference's PrefixTree (src/ctc.cpp:25-88) on the device, the tree and its heap on the host
 * (docs/decoding.md).  An mb_prefix holds nSeq searches (output sequence k = outTok[outOff[k]..outOff[k+1]), tokens 1..nOutTok)
 * and a pool of maxNodes node lattices of (maxOutLen + 1) x 2 x nStates doubles, taken from the library's workspace under the
 * memory budget (mb_set_memory_budget); it never grows: a fill that finds the pool full fails and changes nothing.
 * logSumInTrans is R = log((I - N)^-1), nStates x nStates row-major, N summing exp(w) over the transitions with empty output
 * (EvaluatedMachine::logSumInTrans, src/eval.cpp:146-184); -inf allowed, NaN / +inf rejected.
 * mb_prefix_root fills the root of search `seq`; mb_prefix_extend fills n children in ONE launch: entry i is the child of node
 * parent[i] (a live node of search seq[i]) by input token inTok[i] (1..nInTok).  Both return node handles (slot numbers) and,
 * per node, logSeqProb = log P(x, y) and logPrefixProb = log P(y | an input starting with x).  mb_prefix_release hands slots back.
 * Node lattices: cells[((j*2) + layer)*nStates + state], j = 0..outLen of the node's search, layer 0 = seq, layer 1 = prefix.
 * A fill gives the same bits from call to call. */
typedef struct mb_prefix mb_prefix;
mb_prefix *mb_prefix_create(mb_machine *m, int64_t nSeq, const int32_t *outTok, const int64_t *outOff,
                            const double *logSumInTrans, int64_t maxNodes);
void mb_prefix_destroy(mb_prefix *p);
int mb_prefix_root(mb_prefix *p, int64_t seq, int64_t *nodeOut, double *logSeqProb, double *logPrefixProb);
int mb_prefix_extend(mb_prefix *p, int64_t n, const int64_t *seq, const int64_t *parent, const int32_t *inTok,
                     int64_t *childOut, double *logSeqProb, double *logPrefixProb);
int mb_prefix_release(mb_prefix *p, int64_t n, const int64_t *node);
int64_t mb_prefix_free_nodes(const mb_prefix *p);
int mb_prefix_node_cells(mb_prefix *p, int64_t node, double *cellsOut);
/* The same searches against PROFILES (soft outputs) in place of token strings: search k decodes rows rowOff[k]..rowOff[k+1] of
 * logP, rows of nOutTok + 1 log weights with column 0 the blank (the layout of mb_profiles_create; -inf allowed, NaN / +inf
 * rejected).  The answers are those of the token search on compose(machine, profile recogniser) with an empty output, swept
 * natively over the profile's rows (docs/decoding.md).  Every other mb_prefix_* call works on the returned object unchanged;
 * a node's lattice is cells[((r*2) + layer)*nStates + state], r = 0..rows, layer 0 = Forward, layer 1 = prefix. */
mb_prefix *mb_prefix_create_profiles(mb_machine *m, int64_t nProfiles, const double *logP, const int64_t *rowOff,
                                     const double *logSumInTrans, int64_t maxNodes);
/* The same against CTC-MERGED profiles (the layout of mb_profiles_create_merged): rows of nCols + 1 log weights, column 0 the
 * blank, column c the CSV column whose output token is colTok[c - 1] (1..nOutTok); a batch has one column map.  The answers are
 * those of the token search on compose(machine, merging recogniser) with an empty output.  A node's lattice has nCols + 1 planes:
 * cells[(((r*2) + layer)*(nCols+1) + plane)*nStates + state], plane 0 = the last row took the blank (or no row yet), plane c = it
 * took column c; a slot is 2 (maxRows + 1)(nCols + 1) nStates doubles, which mb_prefix_node_cells copies.  Errors: nCols < 1, a
 * token outside 1..nOutTok, NaN / +inf, a pool over the memory budget, and a machine whose working set
 * ((6 nCols + 5) nStates + nCols + 1 doubles) exceeds the 160 KiB of LDS of a workgroup. */
mb_prefix *mb_prefix_create_merged(mb_machine *m, int64_t nProfiles, const double *logP, const int64_t *rowOff, int32_t nCols,
                                   const int32_t *colTok, const double *logSumInTrans, int64_t maxNodes);

/* ---- convenience wrappers over host buffers (create batch, run, destroy) ----------------------------------
 * forwardLogLike / viterbiLogLike+viterbiAlign / forwardBackwardCounts of src/api.h:20-34.                   */
int mb_forward_batch(mb_machine *m, int64_t nPairs, const int32_t *inTok, const int64_t *inOff,
                     const int32_t *outTok, const int64_t *outOff, int flags, double *loglike);
int mb_viterbi_batch(mb_machine *m, int64_t nPairs, const int32_t *inTok, const int64_t *inOff,
                     const int32_t *outTok, const int64_t *outOff, double *loglike, int64_t *pathOff,
                     uint32_t *pathEdges, int64_t pathCap);
int mb_counts_batch(mb_machine *m, int64_t nPairs, const int32_t *inTok, const int64_t *inOff,
                    const int32_t *outTok, const int64_t *outOff, double *counts, double *loglikeSum,
                    double *loglike);

/* ---- multi-GPU: the one exchange step of the path ---------------------------------------------------------------
 * Pairs are independent, so a sharded pair list needs no collective for --loglike / --viterbi / --align.  For
 * --counts / --train the per-rank MachineCounts are summed (MachineCounts::operator+=, src/counts.cpp:66-71): ONE
 * all-reduce of nTransitions + 1 doubles per EM iteration over RCCL (xGMI).  The communicator is bootstrapped by the
 * host: rank 0 calls mb_comm_unique_id and ships the 128 bytes to the other ranks by its own means, every rank calls
 * mb_comm_init (after mb_set_device).  comm == NULL (single process) makes mb_allreduce_counts a no-op.  RCCL is
 * opened on first use; a caller that never shards never needs it. */
typedef struct mb_comm mb_comm;
int mb_comm_unique_id(char id[128]);
mb_comm *mb_comm_init(const char id[128], int nRanks, int rank);
void mb_comm_destroy(mb_comm *comm);
int mb_allreduce_counts(mb_comm *comm, double *counts, size_t n, double *loglike);   /* in place; loglike may be NULL */

/* ---- host-side log-space helpers (src/logsumexp.h:72-172) -----------------------------------------------------------------
 * The helpers of logsumexp.h that code outside the DP fills uses (fitting, prefix/beam decoders, tests).  Pure host
 * arithmetic with the reference's table semantics (100 001-entry table of log(1+exp(-x)), step 1e-4, linear interpolation,
 * 0 beyond 10 nats), bit for bit; machineboss_amd/cxx/mb_logsumexp.hpp wraps them under the reference's names. */
double mb_log_sum_exp(double a, double b);                                          /* log_sum_exp(a,b), :72-90        */
double mb_log_sum_exp_n(const double *v, size_t n);                                 /* log_sum_exp(vguard<double>), :109 */
double mb_log_inner_product(const double *v1, const double *v2, const double *v3 /* or NULL */, size_t n);   /* :143-155 */

/* ---- tuning / introspection (not part of the reference surface) ------------------------------------------ */
/* Select the kernel family: 0 = auto, 1 = generic (any machine), 2 = small-S lanes=cells, 3 = medium-S
 * lanes=states.  Used by tests to cross-check kernels against each other and by bench.py. */
int mb_set_kernel(int which);
/* Bytes of device memory the library may use for DP matrices (default: 80 % of free HBM). */
int mb_set_memory_budget(size_t bytes);
size_t mb_memory_budget(void);   /* what the pools of one call may take now: the explicit budget, else a share of the device (0: no device) */
/* The library keeps its matrix pools allocated between calls (grow-only); this frees them. */
int mb_release_workspace(void);
/* What the matrix pools cost this process so far: device allocations and releases of pool slots, slots evicted to make room,
 * bytes allocated in all, and the wall-clock milliseconds spent inside hipMalloc / hipFree for them.  Steady-state calls do none
 * (the pools are grow-only and the budget that sizes chunks is sticky); a caller that sees these move between two like calls is
 * paying seconds per call for memory, not for kernels.  Any pointer may be NULL. */
int mb_alloc_stats(int64_t *poolAllocs, int64_t *poolFrees, int64_t *evictions, uint64_t *bytesAllocated, double *ms);
/* Run-time compilation (hiprtc) done by this process so far: wall-clock milliseconds, compiles, and code objects taken
 * from the on-disk cache instead ($MB_JIT_CACHE_DIR, default ~/.cache/mbhip; MB_JIT_CACHE=0 disables it). */
int mb_jit_stats(double *compileMs, int64_t *compiles, int64_t *cacheHits);
/* Transcendental instructions the log-sum-exp Forward sweep of this machine issues per lattice CELL (v_exp_f32, v_log_f32,
 * padding lanes of the kernel family included) -- what the rolling (log-likelihood-only) mode is priced against, since it
 * moves no matrix through HBM.  family: name of the kernel family that would run the sweep. */
int mb_machine_sweep_ops(mb_machine *m, double *expPerCell, double *logPerCell, const char **family);
/* Tuning knobs (kernel family thresholds, strip geometry, closure stages ...: DESIGN.md section 4.7).  They are read when
 * a machine's programs and kernels are built, from the process environment; these calls are the same switchboard for a
 * host that prefers calls: a table inside the library, consulted before the environment.  Value NULL or "" takes the
 * entry out of that table again (back to the environment's value, or the default).  A name the library does not know, or
 * a read-only one, is refused: mb_set_option returns non-zero and mb_last_error names the option; mb_get_option returns
 * NULL for it.  mb_get_option(NULL) returns the list of all options, one per line: name, kind (Int, Real, Text, Present),
 * default (or "by call", or "-"), class and a note, separated by tabs. */
int mb_set_option(const char *name, const char *value);
const char *mb_get_option(const char *name);

/* Writes the HIP source the run-time code generator produces for this machine (mode MB_FORWARD = sum semiring,
 * MB_VITERBI = max, 3 = Forward fused with posterior counts, 4 = max keeping one traceback byte per cell; + 16 = the tile
 * kernel that keeps no matrix (implied by 4); backward and closure (0 = levelled, K >= 1 = silent closure in
 * K stages) select the program; G = columns per
 * wavefront, 1 ... 64) to `path`.  mode + 32 writes the PROGRAM instead of the source, as the kernels read it: 16 int32 (magic
 * 0x4D454431, S, Spad, LPG, G, chunks, nIn, nOut, seedOff, dummyOff, records, usage slots, backward, closure, counting, flat),
 * chunks x 8 int32 descriptors, records of 16 bytes (fp64 weight, srcOff, dstOff), usage slots (int32 table, int32 first
 * record), one int32 per record (the transition it stands for, -1 padding) -- tests/test_tiled_plan.py replays it against the oracle.  Host only: works without a GPU, so the generated kernel
 * can be inspected / cross-compiled offline. */
int mb_debug_jit_source(int32_t nStates, int32_t nInTok, int32_t nOutTok, int64_t nTrans, const uint32_t *src,
                        const uint32_t *dst, const uint16_t *inTok, const uint16_t *outTok, const double *logWeight,
                        int mode, int backward, int closure, int G, const char *path);

/* The plan of the persistent-strip form of the pipelined Forward (host only): strips of C columns, pair p in matrix slot p % nSlots.
 * Writes the tickets as (pair, strip) int32 pairs in the order workgroups take them, and per pair (slot, strips of that slot that
 * must have finished before the pair starts); returns the number of tickets, -1 on error. */
int64_t mb_debug_persist_plan(int64_t nPairs, const int32_t *inLen, const int32_t *outLen, int32_t C, int64_t nSlots, int32_t *tickets,
                              int64_t maxTickets, int32_t *wait);

/* The same for the small-machine family (machines of <= 16 states: lane = column, states in registers); mode 0 = sum
 * semiring, 1 = max with fp64 cells, 2 = max with one traceback byte per cell, 3 = Forward fused with posterior counts;
 * mode + 32 writes the PROGRAM the generator unrolls instead: 20 int32 (magic 0x534D5031, S, nIn, nOut, backward, seed and end
 * state, table entries, off[4], nTab[4], candidates, 3 x 0), the evaluation order, decOff [S + 1], the candidates (T, src, dup,
 * tab) in the reference's enumeration order, w[] (fp64), eid[] (int32) -- tests/test_small_plan.py replays it. */
int mb_debug_small_source(int32_t nStates, int32_t nInTok, int32_t nOutTok, int64_t nTrans, const uint32_t *src,
                          const uint32_t *dst, const uint16_t *inTok, const uint16_t *outTok, const double *logWeight,
                          int mode, int backward, int materialise, const char *path);

/* The retimed program of a ONE-TAPE machine (the one-tape family's sweep, mb_wide.hip) exactly as the kernel reads it,
 * written to `path`: 12 int32 -- magic 0x52455431, lanes, slots per period, ring depth NB, doubles per ring vector, largest
 * lag, penalty row length, penalty entries, period, states, 1 = ring in L2 (records name entries, not LDS addresses),
 * streams -- then (NB * slots + 8) * lanes records of 16 bytes (fp64 weight, source word, end-of-round word).
 * mode MB_FORWARD = sum semiring, MB_VITERBI = max; MB_VITERBI + 16 (forward only) = the max program that keeps one traceback
 * code per cell (the default route of --align on one-tape machines), followed by its decode tables: int32 count + tbOff
 * [states + 1], int32 count + tbEntry (position in the incoming view << 16 | emitting << 15 | source state; 0xFFFFFFFF the
 * seed), int32 count + the incoming view's global edge ids.  Host only: the planner can be checked without a device. */
int mb_debug_wide_retimed(int32_t nStates, int32_t nInTok, int32_t nOutTok, int64_t nTrans, const uint32_t *src,
                          const uint32_t *dst, const uint16_t *inTok, const uint16_t *outTok, const double *logWeight,
                          int mode, int backward, const char *path);

/* The same program cut for k WORKGROUPS PER SEQUENCE (batches of fewer sequences than the device has CUs): int32
 * magic 0x52455432, parts, exchange columns, states; then per part 16 int32 (lanes, slots per period, NB, doubles per ring vector,
 * largest lag, penalty row length, penalty entries, period, own states, imports, first export entry, first exchange column,
 * exports, result entry or -1, table words, byte offset of the second weights or 0), the table (machine state of every own state,
 * then the exchange column of every import), (NB * slots + 8) * lanes records and -- parts with two-transition candidates (DESIGN
 * 4.2d) -- as many doubles, the candidates' second weights.  lanes = 0: the library's own choice.  Fails when the machine's
 * transition graph has no cut. */
int mb_debug_wide_parts(int32_t nStates, int32_t nInTok, int32_t nOutTok, int64_t nTrans, const uint32_t *src,
                        const uint32_t *dst, const uint16_t *inTok, const uint16_t *outTok, const double *logWeight,
                        int mode, int backward, int k, int lanes, const char *path);
/* The one-tape sweep GENERATED for this machine (run-time specialised retimed kernel), rendered on the host only: HIP source to `path`,
 * the unrolled program (rounds, slots, per-lane constant table) to `path`.prog for a device-free replay; k >= 2: the machine cut for k
 * workgroups per sequence, k <= 1: the one-workgroup program; mode: MB_FORWARD / MB_VITERBI (+ 16: traceback codes, + 64: fp64 correction
 * term); compile != 0: also compiled with hiprtc (fails when the kernel would spill to scratch memory). */
int mb_debug_wide_jit(int32_t nStates, int32_t nInTok, int32_t nOutTok, int64_t nTrans, const uint32_t *src, const uint32_t *dst,
                      const uint16_t *inTok, const uint16_t *outTok, const double *logWeight, int mode, int backward, int k, int lanes, int compile, const char *path);

#ifdef __cplusplus
}
#endif
#endif /* MBHIP_H_INCLUDED */
