// mb_options.h -- every MB_* option the library reads, written once: name, kind, default, class and a line of text.
//
// A reader names an option by its enumerator -- opt_int<MB_SMALL_JSUB>() -- so a misspelt name, the wrong accessor for the
// entry's kind, a default handed to an entry that has a fixed one or left out where the default depends on the call do not
// compile.  Every access asks the library's own override table (mb_set_option) first, then the environment; nothing is cached,
// so an option takes effect at the next read.  The few options that are latched (read once and then held) say so in their note.
// mb_get_option(NULL) returns this table as text; DESIGN.md section 4.7 describes the `host` entries.
#pragma once

#include <cstdlib>

namespace mb {

enum class OptKind {
  Int,       // atoi; unset or empty: the default
  Real,      // atof; unset or empty: the default
  Text,      // the string as it stands, or null when unset (the call site parses it)
  Present    // set at all, to whatever value (an empty environment value counts)
};
enum class OptClass {
  host,         // what a host may reasonably touch: the rows of DESIGN.md section 4.7
  planner,      // knobs of the planners and code generators, kept for the measurements in docs/history; not a supported surface
  diagnostic,   // logs, dumps and the hooks the tests use to reach a path (a time-out in microseconds, a poisoned pool)
  experiment,   // wrong results by design: read only in a library built with -DMB_EXPERIMENTS
  info          // read-only, answered by mb_get_option alone
};
constexpr double OPT_BY_CALL = 1e300;    // in the default column: the default depends on the call, the reader passes it
constexpr double OPT_NONE = -1e300;      // in the default column: Text, Present and info entries have none

// X(identifier = name, kind, default, class, note)
#define MB_OPTION_TABLE(X) \
  /* memory, reproducibility, multi-GPU */ \
  X(MB_MEM_FRACTION, Real, 0.90, host, "share of free + cached device memory the pools may fill; taken if 0 < f <= 0.95") \
  X(MB_POOL_STICKY, Int, 1, planner, "0: the memory budget follows the free memory at every call") \
  X(MB_DETERMINISTIC, Int, 0, host, "1: posterior counts through 64-bit fixed point, the same bits from run to run; read when a count call begins") \
  X(MB_COMM_TIMEOUT_S, Real, 180, host, "seconds mb_comm_init waits for the other ranks; <= 0: no limit") \
  X(MB_TIMING, Present, OPT_NONE, host, "host-side phase timing on stderr") \
  X(MB_DEBUG_POISON, Int, 0, diagnostic, "1: fill the count pool with 0xFF behind a call") \
  X(MB_INFO_INPLACE_RING_KERNELS, Int, OPT_NONE, info, "kernel kinds that took the in-place ring so far") \
  /* run-time compiler */ \
  X(MB_JIT_CACHE, Text, OPT_NONE, host, "first character 0: no code-object cache on disk") \
  X(MB_JIT_CACHE_DIR, Text, OPT_NONE, host, "directory of the code-object cache (default ~/.cache/mbhip; used only if private to the user)") \
  X(MB_JIT_EXTRA_OPTS, Text, OPT_NONE, planner, "further space-separated hiprtc options; part of the cache key") \
  /* family selection */ \
  X(MB_SMALL, Int, 1, host, "0: no small family") \
  X(MB_SMALL_MAX_STATES, Int, OPT_BY_CALL, host, "most states of the small family (its built-in limit, 16; the option can only lower it)") \
  X(MB_WIDE, Int, 1, host, "0: no one-tape family") \
  X(MB_WIDE_MIN_STATES, Int, 256, host, "fewest states of the one-tape family") \
  X(MB_MEDIUM_MIN_STATES, Int, 2, planner, "fewest states of the tiled family") \
  X(MB_ROLLING_MIN_PAIRS, Int, 192, host, "below this many pairs a rolling Forward runs through tiles") \
  /* small family */ \
  X(MB_SMALL_ONE_LAUNCH, Int, -1, host, "0 launch by launch, 1 tiles in one grid, 2 persistent strips always, -1 by rule") \
  X(MB_SMALL_ONE_LAUNCH_TIMEOUT_S, Int, 20, host, "seconds a strip waits for its neighbour") \
  X(MB_SMALL_ONE_LAUNCH_TIMEOUT_US, Int, 0, diagnostic, "the same wait in microseconds, over the seconds (the tests' way to a time-out)") \
  X(MB_SMALL_JSUB, Int, 16, host, "steps per hand-over of the persistent strips (even, 2..64)") \
  X(MB_SMALL_STRIP_PER_WG, Int, 1, planner, "0: four strips per workgroup") \
  X(MB_SMALL_MINWAVES, Int, OPT_BY_CALL, planner, "wavefronts per SIMD the generated kernel is bounded for (counts 4, under envelopes 3, else 1)") \
  X(MB_SMALL_STORE_LINES, Int, 1, planner, "0: 64 lanes per stored line") \
  X(MB_SMALL_BLOAD, Int, 0, planner, "1: count sweep loads the Backward cells late") \
  X(MB_SMALL_TS, Int, 0, planner, "steps per tile; 0 by rule") \
  X(MB_SMALL_ALLOW_SCRATCH, Int, 0, planner, "1: keep a generated kernel that spills to scratch memory") \
  X(MB_SMALL_TRACEBACK_WAVE_MAX_PAIRS, Int, 262144, planner, "most pairs traced back one per wavefront; latched at first use") \
  X(MB_SMALL_JIT_DUMP, Text, OPT_NONE, diagnostic, "prefix of files the generated sources are written to") \
  X(MB_SMALL_JIT_VERBOSE, Present, OPT_NONE, diagnostic, "compiler log of the small family") \
  /* tiled family: program */ \
  X(MB_MEDIUM_G, Int, 0, host, "columns per wavefront; 0 by rule") \
  X(MB_MEDIUM_CLOSURE, Int, 1, planner, "0: exact silent closure only") \
  X(MB_MEDIUM_CLOSURE_STAGES, Int, -1, host, "closure stages; -1 by rule") \
  X(MB_MEDIUM_CUTS, Text, OPT_NONE, planner, "comma list of level cuts; set: no search") \
  X(MB_MEDIUM_CUTS_SEARCH, Int, 1, planner, "0: no search over level cuts") \
  X(MB_MEDIUM_SYNC_COST, Int, 1, planner, "cost of a barrier in the cut search") \
  X(MB_MEDIUM_ROUND_COST, Int, 0, planner, "cost of a round in the cut search") \
  X(MB_MEDIUM_SPLIT_DEGREE, Int, 8, planner, "in-degree from which a state's candidates are split") \
  X(MB_MEDIUM_SPLIT_PART, Int, 8, planner, "candidates per part of a split state (at least 2)") \
  X(MB_MEDIUM_INPLACE_MAXSLOTS, Int, 48, planner, "most slots of a program that may update in place") \
  X(MB_MEDIUM_INPLACE_RING, Int, 0, planner, "1: in-place ring for rolling sweeps (measured: does not pay)") \
  X(MB_MEDIUM_COMPACT_MAXWAVES, Int, 12, planner, "most wavefronts of the in-place ring (at most 16)") \
  /* tiled family: geometry and launches */ \
  X(MB_MEDIUM_TS, Text, OPT_NONE, host, "steps per tile, taken if at least the tile's columns") \
  X(MB_MEDIUM_TS_LONG_MIN_PAIRS, Int, 32, planner, "fewest pairs at which long outputs take 128-step tiles") \
  X(MB_MEDIUM_MAXWAVES, Text, OPT_NONE, planner, "most wavefronts per workgroup, taken if positive and below the rule's") \
  X(MB_MEDIUM_FIT_RECORDS, Text, OPT_NONE, planner, "set and 0: columns are not given up for records in LDS") \
  X(MB_MEDIUM_HALO_TILE, Int, 1, planner, "0: no halo pre-load in the tile prologue") \
  X(MB_MEDIUM_ADAPT_WIDTH, Int, 1, planner, "0: the strip width does not follow the batch") \
  X(MB_MEDIUM_STREAMS, Int, 2, host, "streams of the materialised sweeps") \
  X(MB_MEDIUM_ROLLTILES, Int, 1, planner, "0: no rolling Forward through tiles") \
  X(MB_MEDIUM_PIPELINE, Int, 1, host, "0: sub-batches instead of the recycled-slot pipeline") \
  X(MB_MEDIUM_PERSIST, Int, -1, host, "pipeline: 0 launch by launch, else persistent strips where the halo columns fit") \
  X(MB_MEDIUM_PERSIST_AHEAD, Int, 16, host, "halo rows a persistent strip reads ahead (1..256)") \
  X(MB_MEDIUM_PERSIST_TIMEOUT_S, Int, 20, host, "seconds a persistent strip waits for its neighbour") \
  X(MB_MEDIUM_PERSIST_TIMEOUT_US, Int, 0, diagnostic, "the same wait in microseconds, over the seconds (the tests' way to a time-out)") \
  X(MB_MEDIUM_TB, Int, 1, planner, "0: no traceback-byte Viterbi") \
  /* tiled family: E-step */ \
  X(MB_MEDIUM_COUNTS, Int, 1, planner, "0: no count program") \
  X(MB_MEDIUM_COUNT_G, Int, 0, planner, "columns per wavefront of the count program; 0 by rule") \
  X(MB_MEDIUM_COUNT_PASSES, Int, 0, host, "2 fused sweep, 3 two fills + usage pass, 0 by rule") \
  X(MB_MEDIUM_COUNTS_ROLL, Int, 1, planner, "0: counts through materialised matrices") \
  X(MB_MEDIUM_COUNT_FIT, Int, 1, planner, "0: count programs keep their columns") \
  X(MB_MEDIUM_COUNT_FLAT, Int, 1, planner, "0: no flat count program") \
  X(MB_MEDIUM_COUNT_FUSE, Int, 1, planner, "0: count rounds are not fused") \
  X(MB_MEDIUM_COUNT_COMPACT, Int, 1, planner, "0: no compact accumulator table") \
  X(MB_MEDIUM_COUNT_MAXWAVES, Int, 8, planner, "most wavefronts of a count kernel (1..16)") \
  /* tiled family: generated kernels */ \
  X(MB_MEDIUM_JIT, Text, OPT_NONE, host, "first character 0: ahead-of-time interpreter kernels") \
  X(MB_MEDIUM_JIT_VERBOSE, Int, 0, host, "set: planner and compiler log; 2 and more: the program as well") \
  X(MB_MEDIUM_JIT_DUMP, Text, OPT_NONE, diagnostic, "prefix of files the generated sources are written to") \
  X(MB_JIT_MAXCANDS, Int, 12, planner, "candidates of one straight-line round body (at least 2); latched when the library loads") \
  X(MB_JIT_REGBUDGET, Int, OPT_BY_CALL, planner, "registers for records (what the wavefronts leave, less 84)") \
  X(MB_JIT_PLACE, Int, 1, planner, "0: legacy record placement") \
  X(MB_JIT_STORE2, Int, OPT_BY_CALL, planner, "two cells per store (1 for an even state count and at most 8 lanes per group)") \
  X(MB_JIT_STORENT, Int, 0, planner, "1: non-temporal stores") \
  X(MB_JIT_NEIGHBOUR_SYNC, Int, OPT_BY_CALL, planner, "wavefronts wait for their neighbour, not a barrier (0 for count sweeps with G != 1, else 1)") \
  X(MB_JIT_B_DISTANCE, Int, 1, planner, "count sweep: steps the Backward supercells are fetched ahead (1 or 2)") \
  X(MB_JIT_STAGE_LOADS, Int, 1, planner, "0: loads are not staged") \
  X(MB_JIT_STAGE_MAXLOADS, Int, 32, planner, "most loads of a stage (at least 1)") \
  X(MB_JIT_FLAT_CHUNK, Int, 24, planner, "transitions per chunk of the flat count epilogue; <= 0: one chunk") \
  X(MB_JIT_AGPR_SPILLS, Int, 0, planner, "1: keep AGPR spill slots when a kernel uses scratch memory") \
  X(MB_JIT_DEBUG, Int, 0, experiment, "bits that switch loads off in the tile kernels") \
  /* generic family */ \
  X(MB_TRACEBACK_LDS, Text, OPT_NONE, planner, "first character 0: traceback without LDS tables; latched at first use") \
  X(MB_TRACEBACK_SCAN, Int, 1, planner, "0: no scanning traceback") \
  /* one-tape family: program */ \
  X(MB_WIDE_LANES, Int, OPT_BY_CALL, planner, "lanes per workgroup (1024 from 192 states, else 256)") \
  X(MB_WIDE_MAX_GROUP, Int, 64, planner, "most states of a group (1..64)") \
  X(MB_WIDE_FAST_INDEX, Int, 1, planner, "0: no 16-bit indices") \
  X(MB_WIDE_GLOBAL_VECTORS, Int, 0, planner, "1: state vectors in global memory") \
  X(MB_WIDE_VITERBI_PHASES, Int, 1, planner, "0: no phased Viterbi program") \
  X(MB_WIDE_VITERBI_MIN_STATES, Int, 2048, planner, "most states of a one-tape machine whose Viterbi fill may run through tiles") \
  X(MB_WIDE_RETIMED, Int, 1, planner, "0: no retimed program") \
  X(MB_WIDE_RETIMED_PERIOD, Int, 0, planner, "period of the retimed program; 0 searched") \
  X(MB_WIDE_RETIMED_L2, Int, 1, planner, "0: a retimed ring never lives in L2") \
  X(MB_WIDE_FP32, Int, -1, planner, "1 asks for the fp32 kernel, 0 refuses it, -1 by rule") \
  X(MB_WIDE_CLOSURE_STAGES, Int, -1000000, planner, "closure stages; unset: searched") \
  X(MB_WIDE_ADAPTIVE_STAGES, Int, 1, planner, "0: no adaptive closure candidates") \
  X(MB_WIDE_WAVE_LOCAL, Int, 1, planner, "0: no wavefront-local rounds") \
  X(MB_WIDE_HYBRID, Int, -1, planner, "hybrid fp32/fp64 vectors: 1 on, 0 off, -1 by rule") \
  /* one-tape family: generated kernels */ \
  X(MB_WIDE_JIT, Int, 1, host, "0: interpreter kernels") \
  X(MB_WIDE_JIT_LEVEL, Int, -1, host, "constants: 0 in registers, 1 streamed, -1 by rule") \
  X(MB_WIDE_JIT_TWOPASS, Int, 1, host, "0: online log-sum-exp rounds") \
  X(MB_WIDE_JIT_DUMP, Text, OPT_NONE, host, "prefix of files the generated sources are written to") \
  X(MB_WIDE_JIT_ALLOW_SCRATCH, Int, 0, planner, "1: keep a generated kernel that spills to scratch memory") \
  X(MB_WIDE_JIT_ATTEMPT, Int, 0, diagnostic, "first planning attempt of the debug entry point") \
  X(MB_WIDE_JIT_KNOCKOUT, Int, 0, experiment, "bits that switch parts of the generated kernel off") \
  X(MB_WIDE_VERBOSE, Present, OPT_NONE, host, "planner and compiler log of the one-tape family") \
  X(MB_WIDE_VERBOSE_MERGE, Present, OPT_NONE, diagnostic, "with MB_WIDE_VERBOSE: every merge iteration") \
  X(MB_WIDE_VERBOSE_PARTS, Present, OPT_NONE, diagnostic, "with MB_WIDE_VERBOSE: the builds of the part search as well") \
  /* one-tape family: workgroups per sequence, cuts */ \
  X(MB_ONETAPE_PARTS, Int, OPT_BY_CALL, host, "most workgroups per sequence (8; 16 where the ring lives in L2; 1: off)") \
  X(MB_ONETAPE_PARTS_MIN_LEN, Int, OPT_BY_CALL, host, "shortest sweep worth parts (4096; 64 where the ring lives in L2)") \
  X(MB_ONETAPE_PART_LANES, Int, 0, host, "lanes per part (a multiple of 64 up to 1024); 0 searched") \
  X(MB_ONETAPE_PART_RING, Int, 0, planner, "ring depth asked of the parts (4 or 8); 0 by rule") \
  X(MB_ONETAPE_PART_MERGE, Int, 1, host, "0: no two-transition candidates in the parts") \
  X(MB_ONETAPE_PART_TIMEOUT_S, Real, 20, host, "seconds (a fraction counts) a lane waits for another part's value") \
  X(MB_ONETAPE_PART_EXCLUSIVE, Int, 1, planner, "0: parts may share a CU") \
  X(MB_ONETAPE_SPLIT, Int, 1, host, "0: sequences are not cut in two") \
  X(MB_ONETAPE_SPLIT_BALANCE, Int, 1, planner, "0: cut in the middle, not by measured cost") \
  X(MB_ONETAPE_SPLIT_MIN_LEN, Int, 64, planner, "shortest sequence worth a cut") \
  X(MB_ONETAPE_CONCURRENT_FILLS, Int, 1, planner, "0: E-step fills one after the other") \
  /* one-tape family: traceback and counts */ \
  X(MB_ONETAPE_TB, Int, 1, host, "0: alignment through the fp64 matrix, not traceback codes") \
  X(MB_ONETAPE_TB_FAST, Int, 1, planner, "0: no fast traceback tables") \
  X(MB_ONETAPE_TRACEBACK, Int, 1, planner, "0: no device traceback") \
  X(MB_ONETAPE_TRACEBACK_MIN_TRANS, Int, 3584, planner, "transitions above which the one-tape traceback takes the machine") \
  X(MB_ONETAPE_COUNTS, Int, 1, planner, "0: no one-tape count sweep") \
  X(MB_ONETAPE_COUNTS_LDS, Int, 1, planner, "0: no count accumulators in LDS") \
  X(MB_ONETAPE_COUNT_UNITS, Int, 32, planner, "work units per sequence of the count sweep") \
  X(MB_ONETAPE_COUNT_LDS_UNITS, Int, 256, planner, "work units of the LDS count sweep") \
  X(MB_ONETAPE_COUNT_NORMALISE, Int, 1, planner, "0: no per-column normalisation") \
  X(MB_ONETAPE_COUNT_FP64, Int, -1, host, "fp64 correction term of E-step fills: 1 on, 0 off, -1 by length") \
  X(MB_ONETAPE_COUNT_FP64_MIN_LEN, Int, 10000, planner, "length from which E-step fills take the fp64 correction term") \
  /* profile sweeps */ \
  X(MB_ROWPOST_TABLE, Int, OPT_BY_CALL, planner, "entries of the row-posterior table in LDS (its built-in limit, 4096; the option can only lower it)")

enum Opt : int {
#define MB_OPTION_ID(id, kind, dflt, cls, note) id,
  MB_OPTION_TABLE(MB_OPTION_ID)
#undef MB_OPTION_ID
  OPT_COUNT
};

struct OptEntry { const char *name; OptKind kind; double dflt; OptClass cls; const char *kindName, *clsName, *note; };
constexpr OptEntry OPT_TABLE[OPT_COUNT] = {
#define MB_OPTION_ROW(id, kind, dflt, cls, note) {#id, OptKind::kind, dflt, OptClass::cls, #kind, #cls, note},
  MB_OPTION_TABLE(MB_OPTION_ROW)
#undef MB_OPTION_ROW
};

const char *opt_raw(Opt id);                      // the override if there is one, else the environment's value, else null
void opt_override(Opt id, const char *value);     // null or "": the override goes
int opt_find(const char *name);                   // index into OPT_TABLE, -1 for a name that is not in it
const char *opt_list();                           // one line per entry: name, kind, default, class, note, tab-separated

template <Opt id> bool opt_present() { return opt_raw(id) != nullptr; }      // (legal for every kind; the only accessor of a Present entry)
template <Opt id> const char *opt_text() {
  static_assert(OPT_TABLE[id].kind == OptKind::Text, "opt_text: the entry is not of kind Text");
  return opt_raw(id);
}
template <Opt id> int opt_int(int dflt) {
  static_assert(OPT_TABLE[id].kind == OptKind::Int && OPT_TABLE[id].dflt == OPT_BY_CALL, "opt_int(dflt): the entry is not an Int whose default is by call");
  const char *v = opt_raw(id);
  return v && *v ? atoi(v) : dflt;
}
template <Opt id> int opt_int() {
  static_assert(OPT_TABLE[id].kind == OptKind::Int && OPT_TABLE[id].dflt != OPT_BY_CALL && OPT_TABLE[id].dflt != OPT_NONE, "opt_int(): the entry is not an Int with a fixed default");
  const char *v = opt_raw(id);
  return v && *v ? atoi(v) : (int)OPT_TABLE[id].dflt;
}
template <Opt id> double opt_real() {
  static_assert(OPT_TABLE[id].kind == OptKind::Real && OPT_TABLE[id].dflt != OPT_BY_CALL && OPT_TABLE[id].dflt != OPT_NONE, "opt_real(): the entry is not a Real with a fixed default");
  const char *v = opt_raw(id);
  return v && *v ? atof(v) : OPT_TABLE[id].dflt;
}

}  // namespace mb
