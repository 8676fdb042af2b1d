// mb_debug_api.hip -- the introspection entry points of the C-ABI (include/mbhip.h, mb_debug_*): the programs and the generated
// sources of the kernel families, planned and rendered on the host only (no device needed).  The device-free replays of the plan
// tests read what these write.
#include <algorithm>
#include <cstring>
#include <string>
#include <vector>

#include "mb_api_internal.h"
#include "mb_jit.h"
#include "mb_medium.h"
#include "mb_small.h"
#include "mb_wide.h"
#include "mb_wide_jit.h"

using namespace mb;

extern "C" {

// ---- introspection: generated source of the run-time specialised tile kernel (host only, no device needed) ------
int mb_debug_jit_source(int32_t nStates, int32_t nInTok, int32_t nOutTok, int64_t nTrans, const uint32_t *src, const uint32_t *dst,
                        const uint16_t *inTok, const uint16_t *outTok, const double *logWeight, int mode, int backward, int closure,
                        int G, const char *path) {
  ApiLock lock;
  if (nStates <= 0 || nTrans < 0 || !path) { set_error("mb_debug_jit_source: bad argument"); return 1; }
  if (!medium_valid_G(G)) { set_error("mb_debug_jit_source: G must be a power of two in 1..64"); return 1; }
  mb_machine m;
  m.S = nStates; m.nIn = nInTok; m.nOut = nOutTok; m.nTrans = nTrans;
  m.src.assign(src, src + nTrans); m.dst.assign(dst, dst + nTrans);
  m.inTok.assign(inTok, inTok + nTrans); m.outTok.assign(outTok, outTok + nTrans);
  m.logW.assign(logWeight, logWeight + nTrans);
  std::string err;
  if (!compile_machine(&m, &err)) { set_error(err); return 1; }
  // mode: MB_FORWARD sum, MB_VITERBI max, 3 count, 4 max with traceback bytes; + 16: tiles without a matrix (MED_MAT_ROLL; implied by 4);
  // + 32: the PROGRAM instead of the source (see below); + 128: the persistent-strip matrix kernel (MED_MAT_PERSIST, sum only)
  const int matKind = (mode & 128) ? MED_MAT_PERSIST : (((mode & 16) || (mode & 15) == MED_MODE_TB) ? MED_MAT_ROLL : MED_MAT_FULL);
  const bool dumpProgram = (mode & 32) != 0;
  const bool compactRing = (mode & 64) != 0;      // + 64: the matrix-free kernel with the COMPACT ring (as many wavefronts as its LDS allows, at most 12)
  mode &= 15;
  MedProgram P; MedGeom geo;
  if (matKind == MED_MAT_ROLL) geo.haloSteps = 0;
  if (mode == MED_MODE_COUNT) {
    if (!medium_build_count_host(&m, G, P, geo, closure)) { set_error("machine does not qualify for the fused count kernel"); return 1; }
  } else if (!medium_build_host(&m, backward != 0, closure, G, P, geo)) return 1;
  if (opt_present<MB_MEDIUM_JIT_VERBOSE>()) {
    const long long c = medium_program_cost(P); int syncs = 0;
    for (const MedRoundInfo &ri : P.roundInfo) syncs += ri.sync;
    fprintf(stderr, "[mbhip] program cost %lld (rounds %zu, syncs %d, pairs %d, levels %d)\n", c, P.roundInfo.size(), syncs, P.nPairs, backward ? m.nLevB : m.nLevF);
  }
  if (dumpProgram) {
    // The program as the kernels read it -- descriptors + records, what med_slow_supercell (mb_medium.hip) interprets chunk by chunk
    // and the run-time generator unrolls --, for a device-free replay (tests/test_tiled_plan.py): 16 int32 (magic 0x4D454431, S, Spad,
    // LPG, G, nChunks, nIn, nOut, seedOff, dummyOff, records, usage slots of a flat count program, 1 = backward, closure stages,
    // 1 = counting, flags: 1 flat | 2 emitting usage fused into the fill rounds | 4 two accumulator tables), nChunks x 8 int32
    // descriptors, the records (fp64 weight, srcOff, dstOff), the usage slots (int32 table, first record, placement), one int32 per
    // record: the transition it stands for, then int32 fused slots, int32 loop-time accumulators, the fused slots (table, first
    // record, placement) and the loop-time table's transitions
    FILE *f = fopen(path, "wb");
    if (!f) { set_error("mb_debug_jit_source: cannot open output file"); return 1; }
    // usage slots: (table, first record, placement 2 = VGPRs: summed in a register, set down in the after-the-loop table; else: the
    // loop-time table) -- the usage pass of a flat count program, then the fused emit slots of its fill rounds (MedProgram::fusedEmit)
    std::vector<int32_t> flatSlots, fusedSlots;
    for (const MedRoundInfo &ri : P.roundInfo)
      for (const MedSlotInfo &sl : ri.slots) {
        if (ri.flat) { flatSlots.push_back(sl.T); flatSlots.push_back((int32_t)sl.recBase); flatSlots.push_back(sl.place); }
        else if (ri.fused && sl.T < 3) { fusedSlots.push_back(sl.T); fusedSlots.push_back((int32_t)sl.recBase); fusedSlots.push_back(sl.place); }
      }
    const int32_t head[16] = {0x4D454431, m.S, P.Spad, P.LPG, P.G, P.nChunks, m.nIn, m.nOut, (int32_t)P.dev.seedOff, (int32_t)P.dummyOff, (int32_t)P.rec.size(),
                              (int32_t)(flatSlots.size() / 3), P.backward ? 1 : 0, closure, P.counting ? 1 : 0, (P.flatCount ? 1 : 0) | (P.fusedEmit ? 2 : 0) | (P.accAllEntries ? 4 : 0)};
    const int32_t tail[2] = {(int32_t)(fusedSlots.size() / 3), (int32_t)P.accMap.size()};
    const bool ok = fwrite(head, sizeof(head), 1, f) == 1 && fwrite(P.desc.data(), 4, (size_t)P.nChunks * MED_DESC_WORDS, f) == (size_t)P.nChunks * MED_DESC_WORDS &&
                    fwrite(P.rec.data(), sizeof(MedRec), P.rec.size(), f) == P.rec.size() &&
                    (flatSlots.empty() || fwrite(flatSlots.data(), 4, flatSlots.size(), f) == flatSlots.size()) &&
                    fwrite(P.wref.data(), 4, P.wref.size(), f) == P.wref.size() &&      // per record: >= 0 its transition, -1 padding, <= -2 a closure pair
                    fwrite(tail, sizeof(tail), 1, f) == 1 && (fusedSlots.empty() || fwrite(fusedSlots.data(), 4, fusedSlots.size(), f) == fusedSlots.size()) &&
                    (P.accMap.empty() || fwrite(P.accMap.data(), 4, P.accMap.size(), f) == P.accMap.size());      // loop-time accumulator entry -> transition
    fclose(f);
    if (!ok) { set_error("mb_debug_jit_source: short write"); return 1; }
    return 0;
  }
  if (matKind != MED_MAT_FULL) geo.haloSteps = 0;
  if (compactRing) {
    if (matKind != MED_MAT_ROLL || P.recC.empty()) { set_error("mb_debug_jit_source: no compact ring for this kernel kind"); return 1; }
    geo.compact = true; geo.haloSteps = 0;
    for (geo.waves = 12; geo.waves > 1; --geo.waves) {
      geo.C = geo.waves * P.G;
      if (medium_jit_lds_bytes(P, geo, mode == MED_MODE_TB ? MED_MODE_TB : MB_FORWARD) <= 160 * 1024 - 512) break;
    }
  }
  if (mode == MED_MODE_TB && !medium_tb_eligible(&m, P)) { set_error("machine does not qualify for traceback bytes on the tiled family"); return 1; }
  if (matKind == MED_MAT_PERSIST && mode != MB_FORWARD) { set_error("mb_debug_jit_source: the persistent-strip kernel is a sum kernel"); return 1; }
  const std::string code = medium_jit_source(&m, P, geo, mode == MED_MODE_COUNT ? MED_MODE_COUNT : (mode == MED_MODE_TB ? MED_MODE_TB : (mode == MB_VITERBI ? MB_VITERBI : MB_FORWARD)), matKind);
  FILE *f = fopen(path, "w");
  if (!f) { set_error("mb_debug_jit_source: cannot open output file"); return 1; }
  fprintf(f, "// G=%d C=%d waves=%d ldsBytes=%zu ldsRecs=%zu rounds=%zu\n", G, geo.C, geo.waves, medium_jit_lds_bytes(P, geo),
          P.ldsImageIdx.size(), P.roundInfo.size());
  fputs(code.c_str(), f);
  fclose(f);
  return 0;
}

// The retimed program of a one-tape machine (mb_wide.hip, k_wide_retimed) as the kernel reads it, written to `path`: 12 int32
// (magic 0x52455431, lanes, slots per period, ring depth NB, doubles per ring vector, largest lag, penalty row length, penalty
// entries, period, states, 1 = ring in L2, streams) followed by (NB * slots + 8) * lanes records of 16 bytes.  Host only: the
// planner can be checked without a device (tests/test_retimed_plan.py simulates the stream and compares with the oracle).
int mb_debug_wide_retimed(int32_t nStates, int32_t nInTok, int32_t nOutTok, int64_t nTrans, const uint32_t *src, const uint32_t *dst,
                          const uint16_t *inTok, const uint16_t *outTok, const double *logWeight, int mode, int backward, const char *path) {
  ApiLock lock;
  if (nStates <= 0 || nTrans < 0 || !path || (nInTok != 0) == (nOutTok != 0)) { set_error("mb_debug_wide_retimed: bad argument (one-tape machines only)"); return 1; }
  mb_machine m;
  m.S = nStates; m.nIn = nInTok; m.nOut = nOutTok; m.nTrans = nTrans;
  m.src.assign(src, src + nTrans); m.dst.assign(dst, dst + nTrans);
  m.inTok.assign(inTok, inTok + nTrans); m.outTok.assign(outTok, outTok + nTrans);
  m.logW.assign(logWeight, logWeight + nTrans);
  std::string err;
  if (!compile_machine(&m, &err)) { set_error(err); return 1; }
  WideProgram P;
  std::vector<WideRec> stream;
  // mode + 16 (with MB_VITERBI, forward): the program that keeps one traceback CODE per cell; its decode tables and the incoming
  // view's edge ids follow the record streams: int32 count + tbOff, int32 count + tbEntry, int32 count + inEid
  const bool tbCodes = (mode & 16) != 0;
  mode &= 15;
  if (tbCodes && (mode != MB_VITERBI || backward)) { set_error("mb_debug_wide_retimed: traceback codes belong to the forward max program"); return 1; }
  if (!wide_ret_host(&m, backward != 0, mode == MB_VITERBI, P, stream, tbCodes)) { set_error("machine has no retimed program"); return 1; }
  if (tbCodes && !P.tbOk) { set_error("machine does not qualify for traceback codes"); return 1; }
  FILE *f = fopen(path, "wb");
  if (!f) { set_error("mb_debug_wide_retimed: cannot open output file"); return 1; }
  const int32_t head[12] = {0x52455431, P.W, P.ret.nSlots, P.ret.NB, P.ret.NVs, P.ret.kMax, P.ret.rowLen, P.ret.nPen, P.retPeriod, nStates, P.retGv ? 1 : 0, P.ret.NB};
  bool ok = fwrite(head, sizeof(head), 1, f) == 1 && fwrite(stream.data(), sizeof(WideRec), stream.size(), f) == stream.size();
  if (ok && tbCodes) {
    const int32_t n0 = (int32_t)P.h_tbOff.size(), n1 = (int32_t)P.h_tbEntry.size(), n2 = (int32_t)m.inPerm.size();
    ok = fwrite(&n0, 4, 1, f) == 1 && fwrite(P.h_tbOff.data(), 4, (size_t)n0, f) == (size_t)n0 &&
         fwrite(&n1, 4, 1, f) == 1 && fwrite(P.h_tbEntry.data(), 4, (size_t)n1, f) == (size_t)n1 &&
         fwrite(&n2, 4, 1, f) == 1 && fwrite(m.inPerm.data(), 4, (size_t)n2, f) == (size_t)n2;
  }
  fclose(f);
  if (!ok) { set_error("mb_debug_wide_retimed: short write"); return 1; }
  return 0;
}

// the k-part form of the retimed program (k workgroups per sequence, WidePartDev), planned on the host only: int32 magic 0x52455432,
// parts, exchange columns, states; then per part 16 int32 (lanes, slots, NB, NVs, kMax, rowLen, nPen, period, own states, imports,
// first export entry, first exchange column, exports, result entry, table words, byte offset of the second weights or 0), the table (machine
// state of every own state, then the exchange column of every import), the record streams as in mb_debug_wide_retimed and -- parts with
// two-transition candidates -- one double per record: the candidate's second weight
int mb_debug_wide_parts(int32_t nStates, int32_t nInTok, int32_t nOutTok, int64_t nTrans, const uint32_t *src, const uint32_t *dst,
                        const uint16_t *inTok, const uint16_t *outTok, const double *logWeight, int mode, int backward, int k, int lanes, const char *path) {
  ApiLock lock;
  if (nStates <= 0 || nTrans < 0 || !path || (nInTok != 0) == (nOutTok != 0)) { set_error("mb_debug_wide_parts: bad argument (one-tape machines only)"); return 1; }
  mb_machine m;
  m.S = nStates; m.nIn = nInTok; m.nOut = nOutTok; m.nTrans = nTrans;
  m.src.assign(src, src + nTrans); m.dst.assign(dst, dst + nTrans);
  m.inTok.assign(inTok, inTok + nTrans); m.outTok.assign(outTok, outTok + nTrans);
  m.logW.assign(logWeight, logWeight + nTrans);
  std::string err;
  if (!compile_machine(&m, &err)) { set_error(err); return 1; }
  const bool tbCodes = (mode & 16) != 0;
  mode &= 15;
  std::vector<WidePartHost> parts;
  int nExpTot = 0;
  std::vector<int> tbOff; std::vector<uint32_t> tbEntry;
  if (tbCodes && (mode != MB_VITERBI || backward)) { set_error("mb_debug_wide_parts: traceback codes belong to the forward max program"); return 1; }
  int lanesChosen = lanes, ringChosen = 8;
  if (!wide_parts_host(&m, backward != 0, mode == MB_VITERBI, tbCodes, k, lanes, parts, nExpTot, &tbOff, &tbEntry, nullptr, &lanesChosen, &ringChosen)) { set_error("machine has no k-part retimed program"); return 1; }
  lanes = lanesChosen;
  FILE *f = fopen(path, "wb");
  if (!f) { set_error("mb_debug_wide_parts: cannot open output file"); return 1; }
  const int32_t head[4] = {0x52455432, (int32_t)parts.size(), nExpTot, nStates};
  bool ok = fwrite(head, sizeof(head), 1, f) == 1;
  for (const WidePartHost &H : parts) {
    const int32_t ph[16] = {lanes, H.h.ret.nSlots, H.h.ret.NB, H.h.ret.NVs, H.h.ret.kMax, H.h.ret.rowLen, H.h.ret.nPen, H.period, H.h.Sloc, H.h.nImp,
                            H.h.expBase, H.h.expIdx0, H.h.nExp, H.h.resultEntry, (int32_t)H.tab.size(), H.h.w2Offset};
    ok = ok && fwrite(ph, sizeof(ph), 1, f) == 1 && fwrite(H.tab.data(), 4, H.tab.size(), f) == H.tab.size() &&
         fwrite(H.stream.data(), sizeof(WideRec), H.stream.size(), f) == H.stream.size();
  }
  if (ok && tbCodes) {      // the joined decode tables of the parts' candidate lists, and the incoming view's edge ids
    const int32_t n0 = (int32_t)tbOff.size(), n1 = (int32_t)tbEntry.size(), n2 = (int32_t)m.inPerm.size();
    ok = fwrite(&n0, 4, 1, f) == 1 && fwrite(tbOff.data(), 4, (size_t)n0, f) == (size_t)n0 &&
         fwrite(&n1, 4, 1, f) == 1 && fwrite(tbEntry.data(), 4, (size_t)n1, f) == (size_t)n1 &&
         fwrite(&n2, 4, 1, f) == 1 && fwrite(m.inPerm.data(), 4, (size_t)n2, f) == (size_t)n2;
  }
  fclose(f);
  if (!ok) { set_error("mb_debug_wide_parts: short write"); return 1; }
  return 0;
}

// the one-tape sweep GENERATED for this machine (mb_wide_jit.cpp), planned and rendered on the host only: k >= 2: the machine cut for k
// workgroups per sequence (lanes = 0: searched), k <= 1: the one-workgroup program.  mode: MB_FORWARD / MB_VITERBI, + 16 traceback codes,
// + 64 the fp64 correction term.  Writes the HIP source to `path` and, to `path`.prog, what the source unrolls -- for the device-free replay
// of tests/test_retimed_plan.py: int32 magic 0x4A495431, parts, exchange columns, states; per part 24 int32 (lanes, NB, NVs, kMax, rowLen,
// nPen, nImp, S, expBase, nExp, expIdx0, resultEntry, slots, rounds, NPT, U, penBase, tokBase, ringBase, dummyAddr, ldsBytes, fields,
// words, 0), per slot 2 int32 (anyPen, anyW2), per round 8 int32 (firstSlot, depth, sync, uniform, gAll, anyMixed, resultLane, mask of the lane-group sizes its switch serves), per
// field 4 int32 (kind, index, cm, words), then the table [words][lanes] uint32.  compile != 0: the source is also compiled with hiprtc
// (no device needed) and the call fails when the kernel would use scratch memory.
int mb_debug_wide_jit(int32_t nStates, int32_t nInTok, int32_t nOutTok, int64_t nTrans, const uint32_t *src, const uint32_t *dst,
                      const uint16_t *inTok, const uint16_t *outTok, const double *logWeight, int mode, int backward, int k, int lanes, int compile, const char *path) {
  ApiLock lock;
  if (nStates <= 0 || nTrans < 0 || !path || (nInTok != 0) == (nOutTok != 0)) { set_error("mb_debug_wide_jit: bad argument (one-tape machines only)"); return 1; }
  mb_machine m;
  m.S = nStates; m.nIn = nInTok; m.nOut = nOutTok; m.nTrans = nTrans;
  m.src.assign(src, src + nTrans); m.dst.assign(dst, dst + nTrans);
  m.inTok.assign(inTok, inTok + nTrans); m.outTok.assign(outTok, outTok + nTrans);
  m.logW.assign(logWeight, logWeight + nTrans);
  std::string err;
  if (!compile_machine(&m, &err)) { set_error(err); return 1; }
  const bool tbCodes = (mode & 16) != 0, acc = (mode & 64) != 0;
  mode &= 15;
  if (tbCodes && (mode != MB_VITERBI || backward)) { set_error("mb_debug_wide_jit: traceback codes belong to the forward max program"); return 1; }
  std::vector<WidePartHost> parts;
  std::vector<WideRec> stream;
  WideProgram P;
  std::vector<WideJitIn> ins;
  int nExpTot = 0;
  if (k >= 2) {
    int lanesChosen = lanes, mergeFlag = 0;
    if (!wide_parts_host(&m, backward != 0, mode == MB_VITERBI, tbCodes, k, lanes, parts, nExpTot, nullptr, nullptr, nullptr, &lanesChosen, &mergeFlag)) { set_error("machine has no k-part retimed program"); return 1; }
    for (const WidePartHost &H : parts) {
      WideJitIn in;
      in.ret = H.h.ret; in.W = lanesChosen; in.stream = H.stream.data();
      in.w2 = H.h.w2Offset ? (const double *)((const char *)H.stream.data() + H.h.w2Offset) : nullptr;
      in.part = true; in.S = H.h.Sloc; in.Sg = nStates; in.nImp = H.h.nImp; in.expBase = H.h.expBase; in.nExp = H.h.nExp; in.expIdx0 = H.h.expIdx0; in.resultEntry = H.h.resultEntry;
      in.gmap = H.tab.data();
      ins.push_back(in);
    }
  } else {
    if (!wide_ret_host(&m, backward != 0, mode == MB_VITERBI, P, stream, tbCodes) || P.retGv) { set_error("machine has no retimed program with its ring in LDS"); return 1; }
    WideJitIn in;
    in.ret = P.ret; in.W = P.W; in.stream = stream.data(); in.S = nStates; in.Sg = nStates; in.resultEntry = backward ? 0 : nStates - 1;
    ins.push_back(in);
  }
  WideJitFlags F; F.viterbi = mode == MB_VITERBI; F.tb = tbCodes; F.acc = acc; F.backward = backward != 0; F.inputTape = nOutTok == 0; F.nExpTot = nExpTot;
  // the plan the library would run: the register estimate's choice, planned again with fewer constants in registers while the compiled
  // kernel spills (mb_wide_jit.cpp, wide_jit_plan; MB_WIDE_JIT_ATTEMPT: the attempt to start from -- the device-free replays of the later ones)
  std::vector<WideJitDesc> descs;
  std::string code, obj;
  for (int attempt = std::max(0, std::min(opt_int<MB_WIDE_JIT_ATTEMPT>(), WIDE_JIT_ATTEMPTS - 1));; ++attempt) {
    std::string why;
    if (!wide_jit_plan(ins, acc != 0, attempt, descs, &why)) { set_error("mb_debug_wide_jit: " + why); return 1; }
    code = wide_jit_source(descs, F);
    if (!compile) break;
    std::string log;
    if (!jit_compile(code, "mb_wide_jit.hip", obj, &log, nullptr)) { set_error("mb_debug_wide_jit: hiprtc: " + log.substr(0, 2000)); return 1; }
    const long long scratch = jit_kernel_meta(obj, ".private_segment_fixed_size");
    if (scratch <= 0) break;
    if (attempt + 1 >= WIDE_JIT_ATTEMPTS) { set_error("mb_debug_wide_jit: the kernel uses " + std::to_string(scratch) + " bytes of scratch memory"); return 1; }
  }
  FILE *f = fopen(path, "w");
  if (!f) { set_error("mb_debug_wide_jit: cannot open output file"); return 1; }
  fputs(code.c_str(), f);
  fclose(f);
  f = fopen((std::string(path) + ".prog").c_str(), "wb");
  if (!f) { set_error("mb_debug_wide_jit: cannot open output file"); return 1; }
  const int32_t head[4] = {0x4A495431, (int32_t)descs.size(), nExpTot, nStates};
  bool ok = fwrite(head, sizeof(head), 1, f) == 1;
  for (const WideJitDesc &D : descs) {
    const WideJitIn &in = D.in;
    const int32_t ph[24] = {in.W, in.ret.NB, in.ret.NVs, in.ret.kMax, in.ret.rowLen, in.ret.nPen, in.nImp, in.S, in.expBase, in.nExp, in.expIdx0, in.resultEntry,
                            D.nSlots, (int32_t)D.rounds.size(), D.NPT, D.U, (int32_t)D.penBase, (int32_t)D.tokBase, (int32_t)D.ringBase, (int32_t)D.dummyAddr, (int32_t)D.ldsBytes,
                            (int32_t)D.fields.size(), D.nWords, D.level | (D.IP << 8) | (D.ring << 20)};
    ok = ok && fwrite(ph, sizeof(ph), 1, f) == 1;
    for (const WideJitSlot &sl : D.slots) { const int32_t v[2] = {sl.anyPen, sl.anyW2}; ok = ok && fwrite(v, sizeof(v), 1, f) == 1; }
    for (const WideJitRound &R : D.rounds) {
      int32_t mask = 0;      // the lane-group sizes the round's switch has a case for
      for (int g : R.gWaves) mask |= g;
      const int32_t v[8] = {R.firstSlot, R.depth, R.sync, R.uniform, R.gAll, R.anyMixed, R.resultLane, mask};
      ok = ok && fwrite(v, sizeof(v), 1, f) == 1;
    }
    for (const WideJitField &fd : D.fields) { const int32_t v[4] = {fd.kind, fd.index, fd.cm, fd.words}; ok = ok && fwrite(v, sizeof(v), 1, f) == 1; }
    std::vector<uint32_t> tab, stream;
    wide_jit_table(D, F, tab, &stream);
    ok = ok && fwrite(tab.data(), 4, tab.size(), f) == tab.size();
    if (D.level >= 1) ok = ok && fwrite(stream.data(), 4, stream.size(), f) == stream.size();      // [NB][IP][lanes] packed address words
    if (in.part) ok = ok && fwrite(in.gmap + in.S, 4, (size_t)in.nImp, f) == (size_t)in.nImp;      // the exchange columns of the imports
  }
  fclose(f);
  if (!ok) { set_error("mb_debug_wide_jit: short write"); return 1; }
  if (compile) {
    if (FILE *g = fopen((std::string(path) + ".co").c_str(), "wb")) { fwrite(obj.data(), 1, obj.size(), g); fclose(g); }
  }
  return 0;
}

// generated source of the small-machine family's sweep (mode: 0 sum, 1 max, 2 traceback bytes, 3 counts); host only
int mb_debug_small_source(int32_t nStates, int32_t nInTok, int32_t nOutTok, int64_t nTrans, const uint32_t *src, const uint32_t *dst,
                          const uint16_t *inTok, const uint16_t *outTok, const double *logWeight, int mode, int backward,
                          int materialise, const char *path) {
  ApiLock lock;
  const bool dumpProgram = (mode & 32) != 0;      // the PROGRAM instead of the source (see below)
  mode &= 31;
  if (nStates <= 0 || nTrans < 0 || !path || mode < 0 || mode >= SM_NMODE) { set_error("mb_debug_small_source: bad argument"); return 1; }
  mb_machine m;
  m.S = nStates; m.nIn = nInTok; m.nOut = nOutTok; m.nTrans = nTrans;
  m.src.assign(src, src + nTrans); m.dst.assign(dst, dst + nTrans);
  m.inTok.assign(inTok, inTok + nTrans); m.outTok.assign(outTok, outTok + nTrans);
  m.logW.assign(logWeight, logWeight + nTrans);
  std::string err;
  if (!compile_machine(&m, &err)) { set_error(err); return 1; }
  SmallProgram P;
  if (!small_build_host(&m, backward != 0, P)) { set_error("machine does not qualify for the small-machine family"); return 1; }
  if (dumpProgram) {
    // what the generator unrolls, for a device-free replay (tests/test_small_plan.py): 20 int32 (magic 0x534D5031, S, nIn, nOut,
    // backward, seed state, end state, table entries, off[0..3], nTab[0..3], candidates, 3 x 0), the evaluation order [S], decOff
    // [S + 1], the candidates (T, src, dup, tab) in the reference's enumeration order, then w[] (fp64) and eid[] (int32)
    FILE *f = fopen(path, "wb");
    if (!f) { set_error("mb_debug_small_source: cannot open output file"); return 1; }
    std::vector<int32_t> cands;
    for (int d = 0; d < P.S; ++d) for (const SmSlot &sl : P.cand[d]) { cands.push_back(sl.T); cands.push_back(sl.src); cands.push_back(sl.dup); cands.push_back(sl.tab); }
    const int32_t head[20] = {0x534D5031, P.S, P.nIn, P.nOut, P.backward ? 1 : 0, P.seedState, P.endState, (int32_t)P.nEntries, (int32_t)P.off[0], (int32_t)P.off[1],
                              (int32_t)P.off[2], (int32_t)P.off[3], P.nTab[0], P.nTab[1], P.nTab[2], P.nTab[3], (int32_t)(cands.size() / 4), 0, 0, 0};
    const bool ok = fwrite(head, sizeof(head), 1, f) == 1 && fwrite(P.order.data(), 4, P.order.size(), f) == P.order.size() &&
                    fwrite(P.decOff.data(), 4, P.decOff.size(), f) == P.decOff.size() && fwrite(cands.data(), 4, cands.size(), f) == cands.size() &&
                    fwrite(P.w.data(), 8, P.w.size(), f) == P.w.size() && fwrite(P.eid.data(), 4, P.eid.size(), f) == P.eid.size();
    fclose(f);
    if (!ok) { set_error("mb_debug_small_source: short write"); return 1; }
    return 0;
  }
  const std::string code = small_jit_source(P, mode, (materialise & 1) != 0, (materialise & 2) != 0);   // bit 1: the restricted-envelope variant
  FILE *f = fopen(path, "w");
  if (!f) { set_error("mb_debug_small_source: cannot open output file"); return 1; }
  fprintf(f, "// ldsBytes=%zu H=%d NBD=%d tables: silent %d input %d output %d match %d\n", small_jit_lds_bytes(P, mode), P.H, P.NBD,
          P.nTab[3], P.nTab[1], P.nTab[2], P.nTab[0]);
  fputs(code.c_str(), f);
  fclose(f);
  return 0;
}

}  // extern "C"
