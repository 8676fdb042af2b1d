"""`boss`-compatible command line for the inference surface, backed by the HIP engine.

    python -m machineboss_amd.boss MACHINE.json [--preset NAME] [-P params.json] [-F funcs.json] [-N constraints.json]
           [-D seqpairs.json] [--input-chars S] [--output-chars S] [--input-fasta F] [--output-fasta F]
           [--input-json F] [--output-json F] [--use-defaults] [-L] [-V] [-A] [-C] [-T] [-R width]
           [--generate-json F] [--generate-csv F] [--recognize-csv F [--prefix-decode] [--viterbi-decode] [--profile-band N]]
           [--recognize-merge-csv F [--viterbi-decode]]
           [--prefix-decode] [--prefix-encode] [--prefix-backtrack N] [--viterbi-decode] [--viterbi-encode]
           [--random-encode] [--seed N] [--decode-backend device|numpy] [--decode-nodes N]

Restates the data-handling and inference section of /root/reference/target/boss.cpp:716-847 -- how sequences are
collected into pairs, how parameters are assembled, and the exact output text of --loglike / --viterbi / --align /
--counts / --train -- around the batched GPU calls.  The real `boss` needs Boost and cannot run on the GPU box; the
machine-expression language of its command line is reduced to what assembles the benchmark machines: several
transducer files / presets on one command line are COMPOSED (algebra.py = Machine::compose); the other operators
(concatenate, union, Kleene closures, ...) are not here.

``--recognize-csv FILE`` puts a profile (a soft output sequence, src/csv.cpp) behind the machines.  The reference composes
it as an (L+1)-state recogniser; here the composed left part, which must have an empty input alphabet, is scored natively
against the profile (profile.py, mb_profile.hip) with -L, -V or -C, and prints what the reference prints.  With
``--prefix-decode`` or ``--viterbi-decode`` the left part keeps its input alphabet and the most likely INPUT given the profile is
imputed (prefixtree.ProfilePrefixDP, k_prefix_fill_profile in mb_prefix.hip; docs/decoding.md).
``--recognize-merge-csv FILE`` reads the same file as a CTC profile (CSVProfile::mergingMachine, src/csv.cpp:20-46): a symbol
repeated in consecutive rows is one symbol, and only a blank separates two equal symbols.  It goes wherever ``--recognize-csv``
goes except with ``--prefix-decode`` (profile.MergedProfileDP, mb_profile_merge.hip; docs/profile_tapes.md); the prefix search
against a merged profile is ``prefixDecodeProfile(..., merge=True)`` (k_prefix_fill_merged, docs/decoding.md).
``--profile-posteriors`` beside either, alone or after -L, -V and -C, prints the gradient of the log-likelihood in the profile's
rows (``profilePosteriors``, k_profile_rowpost in mb_profile_post.hip; docs/profile_tapes.md, "Row posteriors of one-tape profiles").

``--generate-csv A.csv`` beside ``--recognize-csv B.csv`` (with -L, -V, -C or --profile-posteriors) scores a machine that keeps its input alphabet
between two profiles, A the soft input and B the soft output, without composing A's generator in front (profile.TwoProfileDP,
mb_profile_two.hip; docs/profile_tapes.md, "Pairs of profiles"); ``scoreTwoProfiles`` is the same for a batch of input profiles.

``--prefix-decode`` imputes the most likely INPUT for each given output by the reference's prefix search (src/ctc.cpp), its
node fills on the device (prefixtree.py, mb_prefix.hip, docs/decoding.md); ``--prefix-encode`` the most likely OUTPUT for each
given input (the same search on the transposed machine), ``--random-encode`` samples one; ``--viterbi-decode / --viterbi-encode``
read the answer off the Viterbi path of the input-silenced machine (target/boss.cpp:850-921).  All print a SeqPairList.

Numbers print like C++ `ostream << double` (6 significant digits, target/boss.cpp:794-807 via src/jsonio.h:14-22),
parameters with 15 (src/weight.cpp:483).  Work is batched: all pairs go through one device call per mode; with
torch.distributed initialised (torchrun) the pairs are sharded over ranks, --train/--counts all-reduce their counts
(RCCL) and rank 0 prints.
"""
from __future__ import annotations

import argparse
import json
import math
import os
import sys
from typing import Any, Dict, List, Optional, Tuple

from .evalmachine import EvaluatedMachine
from .machine import Constraints, Machine, MachineError
from .seqpair import SeqPair, seqPairListFromJson

PRESET_DIRS = [os.environ.get("MB_PRESET_DIR", ""), os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))),
                                                                  "tests", "golden", "preset")]


def fmt(x: float) -> str:
    """toInfinitySafeString (src/jsonio.h:14-22): `out << x` = %g with 6 significant digits."""
    if x == math.inf:
        return '"Infinity"'
    if x == -math.inf:
        return '"-Infinity"'
    return "%g" % x


def fmtParam(x: Any) -> str:
    """WeightAlgebra::toJsonStream for constants (src/weight.cpp:471-484): 0, 1, ints, doubles at 15 digits."""
    if isinstance(x, bool):
        return "1" if x else "0"
    if isinstance(x, (int, float)):
        if x == 0:
            return "0"
        if x == 1:
            return "1"
        if isinstance(x, int):
            return str(x)
        return "%.15g" % x
    return json.dumps(x, separators=(",", ":"))


def escaped(s: str) -> str:
    return json.dumps(s)[1:-1]


def readFasta(path: str) -> List[Tuple[str, str]]:
    out: List[Tuple[str, str]] = []
    name, seq = None, []
    with open(path) as f:
        for line in f:
            line = line.strip()
            if line.startswith(">"):
                if name is not None:
                    out.append((name, "".join(seq)))
                name, seq = line[1:].split()[0] if len(line) > 1 else "", []
            elif line and name is not None:
                seq.append(line)
    if name is not None:
        out.append((name, "".join(seq)))
    return out


def seqPairJson(sp: SeqPair) -> str:
    """SeqPair::writeJson (src/seqpair.cpp:40-58)."""
    named = lambda n, s: '{"name":"%s","sequence":[%s]}' % (n, ",".join('"%s"' % x for x in s))
    out = '{"input":' + named(sp.inputName, sp.input) + ',"output":' + named(sp.outputName, sp.output)
    if sp.alignment:
        out += ',"alignment":[' + ",".join('["%s","%s"]' % (escaped(a), escaped(b)) for a, b in sp.alignment) + "]"
    if sp.metadata is not None:
        out += ',"meta":' + json.dumps(sp.metadata, separators=(",", ":"), sort_keys=True)
    return out + "}"


def pathJson(m: Machine, path) -> dict:
    """MachinePath::writeJson (src/machine.cpp:1982-2000) as the JSON object stored under meta.path."""
    j: Dict[str, Any] = {"start": m.startState()}
    if m.state[m.startState()].name is not None:
        j["id"] = m.state[m.startState()].name
    trans = []
    for t in path.trans:
        tj: Dict[str, Any] = {"to": t.dest}
        if m.state[t.dest].name is not None:
            tj["id"] = m.state[t.dest].name
        if t.inp:
            tj["in"] = t.inp
        if t.out:
            tj["out"] = t.out
        trans.append(tj)
    j["trans"] = trans
    return j


def seqPairFromPath(m: Machine, path, inputName: str, outputName: str) -> SeqPair:
    """SeqPair::seqPairFromPath (src/seqpair.cpp:60-89)."""
    ali = [(t.inp, t.out) for t in path.trans if t.inp or t.out]
    return SeqPair([a for a, _ in ali if a], [b for _, b in ali if b], inputName, outputName, ali, {"path": pathJson(m, path)})


def buildParser() -> argparse.ArgumentParser:
    ap = argparse.ArgumentParser(prog="boss", description=__doc__.split("\n\n")[0])
    ap.add_argument("machine", nargs="*", help="transducer JSON file")
    ap.add_argument("--preset", action="append", default=[], help="preset name (dnapsw, protpsw, psw2dna, translate, hamming74); repeatable")
    ap.add_argument("-H", "--hmmer", help="generator from a HMMER3 model file, local alignment mode (target/boss.cpp:574-579); leftmost")
    ap.add_argument("--hmmer-global", help="the same in global alignment mode")
    ap.add_argument("--hmmer-plan7", help="Plan7 generator (single hit, N/C flanks)")
    ap.add_argument("--hmmer-multihit", help="Plan7 generator with the J loop")
    ap.add_argument("--generate-chars", help="compose a generator of this sequence in front of the machine(s)")
    ap.add_argument("--recognize-chars", help="compose a recogniser of this sequence behind the machine(s)")
    ap.add_argument("--generate-json", help="compose a generator of the sequence in this JSON file ({name, sequence}) in front of the machine(s)")
    ap.add_argument("--generate-csv", help="beside --recognize-csv with -L, -V, -C or --profile-posteriors: score the machine(s) between this CSV profile as the soft input and that one as the soft output")
    ap.add_argument("--recognize-csv", help="score the machine(s) against this CSV profile (rightmost; with -L, -V or -C), or decode it (--prefix-decode, --viterbi-decode)")
    ap.add_argument("--profile-band", type=int, metavar="N", help="with --recognize-csv beside an input sequence: sweep each pair under a band of half-width N around the diagonal (seqpair.Envelope.band)")
    ap.add_argument("--profile-posteriors", action="store_true", help="with --recognize-csv beside an input sequence: per pair the posterior probability that each row of the profile was consumed as each output symbol, column 0 the blank (the gradient of the log-likelihood in the profile); beside --generate-csv: the same for the rows of both profiles; with --recognize-csv or --recognize-merge-csv alone on a machine with an empty input alphabet: the same for the one profile (merged: per CSV column)")
    ap.add_argument("--recognize-merge-csv", help="the same against a CTC profile: a symbol repeated in consecutive rows is one symbol, and only a blank separates two equal symbols (not with --prefix-decode)")
    ap.add_argument("-P", "--params", action="append", default=[])
    ap.add_argument("-F", "--functions", action="append", default=[])
    ap.add_argument("-N", "--constraints", action="append", default=[])
    ap.add_argument("-D", "--data", action="append", default=[])
    ap.add_argument("--use-defaults", action="store_true")
    ap.add_argument("--input-chars"); ap.add_argument("--output-chars")
    ap.add_argument("--input-fasta"); ap.add_argument("--output-fasta")
    ap.add_argument("--input-json"); ap.add_argument("--output-json")
    ap.add_argument("-L", "--loglike", action="store_true")
    ap.add_argument("-V", "--viterbi", action="store_true")
    ap.add_argument("-A", "--align", action="store_true")
    ap.add_argument("-C", "--counts", action="store_true")
    ap.add_argument("-T", "--train", action="store_true")
    ap.add_argument("-R", "--wiggle-room", type=int)
    ap.add_argument("--prefix-decode", action="store_true", help="most likely input for each output, by prefix search")
    ap.add_argument("--prefix-encode", action="store_true", help="most likely output for each input, by prefix search")
    ap.add_argument("--prefix-backtrack", type=int, help="purge open prefixes more than N symbols shorter than the longest")
    ap.add_argument("--viterbi-decode", action="store_true", help="input of the Viterbi path for each output")
    ap.add_argument("--viterbi-encode", action="store_true", help="output of the Viterbi path for each input")
    ap.add_argument("--random-encode", action="store_true", help="sample an output for each input")
    ap.add_argument("--seed", type=int, help="random number seed")
    ap.add_argument("--decode-backend", choices=("device", "numpy"), default=os.environ.get("MB_DECODE_BACKEND") or "device",
                    help="who fills the search lattices: the HIP kernels (default) or the numpy restatement")
    ap.add_argument("--decode-nodes", type=int, help="size of the node pool of a prefix search (lattices of 2 (L+1) S doubles)")
    return ap


def loadPreset(name: str) -> Machine:
    for d in PRESET_DIRS:
        p = os.path.join(d, name + ".json")
        if d and os.path.exists(p):
            return Machine.fromFile(p)
    raise MachineError("Unknown preset %s" % name)


def loadMachine(args) -> Machine:
    """Several machines on one command line are composed, right to left (target/boss.cpp:268-276, 628-634); presets come
    first, in the order given."""
    from .algebra import composeAll, generator, recognizer
    machines = [loadPreset(n) for n in args.preset] + [Machine.fromFile(f) for f in args.machine]
    from .hmmer import HmmerModel               # profile generators go in front of the transducers (target/boss.cpp:574-600)
    for path, build in ((args.hmmer, lambda h: h.machine(True)), (args.hmmer_global, lambda h: h.machine(False)),
                        (args.hmmer_plan7, lambda h: h.plan7Machine(False)), (args.hmmer_multihit, lambda h: h.plan7Machine(True))):
        if path is not None:
            machines.insert(0, build(HmmerModel.fromFile(path)))
    if args.generate_chars is not None:       # leftmost: a generator of the sequence (target/boss.cpp:362-364)
        machines.insert(0, generator(list(args.generate_chars), args.generate_chars))
    if args.generate_json is not None:        # leftmost, like --generate-chars (target/boss.cpp:355-357)
        j = json.load(open(args.generate_json))
        machines.insert(0, generator(list(j["sequence"]), j.get("name", "")))
    if args.recognize_chars is not None:      # rightmost: a recogniser of the sequence (target/boss.cpp:384-386)
        machines.append(recognizer(list(args.recognize_chars), args.recognize_chars))
    if not machines:
        raise MachineError("Please specify a transducer")
    return composeAll(machines)


def collectData(args, machine: Machine, inferenceRequested: bool, encoding: bool = False, decoding: bool = False) -> List[SeqPair]:
    """target/boss.cpp:716-773."""
    data: List[SeqPair] = []
    for f in args.data:
        data += seqPairListFromJson(json.load(open(f)))
    inSeqs: List[Tuple[str, List[str]]] = []
    outSeqs: List[Tuple[str, List[str]]] = []
    if args.input_fasta:
        inSeqs += [(n, list(s)) for n, s in readFasta(args.input_fasta)]
    if args.input_chars is not None:
        inSeqs.append((args.input_chars, list(args.input_chars)))
    if args.output_fasta:
        outSeqs += [(n, list(s)) for n, s in readFasta(args.output_fasta)]
    if args.output_chars is not None:
        outSeqs.append((args.output_chars, list(args.output_chars)))
    if args.input_json:
        j = json.load(open(args.input_json)); inSeqs.append((j.get("name", ""), list(j["sequence"])))
    if args.output_json:
        j = json.load(open(args.output_json)); outSeqs.append((j.get("name", ""), list(j["sequence"])))
    inputEmpty, outputEmpty = not machine.inputAlphabet(), not machine.outputAlphabet()
    if not inSeqs and ((inputEmpty and ((outputEmpty and inferenceRequested) or outSeqs)) or encoding or decoding):
        inSeqs.append(("", []))
    if not outSeqs and ((inSeqs and outputEmpty) or encoding):
        outSeqs.append(("", []))
    for iname, iseq in inSeqs:
        for oname, oseq in outSeqs:
            data.append(SeqPair(iseq, oseq, iname, oname))
    if inferenceRequested and not data and inputEmpty and outputEmpty:
        data.append(SeqPair([], [], "", ""))
    return data


_GROUP = None      # shard.RankGroup of this process when launched as one rank of several (main() opens it)


def _dist():
    try:
        import torch.distributed as dist
        if dist.is_available() and dist.is_initialized():
            return dist
    except Exception:
        pass
    return None


def _reduce_counts(counts, loglike):
    """Sum of the E-step statistics over the ranks (MachineCounts::operator+=, src/counts.cpp:66-71): RCCL through the C-ABI when
    main() opened the ranks (shard.RankGroup), torch.distributed's own group when a host program opened one."""
    if _GROUP is not None:
        return _GROUP.allreduce_counts(counts, loglike)
    from .shard import allreduce_counts
    import torch
    return allreduce_counts(counts, loglike, "cuda" if (torch.cuda.is_available() and _dist().get_backend() == "nccl") else "cpu")


def _shard(data: List[Any], machine, world: int) -> List[List[int]]:
    """Which pairs each rank takes: sorted by DP cell count and dealt greedily to the least loaded rank
    (shard.lpt_assign) -- pairs are independent units (the `for seqPair` loops of target/boss.cpp:796,826), and a ragged list
    dealt round-robin leaves the rank that drew the long pairs working alone.  Deterministic: every rank computes the same."""
    from .shard import lpt_assign
    nStates = len(machine.state)
    cells = [(len(sp.input) + 1) * (len(sp.output) + 1) * nStates for sp in data]
    return lpt_assign(cells, world)


def _gather_in_order(local: List[Any], n: int, rank: int, world: int, owned: Optional[List[List[int]]] = None) -> List[Any]:
    """Results of the sharded pairs back in input order on every rank (no data-path collective: host gather).
    owned[r] = indices of the pairs rank r took, in the order it processed them."""
    dist = _dist()
    if dist is None or world == 1:
        return local
    parts: List[Any] = [None] * world
    dist.all_gather_object(parts, local)
    out: List[Any] = [None] * n
    for r in range(world):
        for k, v in zip(owned[r] if owned is not None else range(r, n, world), parts[r]):
            out[k] = v
    return out


def _profileParams(args, machine: Machine) -> Dict[str, Any]:
    params: Dict[str, Any] = {}
    for f in args.functions:
        params.update(json.load(open(f)))
    for f in args.params:
        params.update(json.load(open(f)))
    for k, v in machine.getParamDefs(args.use_defaults).items():
        params.setdefault(k, v)
    return params


def runProfileDecode(args, out) -> int:
    """--recognize-csv with --prefix-decode / --viterbi-decode: the most likely input of the machines left of the profile given
    the profile.  Prints what the reference prints for the composed machine, whose output tape is empty."""
    from . import algebra, prefixtree
    from .profile import Profile
    if args.prefix_encode or args.viterbi_encode or args.random_encode:
        raise MachineError("--recognize-csv cannot be encoded: the profile is an output; use --prefix-decode or --viterbi-decode")
    if args.loglike or args.viterbi or args.counts or args.align or args.train:
        raise MachineError("--recognize-csv decodes (--prefix-decode, --viterbi-decode) or scores (-L, -V, -C), not both in one run")
    if args.recognize_chars is not None or args.data or args.input_chars is not None or args.output_chars is not None or \
            args.input_fasta or args.output_fasta or args.input_json or args.output_json:
        raise MachineError("--recognize-csv takes no other sequence data: the profile is the output to decode")
    if _dist() is not None and _dist().get_world_size() > 1:
        raise MachineError("--recognize-csv runs on one rank")
    if args.merge and args.prefix_decode:
        # (the fill exists: prefixDecodeProfile(..., merge=True).  The spelling stays rejected, message and all, while the test that
        # pins it stands -- docs/decoding.md, "Decoding against a merged profile")
        raise MachineError("--recognize-merge-csv cannot be prefix-decoded: there is no merged prefix fill; use --viterbi-decode")
    machine = loadMachine(args)
    if not os.path.exists(args.recognize_csv):
        raise MachineError("CSV file not found")
    profile = Profile.fromCsv(args.recognize_csv)
    params = _profileParams(args, machine)
    decoded: List[List[str]] = []
    if args.prefix_decode:
        maxBacktrack = args.prefix_backtrack if args.prefix_backtrack is not None else prefixtree.NO_BACKTRACK_LIMIT
        ev = EvaluatedMachine.fromMachine(machine, params)
        decoded.append(prefixtree.decodeBatch(ev, None, maxBacktrack, args.decode_backend, args.decode_nodes, profiles=[profile])[0][0])
    if args.viterbi_decode:
        decoded.append(viterbiDecodeProfile(machine, profile, args.decode_backend, params, args.merge))
    for d in decoded:
        out.write("[" + seqPairJson(SeqPair(d, [], "input", "")) + "]\n")
    return 0


def viterbiDecodeProfile(machine: Machine, profile, backend: str = "device", params=None, merge: bool = False) -> List[str]:
    """--viterbi-decode against a profile: the Viterbi path of the input-silenced machine through the profile (the existing
    profile Viterbi with paths), then the input symbols of the heaviest matching transitions of the machine itself.  ``merge``:
    the profile is CTC-merged (--recognize-merge-csv; a Profile, or a pair (logP, colTok) as Profile.mergeRows returns)."""
    from . import algebra, dp
    params = machine.getParamDefs(True) if params is None else params
    silent = algebra.silenceInput(machine)
    ev = EvaluatedMachine.fromMachine(silent, params)
    colTok = None
    if merge:
        P, colTok = _mergedRows(profile, ev) if hasattr(profile, "mergeRows") else profile
    else:
        P = profile.logRows(ev) if hasattr(profile, "logRows") else profile
    if backend == "numpy":
        from .profile import MergedProfileDP, ProfileDP
        v, edges, _ = (MergedProfileDP(ev, colTok) if merge else ProfileDP(ev)).viterbi(P)
    else:
        from . import capi
        dm = capi.DeviceMachine(ev)
        prof = capi.DeviceProfiles(dm, [P], colTok)
        try:
            ll, off, e, _ = prof.viterbi(paths=True)
        finally:
            prof.close(); dm.close()
        v, edges = float(ll[0]), e[off[0]:off[1]]
    if not v > -math.inf:
        raise MachineError("Can't do traceback: no finite-weight paths")
    return algebra.decodePath(dp.edgesToPath(ev, silent, edges), machine, params)


def prefixDecodeProfile(machine: Machine, profile, backend: str = "device", params=None, merge: bool = False,
                        maxBacktrack: Optional[int] = None, maxNodes: Optional[int] = None) -> List[str]:
    """--prefix-decode against a profile: the most likely input of the machine given the profile, by prefix search with native node
    fills.  ``merge``: the profile is CTC-merged (a Profile, or a pair (logP, colTok) as Profile.mergeRows returns;
    prefixtree.MergedProfilePrefixDP, k_prefix_fill_merged).  ``maxBacktrack`` None: no limit."""
    from . import prefixtree
    params = machine.getParamDefs(True) if params is None else params
    ev = EvaluatedMachine.fromMachine(machine, params)
    colTok = None
    if merge:
        profile, colTok = _mergedRows(profile, ev) if hasattr(profile, "mergeRows") else profile
    limit = prefixtree.NO_BACKTRACK_LIMIT if maxBacktrack is None else maxBacktrack
    return prefixtree.decodeBatch(ev, None, limit, backend, maxNodes, profiles=[profile], colTok=colTok)[0][0]


def _mergedRows(profile, ev):
    """Profile.mergeRows for the device: (logP, colTok) with at least one column.  A header none of whose symbols the machine
    emits leaves only the blank; a column of weight 0 for the machine's first token says the same."""
    import numpy as np
    P, colTok = profile.mergeRows(ev)
    if len(colTok) == 0 and ev.nOutTok:
        P, colTok = np.concatenate([P, np.full((len(P), 1), -math.inf)], axis=1), np.array([1], np.int32)
    return P, colTok


def runProfile(args, out) -> int:
    """--recognize-csv / --recognize-merge-csv: the machines left of the profile, composed, against the profile tape (-L / -V /
    -C, and --profile-posteriors after them or alone: [["","",rows]], profilePosteriors).  With --decode-backend numpy a merged
    profile is swept by the numpy restatement (profile.MergedProfileDP), and the posteriors of either kind by the yardstick."""
    from . import capi, dp
    from .profile import Profile
    args.merge = args.recognize_merge_csv is not None
    if args.merge:
        if args.recognize_csv is not None:
            raise MachineError("--recognize-csv and --recognize-merge-csv cannot be combined: the profile is one file, read one way")
        args.recognize_csv = args.recognize_merge_csv
    if args.prefix_decode or args.viterbi_decode or args.prefix_encode or args.viterbi_encode or args.random_encode:
        return runProfileDecode(args, out)
    if args.align or args.train:
        raise MachineError("--recognize-csv supports -L, -V and -C")
    if not (args.loglike or args.viterbi or args.counts or args.profile_posteriors):
        raise MachineError("--recognize-csv needs -L, -V or -C")
    if args.recognize_chars is not None or args.data or args.output_chars is not None or args.output_fasta or args.output_json:
        raise MachineError("--recognize-csv takes no other sequence data")
    hasInput = args.input_chars is not None or bool(args.input_fasta) or bool(args.input_json)
    if hasInput and args.merge:
        raise MachineError("--recognize-merge-csv takes no input sequence: two-tape sweeps take plain profiles (--recognize-csv)")
    if _dist() is not None and _dist().get_world_size() > 1:
        raise MachineError("--recognize-csv runs on one rank")
    machine = loadMachine(args)
    if hasInput:
        if not machine.inputAlphabet():
            raise MachineError("--recognize-csv takes no other sequence data: the machine has no input alphabet to read an input sequence")
        return _runProfilePairs(args, out, machine)
    if args.generate_csv is not None:
        return _runTwoProfiles(args, out, machine)
    if args.profile_posteriors and machine.inputAlphabet():
        raise MachineError(_POSTERIORS_ONLY)
    if args.profile_band is not None:
        raise MachineError(_BAND_ONLY)
    if machine.inputAlphabet():
        raise MachineError("--recognize-csv needs a machine with an empty input alphabet (compose a generator in front); input alphabet: %s"
                           % ",".join(machine.inputAlphabet()))
    if not os.path.exists(args.recognize_csv):
        raise MachineError("CSV file not found")
    profile = Profile.fromCsv(args.recognize_csv)
    params = _profileParams(args, machine)
    ev = EvaluatedMachine.fromMachine(machine, params)
    if args.merge and not ev.nOutTok:
        raise MachineError("--recognize-merge-csv needs a machine with an output alphabet")
    if args.merge and args.decode_backend == "numpy":
        return _runMergedNumpy(args, out, machine, params, ev, profile)
    numpyPost = args.profile_posteriors and args.decode_backend == "numpy"      # the yardstick: no device object for it
    if args.loglike or args.counts or args.viterbi or (args.profile_posteriors and not numpyPost):
        dm = capi.DeviceMachine(ev)
        if args.merge:
            P, colTok = _mergedRows(profile, ev)
            prof = capi.DeviceProfiles(dm, [P], colTok)
        else:
            prof = capi.DeviceProfiles(dm, [profile.logRows(ev)])
        if args.loglike:
            out.write('[["","",%s]]\n' % fmt(prof.forward(capi.MB_ROLLING)[0]))
        if args.counts:
            counts = dp.MachineCounts(ev)
            _, s, _ = prof.counts(counts._flat)
            counts.loglike += s
            pc = counts.paramCounts(machine, params)
            out.write("{" + ",".join('"%s":%s' % (escaped(k), "%g" % pc[k]) for k in sorted(pc)) + "}\n")
        if args.viterbi:
            out.write('[["","",%s]]\n' % fmt(prof.viterbi(paths=False)[0][0]))
        if args.profile_posteriors and not numpyPost:
            _writeProfilePosteriors(out, prof.row_posteriors()[0])
        prof.close(); dm.close()
    if numpyPost:
        _writeProfilePosteriors(out, profilePosteriors(machine, profile, "numpy", params)[0])
    return 0


def _writeProfilePosteriors(out, post) -> None:
    out.write('[["","",[' + ",".join("[" + ",".join(fmt(float(v)) for v in row) + "]" for row in post) + "]]]\n")


def profilePosteriors(machine: Machine, profile, backend: str = "device", params=None, merge: bool = False):
    """--profile-posteriors of a one-tape profile: (post[L, width], loglike) of a machine with an empty input alphabet against the
    profile, post[r][x] the posterior probability that row r was consumed as column x (0: the blank), the gradient of loglike in
    the profile's log weights (docs/profile_tapes.md, "Row posteriors of one-tape profiles"); zeros for a profile that scores
    -inf.  ``profile``: a Profile, or its rows (merged: a pair (logP, colTok) as Profile.mergeRows returns).  ``merge``: the
    profile is CTC-merged and width = nCols + 1, else width = nOutTok + 1.  ``backend``: "device" (capi.DeviceProfiles) or "numpy"
    (profile.ProfileDP / MergedProfileDP)."""
    params = machine.getParamDefs(True) if params is None else params
    if machine.inputAlphabet():
        raise MachineError("--recognize-csv needs a machine with an empty input alphabet (compose a generator in front); input alphabet: %s"
                           % ",".join(machine.inputAlphabet()))
    ev = EvaluatedMachine.fromMachine(machine, params)
    colTok = None
    if merge:
        if not ev.nOutTok:
            raise MachineError("--recognize-merge-csv needs a machine with an output alphabet")
        P, colTok = _mergedRows(profile, ev) if hasattr(profile, "mergeRows") else profile
    else:
        P = profile.logRows(ev) if hasattr(profile, "logRows") else profile
    if backend == "numpy":
        from .profile import MergedProfileDP, ProfileDP
        post, ll = (MergedProfileDP(ev, colTok) if merge else ProfileDP(ev)).rowPosteriors(P)
        return post, float(ll)
    if backend != "device":
        raise MachineError('backend is "device" or "numpy"')
    from . import capi
    dm = capi.DeviceMachine(ev)
    prof = None
    try:
        prof = capi.DeviceProfiles(dm, [P], colTok)
        post, ll = prof.row_posteriors()
    finally:
        if prof is not None:
            prof.close()
        dm.close()
    return post, float(ll[0])


def scoreProfilePairs(machine: Machine, inputs, profile, backend: str = "device", params=None, merge: bool = False,
                      loglike: bool = True, viterbi: bool = False, counts: bool = False, band: Optional[int] = None,
                      posteriors: bool = False):
    """Every input sequence (a list of symbols) as one pair with ``profile`` (a profile.Profile), all pairs in one batch, on a
    machine with an input alphabet (docs/profile_tapes.md, "Pairs" and "Pairs against a merged profile").  ``merge``: the profile
    is read CTC-merged, as --recognize-merge-csv reads it.  ``backend``: "device" (capi.DeviceProfilePairs) or "numpy"
    (profile.PairProfileDP / PairMergedProfileDP).  Returns (scores, paramCounts): scores["loglike"] and scores["viterbi"] hold one
    float per input, or None where not asked for -- a sequence that cannot be tokenised scores -inf and adds nothing to the counts,
    as the --loglike loop (dp.loglikeBatch); paramCounts is the posterior count of every parameter summed over the pairs, or None.
    ``band``: every tokenisable input is swept under seqpair.Envelope.band(len(x), len(profile), band) (docs/profile_tapes.md,
    "Pairs under an envelope"); plain profiles only here -- scoreMergedPairs bands a merged profile.  ``posteriors``: scores["posteriors"] holds one [rows, nOutTok + 1] array per
    input, the posterior probability that each row was consumed as each output token (column 0: as the blank; docs/profile_tapes.md,
    "Row posteriors") -- zeros for an input that cannot be tokenised or scores -inf; plain profiles only (merged: scoreMergedPairs); the key is absent when not
    asked for."""
    import numpy as np
    from . import dp
    from .profile import PairMergedProfileDP, PairProfileDP
    from .seqpair import Envelope
    ev = EvaluatedMachine.fromMachine(machine, params)
    if merge and not ev.nOutTok:
        raise MachineError("--recognize-merge-csv needs a machine with an output alphabet")
    if band is not None and merge:
        raise MachineError("envelopes take plain profiles")
    if posteriors and merge:
        raise MachineError("row posteriors take plain profiles")
    ok = [ev.inputTokenizer.canTokenize(seq) for seq in inputs]
    xs = [np.asarray(ev.inputTokenizer.tokenize(seq), np.int64).reshape(-1) for seq, k in zip(inputs, ok) if k]
    P, colTok = _mergedRows(profile, ev) if merge else (profile.logRows(ev), None)
    acc = dp.MachineCounts(ev)
    fwd = vit = post = None
    envs = None if band is None else [Envelope.band(len(x), len(P), int(band)) for x in xs]
    if backend == "numpy" and envs is not None:
        pdp = PairProfileDP(ev)
        fwd = [pdp.forward(x, P, env=e)[0] for x, e in zip(xs, envs)] if loglike else None
        if counts:
            for x, e in zip(xs, envs):
                c, ll = pdp.counts(x, P, env=e)
                acc._flat += c
                acc.loglike += ll
        vit = [pdp.forward(x, P, "max", env=e)[0] for x, e in zip(xs, envs)] if viterbi else None
        post = [pdp.rowPosteriors(x, P, env=e)[0] for x, e in zip(xs, envs)] if posteriors else None
    elif backend == "numpy":
        pdp = PairMergedProfileDP(ev, colTok) if merge else PairProfileDP(ev)
        fwd = [pdp.forward(x, P)[0] for x in xs] if loglike else None
        if counts:
            for x in xs:
                c, ll = pdp.counts(x, P)
                acc._flat += c
                acc.loglike += ll
        vit = [pdp.forward(x, P, "max")[0] for x in xs] if viterbi else None
        post = [pdp.rowPosteriors(x, P)[0] for x in xs] if posteriors else None
    else:
        from . import capi
        dm = capi.DeviceMachine(ev)
        pairs = capi.DeviceProfilePairs(dm, xs, [P] * len(xs), colTok) if merge else capi.DeviceProfilePairs(dm, xs, [P] * len(xs))
        try:
            if envs is not None:
                pairs.set_envelopes(envs)
            fwd = pairs.forward(capi.MB_ROLLING) if loglike else None
            if counts:
                _, s, _ = pairs.counts(acc._flat)
                acc.loglike += s
            vit = pairs.viterbi(paths=False)[0] if viterbi else None
            if posteriors:
                flat = pairs.row_posteriors()[0]
                post = [flat[k * len(P):(k + 1) * len(P)] for k in range(len(xs))]
        finally:
            pairs.close(); dm.close()

    def spread(v):
        if v is None:
            return None
        it = iter(v)
        return [float(next(it)) if k else -math.inf for k in ok]
    scores = {"loglike": spread(fwd), "viterbi": spread(vit)}
    if posteriors:
        it = iter(post)
        scores["posteriors"] = [np.array(next(it)) if k else np.zeros(P.shape) for k in ok]
    return scores, (acc.paramCounts(machine, params) if counts else None)


def sampleProfilePairs(machine: Machine, inputs, profile, nSamples: int, seed: int = 0, backend: str = "device", params=None,
                       band: Optional[int] = None):
    """``nSamples`` alignments of every input sequence with ``profile`` drawn from the posterior (docs/profile_tapes.md,
    "Posterior path samples"), the pairs of scoreProfilePairs in one batch.  Returns (paths, logq, loglike): paths[k][j] is sample j
    of input k as a MachinePath (dp.edgesToPath), logq[k][j] its log posterior probability -- the path's own log weight minus
    loglike[k] -- and loglike[k] the Forward log-likelihood.  An input that cannot be tokenised, or scores -inf, gets empty paths
    and logq = -inf.  A sample depends on (seed, the input's index among the tokenisable ones, j) alone.  ``backend``: "device"
    (capi.DeviceProfilePairs.sample_paths) or "numpy" (profile.PairProfileDP.samplePaths).  ``band``: as scoreProfilePairs."""
    import numpy as np
    from . import dp
    from .profile import PairProfileDP
    from .seqpair import Envelope
    if backend not in ("device", "numpy"):
        raise MachineError('backend is "device" or "numpy"')
    nSamples = int(nSamples)
    if nSamples < 1:
        raise MachineError("nSamples must be at least 1")
    ev = EvaluatedMachine.fromMachine(machine, params)
    ok = [ev.inputTokenizer.canTokenize(seq) for seq in inputs]
    xs = [np.asarray(ev.inputTokenizer.tokenize(seq), np.int64).reshape(-1) for seq, k in zip(inputs, ok) if k]
    P = profile.logRows(ev)
    envs = None if band is None else [Envelope.band(len(x), len(P), int(band)) for x in xs]
    if backend == "numpy":
        pdp = PairProfileDP(ev)
        ll, got = [], []
        for k, x in enumerate(xs):
            l, samples = pdp.samplePaths(x, P, nSamples, seed=seed, pair=k, env=None if envs is None else envs[k])
            ll.append(l); got.append([(e, q) for e, _r, q in samples])
    else:
        from . import capi
        dm = capi.DeviceMachine(ev)
        pairs = capi.DeviceProfilePairs(dm, xs, [P] * len(xs))
        try:
            if envs is not None:
                pairs.set_envelopes(envs)
            ll, off, edges, _rows, lq = pairs.sample_paths(nSamples, seed=seed)
        finally:
            pairs.close(); dm.close()
        got = [[(edges[off[k * nSamples + j]:off[k * nSamples + j + 1]], lq[k * nSamples + j]) for j in range(nSamples)] for k in range(len(xs))]
    it = iter(zip(ll, got))
    paths, logq, loglike = [], [], []
    for good in ok:
        l, samples = next(it) if good else (-math.inf, [(np.zeros(0, np.uint32), -math.inf)] * nSamples)
        paths.append([dp.edgesToPath(ev, machine, e) for e, _q in samples])
        logq.append([float(q) for _e, q in samples])
        loglike.append(float(l))
    return paths, logq, loglike


def scoreMergedPairs(machine: Machine, inputs, profile, backend: str = "device", params=None, loglike: bool = True,
                     viterbi: bool = False, counts: bool = False, posteriors: bool = False, band: Optional[int] = None):
    """scoreProfilePairs for a profile read CTC-merged (a profile.Profile, or a pair (logP[L, nCols + 1], colTok) as
    Profile.mergeRows returns), with everything the merged pairs have: the same return shape, (scores, paramCounts).  ``band``:
    every tokenisable input is swept under seqpair.Envelope.band(len(x), rows, band) (docs/profile_tapes.md, "Pairs against a merged
    profile under an envelope").  ``posteriors``: scores["posteriors"] holds one [rows, nCols + 1] array per input, the posterior
    probability that each row was consumed as each column (column 0: as the blank) -- zeros for an input that cannot be tokenised
    or scores -inf; the key is absent when not asked for.  ``backend``: "device" (capi.DeviceProfilePairs with colTok) or "numpy"
    (profile.PairMergedProfileDP)."""
    import numpy as np
    from . import dp
    from .profile import PairMergedProfileDP
    from .seqpair import Envelope
    if backend not in ("device", "numpy"):
        raise MachineError('backend is "device" or "numpy"')
    ev = EvaluatedMachine.fromMachine(machine, params)
    if not ev.nOutTok:
        raise MachineError("--recognize-merge-csv needs a machine with an output alphabet")
    P, colTok = _mergedRows(profile, ev) if hasattr(profile, "mergeRows") else profile
    P = np.asarray(P, np.float64).reshape(-1, len(colTok) + 1)
    ok = [ev.inputTokenizer.canTokenize(seq) for seq in inputs]
    xs = [np.asarray(ev.inputTokenizer.tokenize(seq), np.int64).reshape(-1) for seq, k in zip(inputs, ok) if k]
    envs = [None] * len(xs) if band is None else [Envelope.band(len(x), len(P), int(band)) for x in xs]
    acc = dp.MachineCounts(ev)
    fwd = vit = post = None
    if backend == "numpy":
        pdp = PairMergedProfileDP(ev, colTok)
        fwd = [pdp.forward(x, P, env=e)[0] for x, e in zip(xs, envs)] if loglike else None
        if counts:
            for x, e in zip(xs, envs):
                c, ll = pdp.counts(x, P, env=e)
                acc._flat += c
                acc.loglike += ll
        vit = [pdp.forward(x, P, "max", env=e)[0] for x, e in zip(xs, envs)] if viterbi else None
        post = [pdp.rowPosteriors(x, P, env=e)[0] for x, e in zip(xs, envs)] if posteriors else None
    else:
        from . import capi
        dm = capi.DeviceMachine(ev)
        pairs = None
        try:
            pairs = capi.DeviceProfilePairs(dm, xs, [P] * len(xs), colTok)
            if band is not None:
                pairs.set_merged_envelopes(envs)
            fwd = pairs.forward(capi.MB_ROLLING) if loglike else None
            if counts:
                _, s, _ = pairs.counts(acc._flat)
                acc.loglike += s
            vit = pairs.viterbi(paths=False)[0] if viterbi else None
            if posteriors:
                flat = pairs.merged_row_posteriors()[0]
                post = [flat[k * len(P):(k + 1) * len(P)] for k in range(len(xs))]
        finally:
            if pairs is not None:
                pairs.close()
            dm.close()

    def spread(v):
        if v is None:
            return None
        it = iter(v)
        return [float(next(it)) if k else -math.inf for k in ok]
    scores = {"loglike": spread(fwd), "viterbi": spread(vit)}
    if posteriors:
        it = iter(post)
        scores["posteriors"] = [np.array(next(it)) if k else np.zeros(P.shape) for k in ok]
    return scores, (acc.paramCounts(machine, params) if counts else None)


def sampleMergedPairs(machine: Machine, inputs, profile, nSamples: int, seed: int = 0, backend: str = "device", params=None,
                      band: Optional[int] = None):
    """sampleProfilePairs for a profile read CTC-merged (a profile.Profile, or a pair (logP[L, nCols + 1], colTok) as
    Profile.mergeRows returns): ``nSamples`` lattice paths of every input sequence drawn from the posterior (docs/profile_tapes.md,
    "Posterior path samples of pairs against a merged profile").  Returns (paths, rowCols, logq, loglike): paths[k][j] is sample j of
    input k as a MachinePath (dp.edgesToPath), rowCols[k][j] the column each of the L rows took in it (0: the blank; c: column c,
    fresh or repeated) -- the frame labelling, which with the path determines the lattice path -- logq[k][j] that lattice path's log
    weight minus loglike[k], and loglike[k] the Forward log-likelihood.  An input that cannot be tokenised, or scores -inf, gets empty
    paths, rowCols of -1 and logq = -inf.  A sample depends on (seed, the input's index among the tokenisable ones, j) alone.
    ``backend``: "device" (capi.DeviceProfilePairs.merged_sample_paths) or "numpy" (profile.PairMergedProfileDP.samplePaths).
    ``band``: as scoreMergedPairs."""
    import numpy as np
    from . import dp
    from .profile import PairMergedProfileDP
    from .seqpair import Envelope
    if backend not in ("device", "numpy"):
        raise MachineError('backend is "device" or "numpy"')
    nSamples = int(nSamples)
    if nSamples < 1:
        raise MachineError("nSamples must be at least 1")
    ev = EvaluatedMachine.fromMachine(machine, params)
    if not ev.nOutTok:
        raise MachineError("--recognize-merge-csv needs a machine with an output alphabet")
    P, colTok = _mergedRows(profile, ev) if hasattr(profile, "mergeRows") else profile
    P = np.asarray(P, np.float64).reshape(-1, len(colTok) + 1)
    L = len(P)
    ok = [ev.inputTokenizer.canTokenize(seq) for seq in inputs]
    xs = [np.asarray(ev.inputTokenizer.tokenize(seq), np.int64).reshape(-1) for seq, k in zip(inputs, ok) if k]
    envs = None if band is None else [Envelope.band(len(x), L, int(band)) for x in xs]
    if backend == "numpy":
        pdp = PairMergedProfileDP(ev, colTok)
        ll, got = [], []
        for k, x in enumerate(xs):
            l, samples = pdp.samplePaths(x, P, nSamples, seed=seed, pair=k, env=None if envs is None else envs[k])
            ll.append(l); got.append([(e, c, q) for e, _r, c, q in samples])
    else:
        from . import capi
        dm = capi.DeviceMachine(ev)
        pairs = None
        try:
            pairs = capi.DeviceProfilePairs(dm, xs, [P] * len(xs), colTok)
            if envs is not None:
                pairs.set_merged_envelopes(envs)
            ll, off, edges, _rows, rc, lq = pairs.merged_sample_paths(nSamples, seed=seed)
        finally:
            if pairs is not None:
                pairs.close()
            dm.close()
        rc = rc.reshape(len(xs), nSamples, L)
        got = [[(edges[off[k * nSamples + j]:off[k * nSamples + j + 1]], rc[k, j].copy(), lq[k * nSamples + j]) for j in range(nSamples)]
               for k in range(len(xs))]
    it = iter(zip(ll, got))
    paths, rowCols, logq, loglike = [], [], [], []
    for good in ok:
        l, samples = next(it) if good else (-math.inf, [(np.zeros(0, np.uint32), np.full(L, -1, np.int32), -math.inf)] * nSamples)
        paths.append([dp.edgesToPath(ev, machine, e) for e, _c, _q in samples])
        rowCols.append([np.asarray(c, np.int32) for _e, c, _q in samples])
        logq.append([float(q) for _e, _c, q in samples])
        loglike.append(float(l))
    return paths, rowCols, logq, loglike


def mergedPairPosteriors(machine: Machine, inputs, profile, backend: str = "device", params=None, band: Optional[int] = None):
    """Every input sequence (a list of symbols) as one pair with ``profile`` read CTC-merged (a profile.Profile, or a pair
    (logP[L, nCols + 1], colTok) as Profile.mergeRows returns), all pairs in one batch: (posteriors, loglike), one [L, nCols + 1]
    array and one float per input -- the posterior probability that each row was consumed as each column (column 0: as the blank),
    the gradient of the pair's log-likelihood in the merged rows (docs/profile_tapes.md, "Row posteriors of pairs against a merged
    profile").  An input that cannot be tokenised scores -inf; it and an input that scores -inf get zeros.  ``backend``: "device"
    (capi.DeviceProfilePairs.merged_row_posteriors) or "numpy" (profile.PairMergedProfileDP.rowPosteriors).  ``band``: every
    tokenisable input is swept under seqpair.Envelope.band(len(x), L, band) (docs/profile_tapes.md, "Pairs against a merged profile
    under an envelope")."""
    import numpy as np
    from .profile import PairMergedProfileDP
    from .seqpair import Envelope
    if backend not in ("device", "numpy"):
        raise MachineError('backend is "device" or "numpy"')
    ev = EvaluatedMachine.fromMachine(machine, params)
    if not ev.nOutTok:
        raise MachineError("--recognize-merge-csv needs a machine with an output alphabet")
    P, colTok = _mergedRows(profile, ev) if hasattr(profile, "mergeRows") else profile
    P = np.asarray(P, np.float64).reshape(-1, len(colTok) + 1)
    ok = [ev.inputTokenizer.canTokenize(seq) for seq in inputs]
    xs = [np.asarray(ev.inputTokenizer.tokenize(seq), np.int64).reshape(-1) for seq, k in zip(inputs, ok) if k]
    envs = None if band is None else [Envelope.band(len(x), len(P), int(band)) for x in xs]
    if backend == "numpy":
        pdp = PairMergedProfileDP(ev, colTok)
        res = [pdp.rowPosteriors(x, P) for x in xs] if envs is None else [pdp.rowPosteriors(x, P, env=e) for x, e in zip(xs, envs)]
        post, ll = [r[0] for r in res], [r[1] for r in res]
    else:
        from . import capi
        dm = capi.DeviceMachine(ev)
        pairs = None
        try:
            pairs = capi.DeviceProfilePairs(dm, xs, [P] * len(xs), colTok)
            if envs is not None:
                pairs.set_merged_envelopes(envs)
            flat, ll = pairs.merged_row_posteriors()
            post = [flat[k * len(P):(k + 1) * len(P)] for k in range(len(xs))]
        finally:
            if pairs is not None:
                pairs.close()
            dm.close()
    ip, il = iter(post), iter(ll)
    return [np.array(next(ip)) if k else np.zeros(P.shape) for k in ok], [float(next(il)) if k else -math.inf for k in ok]


def _runProfilePairs(args, out, machine: Machine) -> int:
    """--recognize-csv beside --input-chars / --input-fasta / --input-json on a machine with an input alphabet: every input
    sequence is one pair with the profile (docs/profile_tapes.md, "Pairs"), all pairs in one batch.  -L and -V print one
    [input name, "", score] per pair, -C the counts summed over the pairs.  --decode-backend numpy: profile.PairProfileDP."""
    from .profile import Profile
    if not os.path.exists(args.recognize_csv):
        raise MachineError("CSV file not found")
    profile = Profile.fromCsv(args.recognize_csv)
    params = _profileParams(args, machine)
    inSeqs: List[Tuple[str, List[str]]] = []
    if args.input_fasta:
        inSeqs += [(n, list(s)) for n, s in readFasta(args.input_fasta)]
    if args.input_chars is not None:
        inSeqs.append((args.input_chars, list(args.input_chars)))
    if args.input_json:
        j = json.load(open(args.input_json)); inSeqs.append((j.get("name", ""), list(j["sequence"])))
    sc, pc = scoreProfilePairs(machine, [seq for _, seq in inSeqs], profile, backend="numpy" if args.decode_backend == "numpy" else "device",
                               params=params, loglike=bool(args.loglike), viterbi=bool(args.viterbi), counts=bool(args.counts),
                               band=args.profile_band, posteriors=bool(args.profile_posteriors))

    def scores(v):
        return "[" + ",".join('["%s","",%s]' % (escaped(n), fmt(x)) for (n, _), x in zip(inSeqs, v)) + "]\n"
    if args.loglike:
        out.write(scores(sc["loglike"]))
    if args.counts:
        out.write("{" + ",".join('"%s":%s' % (escaped(k), "%g" % pc[k]) for k in sorted(pc)) + "}\n")
    if args.viterbi:
        out.write(scores(sc["viterbi"]))
    if args.profile_posteriors:
        rows = lambda a: "[" + ",".join("[" + ",".join(fmt(float(v)) for v in row) + "]" for row in a) + "]"
        out.write("[" + ",".join('["%s","",%s]' % (escaped(n), rows(a)) for (n, _), a in zip(inSeqs, sc["posteriors"])) + "]\n")
    return 0


def scoreTwoProfiles(machine: Machine, inProfiles, outProfile, backend: str = "device", params=None,
                     loglike: bool = True, viterbi: bool = False, counts: bool = False, posteriors: bool = False,
                     band: Optional[int] = None, merge: bool = False):
    """Every input profile (a profile.Profile, read against the machine's input alphabet) as one pair with ``outProfile`` (a
    profile.Profile, read against its output alphabet), all pairs in one batch, on a machine with an input alphabet
    (docs/profile_tapes.md, "Pairs of profiles").  ``backend``: "device" (capi.DeviceProfileTwos) or "numpy"
    (profile.TwoProfileDP).  Returns what scoreProfilePairs returns: (scores, paramCounts), scores["loglike"] and
    scores["viterbi"] one float per input profile, or None where not asked for; paramCounts the posterior count of every parameter
    summed over the pairs, or None.  ``posteriors``: scores["posteriors"] holds one (postA[K, nInTok + 1], postB[L, nOutTok + 1]) per
    input profile, the posterior probability that each row of either tape was consumed as each of its tokens (column 0: as the
    blank; docs/profile_tapes.md, "Row posteriors of pairs of profiles") -- zeros for a pair that scores -inf; the key is absent
    when not asked for.  ``band``: every pair is swept under seqpair.Envelope.band(K, L, band), K the rows of its input profile
    and L those of ``outProfile``, on both backends (docs/profile_tapes.md, "Pairs of profiles under an envelope"); a width that
    cannot bridge the slope raises MachineError("Envelope is not connected").  ``merge``: ``outProfile`` is read CTC-merged, as
    --recognize-merge-csv reads it (docs/profile_tapes.md, "Pairs of profiles against a merged profile"; capi.DeviceProfileTwos
    with colTok / profile.TwoMergedProfileDP); plain profiles only for ``band`` and ``posteriors``."""
    import numpy as np
    from . import dp
    from .profile import TwoMergedProfileDP, TwoProfileDP
    from .seqpair import Envelope
    ev = EvaluatedMachine.fromMachine(machine, params)
    if not ev.nInTok:
        raise MachineError("two-profile sweeps need a machine with an input alphabet")
    if merge and not ev.nOutTok:
        raise MachineError("--recognize-merge-csv needs a machine with an output alphabet")
    if band is not None and merge:
        raise MachineError("envelopes take plain profiles")
    if posteriors and merge:
        raise MachineError("row posteriors take plain profiles")
    As = [a.logRowsIn(ev) for a in inProfiles]
    B, colTok = _mergedRows(outProfile, ev) if merge else (outProfile.logRows(ev), None)
    acc = dp.MachineCounts(ev)
    fwd = vit = post = None
    envs = [None] * len(As) if band is None else [Envelope.band(len(A), len(B), int(band)) for A in As]
    if backend == "numpy" and merge:
        tdp = TwoMergedProfileDP(ev, colTok)
        fwd = [tdp.forward(A, B)[0] for A in As] if loglike else None
        if counts:
            for A in As:
                c, ll = tdp.counts(A, B)
                acc._flat += c
                acc.loglike += ll
        vit = [tdp.forward(A, B, "max")[0] for A in As] if viterbi else None
    elif backend == "numpy":
        tdp = TwoProfileDP(ev)
        fwd = [tdp.forward(A, B, env=e)[0] for A, e in zip(As, envs)] if loglike else None
        if counts:
            for A, e in zip(As, envs):
                c, ll = tdp.counts(A, B, env=e)
                acc._flat += c
                acc.loglike += ll
        vit = [tdp.forward(A, B, "max", env=e)[0] for A, e in zip(As, envs)] if viterbi else None
        post = [tdp.rowPosteriors(A, B, env=e)[:2] for A, e in zip(As, envs)] if posteriors else None
    else:
        from . import capi
        dm = capi.DeviceMachine(ev)
        twos = capi.DeviceProfileTwos(dm, As, [B] * len(As), envs=None if band is None else envs, colTok=colTok)
        try:
            fwd = twos.forward(capi.MB_ROLLING) if loglike else None
            if counts:
                _, s, _ = twos.counts(acc._flat)
                acc.loglike += s
            vit = twos.viterbi(paths=False)[0] if viterbi else None
            if posteriors:
                pa, pb, _ = twos.row_posteriors()
                post = [(np.array(pa[twos.inOff[k]:twos.inOff[k + 1]]), np.array(pb[k * len(B):(k + 1) * len(B)])) for k in range(len(As))]
        finally:
            twos.close(); dm.close()

    def floats(v):
        return None if v is None else [float(x) for x in v]
    scores = {"loglike": floats(fwd), "viterbi": floats(vit)}
    if posteriors:
        scores["posteriors"] = post
    return scores, (acc.paramCounts(machine, params) if counts else None)


def sampleTwoProfiles(machine: Machine, inProfiles, outProfile, nSamples: int, seed: int = 0, backend: str = "device", params=None,
                      band: Optional[int] = None):
    """``nSamples`` alignments of every input profile with ``outProfile`` drawn from the posterior (docs/profile_tapes.md,
    "Posterior path samples of pairs of profiles"), the pairs of scoreTwoProfiles in one batch.  Returns (paths, logq, loglike):
    paths[k][j] is sample j of input profile k as a MachinePath (dp.edgesToPath), logq[k][j] its log posterior probability -- the
    path's own log weight with the blanks of both tapes, minus loglike[k] -- and loglike[k] the Forward log-likelihood.  A pair that
    scores -inf gets empty paths and logq = -inf.  A sample depends on (seed, k, j) alone.  ``backend``: "device"
    (capi.DeviceProfileTwos.sample_paths) or "numpy" (profile.TwoProfileDP.samplePaths).  ``band``: as scoreTwoProfiles."""
    import numpy as np
    from . import dp
    from .profile import TwoProfileDP
    from .seqpair import Envelope
    if backend not in ("device", "numpy"):
        raise MachineError('backend is "device" or "numpy"')
    nSamples = int(nSamples)
    if nSamples < 1:
        raise MachineError("nSamples must be at least 1")
    ev = EvaluatedMachine.fromMachine(machine, params)
    if not ev.nInTok:
        raise MachineError("two-profile sweeps need a machine with an input alphabet")
    As = [a.logRowsIn(ev) for a in inProfiles]
    B = outProfile.logRows(ev)
    envs = None if band is None else [Envelope.band(len(A), len(B), int(band)) for A in As]
    if backend == "numpy":
        tdp = TwoProfileDP(ev)
        ll, got = [], []
        for k, A in enumerate(As):
            l, samples = tdp.samplePaths(A, B, nSamples, seed=seed, pair=k, env=None if envs is None else envs[k])
            ll.append(l); got.append([(s[0], s[3]) for s in samples])
    else:
        from . import capi
        dm = capi.DeviceMachine(ev)
        twos = capi.DeviceProfileTwos(dm, As, [B] * len(As), envs=envs)
        try:
            ll, off, edges, _rows, _ins, lq = twos.sample_paths(nSamples, seed=seed)
        finally:
            twos.close(); dm.close()
        got = [[(edges[off[k * nSamples + j]:off[k * nSamples + j + 1]], lq[k * nSamples + j]) for j in range(nSamples)] for k in range(len(As))]
    paths = [[dp.edgesToPath(ev, machine, e) for e, _q in samples] for samples in got]
    return paths, [[float(q) for _e, q in samples] for samples in got], [float(l) for l in ll]


def scoreMergedTwos(machine: Machine, inProfiles, outProfile, backend: str = "device", params=None, loglike: bool = True,
                    viterbi: bool = False, counts: bool = False, posteriors: bool = False, band: Optional[int] = None):
    """scoreTwoProfiles(merge=True) with everything the merged two-profile pairs have: every input profile (a profile.Profile read
    against the machine's input alphabet, or its [K, nInTok + 1] log rows) as one pair with ``outProfile`` read CTC-merged (a
    profile.Profile, or a pair (logB[L, nCols + 1], colTok) as Profile.mergeRows returns); the same return shape, (scores,
    paramCounts).  ``band``: every pair is swept under seqpair.Envelope.band(K, L, band), K the rows of its input profile, on both
    backends (docs/profile_tapes.md, "Pairs of profiles against a merged profile under an envelope"); a width that cannot bridge
    the slope raises MachineError("Envelope is not connected").  ``posteriors``: scores["posteriors"] holds one
    (postA[K, nInTok + 1], postB[L, nCols + 1]) per input profile, as mergedTwoPosteriors returns them -- zeros for a pair that
    scores -inf; the key is absent when not asked for.  ``backend``: "device" (capi.DeviceProfileTwos with colTok) or "numpy"
    (profile.TwoMergedProfileDP)."""
    import numpy as np
    from . import dp
    from .profile import TwoMergedProfileDP
    from .seqpair import Envelope
    if backend not in ("device", "numpy"):
        raise MachineError('backend is "device" or "numpy"')
    ev = EvaluatedMachine.fromMachine(machine, params)
    if not ev.nInTok:
        raise MachineError("two-profile sweeps need a machine with an input alphabet")
    if not ev.nOutTok:
        raise MachineError("--recognize-merge-csv needs a machine with an output alphabet")
    As = [a.logRowsIn(ev) if hasattr(a, "logRowsIn") else np.asarray(a, np.float64).reshape(-1, ev.nInTok + 1) for a in inProfiles]
    B, colTok = _mergedRows(outProfile, ev) if hasattr(outProfile, "mergeRows") else outProfile
    B = np.asarray(B, np.float64).reshape(-1, len(colTok) + 1)
    envs = [None] * len(As) if band is None else [Envelope.band(len(A), len(B), int(band)) for A in As]
    acc = dp.MachineCounts(ev)
    fwd = vit = post = None
    if backend == "numpy":
        tdp = TwoMergedProfileDP(ev, colTok)
        fwd = [tdp.forward(A, B, env=e)[0] for A, e in zip(As, envs)] if loglike else None
        if counts:
            for A, e in zip(As, envs):
                c, ll = tdp.counts(A, B, env=e)
                acc._flat += c
                acc.loglike += ll
        vit = [tdp.forward(A, B, "max", env=e)[0] for A, e in zip(As, envs)] if viterbi else None
        post = [tdp.mergedRowPosteriors(A, B, env=e)[:2] for A, e in zip(As, envs)] if posteriors else None
    else:
        from . import capi
        dm = capi.DeviceMachine(ev)
        twos = None
        try:
            twos = capi.DeviceProfileTwos(dm, As, [B] * len(As), colTok=colTok, mergedEnvs=None if band is None else envs)
            fwd = twos.forward(capi.MB_ROLLING) if loglike else None
            if counts:
                _, s, _ = twos.counts(acc._flat)
                acc.loglike += s
            vit = twos.viterbi(paths=False)[0] if viterbi else None
            if posteriors:
                pa, pb, _ = twos.merged_row_posteriors()
                post = [(np.array(pa[twos.inOff[k]:twos.inOff[k + 1]]), np.array(pb[k * len(B):(k + 1) * len(B)])) for k in range(len(As))]
        finally:
            if twos is not None:
                twos.close()
            dm.close()

    def floats(v):
        return None if v is None else [float(x) for x in v]
    scores = {"loglike": floats(fwd), "viterbi": floats(vit)}
    if posteriors:
        scores["posteriors"] = post
    return scores, (acc.paramCounts(machine, params) if counts else None)


def mergedTwoPosteriors(machine: Machine, inProfiles, outProfile, backend: str = "device", params=None, band: Optional[int] = None):
    """Every input profile (a profile.Profile read against the machine's input alphabet, or its [K, nInTok + 1] log rows) as one
    pair with ``outProfile`` read CTC-merged, as --recognize-merge-csv reads it (a profile.Profile, or a pair
    (logB[L, nCols + 1], colTok) as Profile.mergeRows returns), all pairs in one batch: (posteriors, loglike), one
    (postA[K, nInTok + 1], postB[L, nCols + 1]) and one float per input profile -- the posterior probability that each input row was
    consumed as each input token and each output row as each column (column 0 of either: as its blank), the gradients of the pair's
    log-likelihood in the two profiles (docs/profile_tapes.md, "Row posteriors of pairs of profiles against a merged profile").  A
    pair that scores -inf gets zeros.  ``backend``: "device" (capi.DeviceProfileTwos.merged_row_posteriors) or "numpy"
    (profile.TwoMergedProfileDP.mergedRowPosteriors).  ``band``: every pair is swept under seqpair.Envelope.band(K, L, band)
    (docs/profile_tapes.md, "Pairs of profiles against a merged profile under an envelope")."""
    import numpy as np
    from .profile import TwoMergedProfileDP
    from .seqpair import Envelope
    if backend not in ("device", "numpy"):
        raise MachineError('backend is "device" or "numpy"')
    ev = EvaluatedMachine.fromMachine(machine, params)
    if not ev.nInTok:
        raise MachineError("two-profile sweeps need a machine with an input alphabet")
    if not ev.nOutTok:
        raise MachineError("--recognize-merge-csv needs a machine with an output alphabet")
    As = [a.logRowsIn(ev) if hasattr(a, "logRowsIn") else np.asarray(a, np.float64).reshape(-1, ev.nInTok + 1) for a in inProfiles]
    B, colTok = _mergedRows(outProfile, ev) if hasattr(outProfile, "mergeRows") else outProfile
    B = np.asarray(B, np.float64).reshape(-1, len(colTok) + 1)
    envs = None if band is None else [Envelope.band(len(A), len(B), int(band)) for A in As]
    if backend == "numpy":
        tdp = TwoMergedProfileDP(ev, colTok)
        res = [tdp.mergedRowPosteriors(A, B) for A in As] if envs is None else [tdp.mergedRowPosteriors(A, B, env=e) for A, e in zip(As, envs)]
        return [(r[0], r[1]) for r in res], [float(r[2]) for r in res]
    from . import capi
    dm = capi.DeviceMachine(ev)
    twos = None
    try:
        twos = capi.DeviceProfileTwos(dm, As, [B] * len(As), colTok=colTok, mergedEnvs=envs)
        pa, pb, ll = twos.merged_row_posteriors()
        post = [(np.array(pa[twos.inOff[k]:twos.inOff[k + 1]]), np.array(pb[k * len(B):(k + 1) * len(B)])) for k in range(len(As))]
    finally:
        if twos is not None:
            twos.close()
        dm.close()
    return post, [float(x) for x in ll]


def _runTwoProfiles(args, out, machine: Machine) -> int:
    """--generate-csv beside --recognize-csv on a machine with an input alphabet: one pair of profiles (docs/profile_tapes.md,
    "Pairs of profiles").  -L and -V print [the --generate-csv argument, "", score], -C the counts, --profile-posteriors after them
    [the --generate-csv argument, "", {"input": the K rows of postA, "output": the L rows of postB}].  --decode-backend numpy:
    profile.TwoProfileDP."""
    from .profile import Profile
    if not machine.inputAlphabet():
        raise MachineError("two-profile sweeps need a machine with an input alphabet")
    if not os.path.exists(args.generate_csv) or not os.path.exists(args.recognize_csv):
        raise MachineError("CSV file not found")
    sc, pc = scoreTwoProfiles(machine, [Profile.fromCsv(args.generate_csv)], Profile.fromCsv(args.recognize_csv),
                              backend="numpy" if args.decode_backend == "numpy" else "device", params=_profileParams(args, machine),
                              loglike=bool(args.loglike), viterbi=bool(args.viterbi), counts=bool(args.counts),
                              posteriors=bool(args.profile_posteriors))
    if args.loglike:
        out.write('[["%s","",%s]]\n' % (escaped(args.generate_csv), fmt(sc["loglike"][0])))
    if args.counts:
        out.write("{" + ",".join('"%s":%s' % (escaped(k), "%g" % pc[k]) for k in sorted(pc)) + "}\n")
    if args.viterbi:
        out.write('[["%s","",%s]]\n' % (escaped(args.generate_csv), fmt(sc["viterbi"][0])))
    if args.profile_posteriors:
        rows = lambda a: "[" + ",".join("[" + ",".join(fmt(float(v)) for v in row) + "]" for row in a) + "]"
        pa, pb = sc["posteriors"][0]
        out.write('[["%s","",{"input":%s,"output":%s}]]\n' % (escaped(args.generate_csv), rows(pa), rows(pb)))
    return 0


def _runMergedNumpy(args, out, machine: Machine, params, ev, profile) -> int:
    """-L / -C / -V of a merged profile through the numpy restatement, printed as runProfile prints the device's."""
    from . import dp
    from .profile import MergedProfileDP
    P, colTok = profile.mergeRows(ev)
    mdp = MergedProfileDP(ev, colTok)
    if args.loglike:
        out.write('[["","",%s]]\n' % fmt(mdp.forward(P)[0]))
    if args.counts:
        counts = dp.MachineCounts(ev)
        c, ll = mdp.counts(P)
        counts._flat += c
        counts.loglike += ll
        pc = counts.paramCounts(machine, params)
        out.write("{" + ",".join('"%s":%s' % (escaped(k), "%g" % pc[k]) for k in sorted(pc)) + "}\n")
    if args.viterbi:
        out.write('[["","",%s]]\n' % fmt(mdp.forward(P, "max")[0]))
    if args.profile_posteriors:
        _writeProfilePosteriors(out, profilePosteriors(machine, profile, "numpy", params, merge=True)[0])
    return 0


def _viterbiInputs(backend: str, silent: Machine, decodeTrans: Machine, params, outputs: List[List[str]]) -> List[List[str]]:
    """--viterbi-decode / --viterbi-encode (target/boss.cpp:869-873, 904-907): the Viterbi path of the input-silenced machine for
    each output, then the input symbols of the heaviest matching transitions of the machine itself (algebra.decodePath).  The
    device backend is the existing Viterbi-with-paths entry point; the numpy one scores the silenced machine, a generator,
    against the output as a one-hot profile (profile.ProfileDP), which takes the same first maximum."""
    from . import dp
    from .algebra import decodePath
    ev = EvaluatedMachine.fromMachine(silent, params)
    if not all(ev.outputTokenizer.canTokenize(o) for o in outputs):
        raise MachineError("Can't do traceback: no finite-weight paths")
    if backend == "numpy":
        import numpy as np
        from .profile import ProfileDP
        pdp = ProfileDP(ev)
        paths = []
        for o in outputs:
            P = np.full((len(o), ev.nOutTok + 1), -math.inf)
            P[np.arange(len(o)), ev.outputTokenizer.tokenize(o)] = 0.0
            v, edges, _ = pdp.viterbi(P)
            paths.append(dp.edgesToPath(ev, silent, edges) if v > -math.inf else None)
    else:
        paths = [p for _, p in dp.viterbiBatch(ev, silent, [SeqPair([], o, "", "") for o in outputs])]
    if any(p is None for p in paths):
        raise MachineError("Can't do traceback: no finite-weight paths")
    return [decodePath(p, decodeTrans, params) for p in paths]


def encodingMachine(machine: Machine, viterbi: bool = False) -> Machine:
    """The machine whose DECODING is the encoding of ``machine`` (target/boss.cpp:854-855)."""
    from . import algebra
    trans = algebra.advancingMachine(algebra.advanceSort(algebra.transpose(machine)))
    return algebra.decodeSort(trans) if viterbi else trans


def viterbiEncode(machine: Machine, inputs: List[List[str]], backend: str = "device", params=None) -> List[List[str]]:
    """--viterbi-encode as a function: the output of the Viterbi path for each input symbol sequence."""
    from . import algebra
    trans = encodingMachine(machine, True)
    return _viterbiInputs(backend, algebra.silenceInput(trans), trans, machine.getParamDefs(True) if params is None else params, inputs)


def _canonical(mt) -> float:
    """uniform_real_distribution<double>(0, 1) over a 32-bit generator: two draws, low word first."""
    lo = mt(); hi = mt()
    return min((lo + hi * 4294967296.0) / 18446744073709551616.0, 1.0 - 2.0 ** -53)


def runCoding(args, machine: Machine, params, data: List[SeqPair], emit) -> None:
    """The encode and decode sections of target/boss.cpp:850-921."""
    from . import algebra, prefixtree
    from .dp import Mt19937
    maxBacktrack = args.prefix_backtrack if args.prefix_backtrack is not None else prefixtree.NO_BACKTRACK_LIMIT
    encoding = args.prefix_encode or args.viterbi_encode or args.random_encode
    decoding = args.prefix_decode or args.viterbi_decode

    def impute(trans: Machine, viterbi: bool, sample: bool, outputs: List[List[str]]) -> List[List[str]]:
        if viterbi:
            return _viterbiInputs(args.decode_backend, algebra.silenceInput(trans), trans, params, outputs)
        ev = EvaluatedMachine.fromMachine(trans, params)
        if not sample:
            return prefixtree.decodeBatch(ev, outputs, maxBacktrack, args.decode_backend, args.decode_nodes)[0]
        import time
        seed = args.seed if args.seed is not None else int(time.time())
        res = []
        for o in outputs:
            mt = Mt19937(seed)                     # makeRnd() per sequence pair (target/boss.cpp:877): every pair starts from the seed
            tree = prefixtree.PrefixTree.forOutput(ev, o, maxBacktrack, args.decode_backend, args.decode_nodes)
            try:
                res.append(tree.sampleSeq(lambda: _canonical(mt)))
            finally:
                tree.close()
        return res

    if encoding:
        if not data:
            raise MachineError("To encode an output sequence, please specify an input sequence file")
        for sp in data:
            if sp.output:
                raise MachineError("You cannot specify output sequences when encoding; the goal of encoding is to generate %s output for a given input"
                                   % ("random" if args.random_encode else "the most likely"))
        trans = encodingMachine(machine, args.viterbi_encode)      # encoding is decoding of the transpose
        enc = impute(trans, args.viterbi_encode, args.random_encode, [sp.input for sp in data])
        emit("[" + ",\n ".join(seqPairJson(SeqPair(sp.input, e, sp.inputName, "output")) for sp, e in zip(data, enc)) + "]\n")
    if decoding:
        if not data:
            raise MachineError("To decode an input sequence, please specify an output sequence file")
        for sp in data:
            if sp.input:
                raise MachineError("You cannot specify input sequences when decoding; the goal of decoding is to impute the most likely input for a given output")
        dec = impute(machine, args.viterbi_decode, False, [sp.output for sp in data])
        emit("[" + ",\n ".join(seqPairJson(SeqPair(d, sp.output, "input", sp.outputName)) for sp, d in zip(data, dec)) + "]\n")


_GENERATE_ONLY = ("--generate-csv goes with --recognize-csv and -L, -V or -C on a machine with an input alphabet, nowhere else: not with "
                  "--recognize-merge-csv, an input sequence, the decode options or --profile-band; --profile-posteriors may stand beside or instead of -L, -V and -C")
_POSTERIORS_ONLY = ("--profile-posteriors goes with --recognize-csv beside an input sequence (--input-chars, --input-fasta, --input-json) or beside --generate-csv, "
                    "or with --recognize-csv / --recognize-merge-csv alone on a machine with an empty input alphabet, nowhere else")
_BAND_ONLY = "--profile-band goes with --recognize-csv beside an input sequence (--input-chars, --input-fasta, --input-json) and -L, -V or -C, nowhere else"


def run(argv: Optional[List[str]] = None, out=None) -> int:
    out = out or sys.stdout
    args = buildParser().parse_args(argv)
    if args.generate_csv is not None:
        decode = args.prefix_decode or args.viterbi_decode or args.prefix_encode or args.viterbi_encode or args.random_encode
        hasInput = args.input_chars is not None or bool(args.input_fasta) or bool(args.input_json)
        if args.recognize_csv is None or args.recognize_merge_csv is not None or hasInput or decode or args.profile_band is not None:
            raise MachineError(_GENERATE_ONLY)
    if args.profile_band is not None:
        decode = args.prefix_decode or args.viterbi_decode or args.prefix_encode or args.viterbi_encode or args.random_encode
        if args.recognize_csv is None or args.recognize_merge_csv is not None or decode:
            raise MachineError(_BAND_ONLY)
        if args.profile_band < 0:
            raise MachineError("--profile-band takes a half-width of 0 or more")
    if args.profile_posteriors:
        decode = args.prefix_decode or args.viterbi_decode or args.prefix_encode or args.viterbi_encode or args.random_encode
        if (args.recognize_csv is None and args.recognize_merge_csv is None) or decode:
            raise MachineError(_POSTERIORS_ONLY)
    if args.recognize_csv is not None or args.recognize_merge_csv is not None:
        return runProfile(args, out)
    machine = loadMachine(args)
    encoding = args.prefix_encode or args.viterbi_encode or args.random_encode
    decoding = args.prefix_decode or args.viterbi_decode
    inference = args.loglike or args.viterbi or args.align or args.counts or args.train or encoding or decoding
    data = collectData(args, machine, inference, encoding, decoding)
    gotData = bool(data)
    noIO = not machine.inputAlphabet() and not machine.outputAlphabet()
    if gotData and not inference:
        raise MachineError("No point in specifying input/output data without --train, --loglike, --counts, --align")
    funcs: Dict[str, Any] = {}
    for f in args.functions:
        funcs.update(json.load(open(f)))
    seed: Dict[str, Any] = {}
    for f in args.params:
        seed.update(json.load(open(f)))
    constraints = Constraints()
    for f in args.constraints:
        c = Constraints.fromJson(json.load(open(f)))
        constraints = Constraints(constraints.prob + c.prob, constraints.norm + c.norm, constraints.rate + c.rate)

    dist = _dist()
    rank = dist.get_rank() if dist else 0
    world = dist.get_world_size() if dist else 1
    owned = _shard(data, machine, world) if world > 1 else [list(range(len(data)))]
    mine = [data[k] for k in owned[rank]]
    emit = (lambda s: out.write(s)) if rank == 0 else (lambda s: None)

    from . import dp
    if args.train:
        from .fitter import MachineFitter, combineConstraints
        if not ((args.constraints or not machine.cons.empty()) and (gotData or noIO)):
            raise MachineError("To fit parameters, please specify a constraints file and (for machines with input/output) a data file")
        fitter = MachineFitter(machine, constraints, funcs)
        sd = combineConstraints(machine.cons, constraints).defaultParams(); sd.update(seed)
        fitter.seed = sd
        reduce = _reduce_counts if world > 1 else None
        params = fitter.fit(mine, args.wiggle_room, reduce)
        emit("{" + ",".join('"%s":%s' % (escaped(k), fmtParam(params[k])) for k in sorted(params)) + "}\n")
    else:
        params = dict(funcs); params.update(seed)
        for k, v in machine.getParamDefs(args.use_defaults).items():
            params.setdefault(k, v)

    if args.loglike:
        ev = EvaluatedMachine.fromMachine(machine, params)
        ll = _gather_in_order(dp.forwardLogLikeBatch(ev, mine, rolling=True), len(data), rank, world, owned)
        emit("[" + ",\n ".join('["%s","%s",%s]' % (escaped(sp.inputName), escaped(sp.outputName), fmt(x))
                                for sp, x in zip(data, ll)) + "]\n")

    if args.counts:
        ev = EvaluatedMachine.fromMachine(machine, params)
        counts = dp.MachineCounts(ev, mine)
        if world > 1:
            _, counts.loglike = _reduce_counts(counts._flat, counts.loglike)
        pc = counts.paramCounts(machine, params)
        emit("{" + ",".join('"%s":%s' % (escaped(k), "%g" % pc[k]) for k in sorted(pc)) + "}\n")

    if args.align or args.viterbi:
        if not gotData:
            raise MachineError("To align sequences, please specify a data file")
        ev = EvaluatedMachine.fromMachine(machine, params)
        res = dp.viterbiBatch(ev, machine, mine)
        res = _gather_in_order(res, len(data), rank, world, owned)
        if args.viterbi:
            emit("[" + ",\n ".join('["%s","%s",%s]' % (escaped(sp.inputName), escaped(sp.outputName), fmt(v))
                                    for sp, (v, _) in zip(data, res)) + "]\n")
        if args.align:
            aligned = [seqPairFromPath(machine, p, sp.inputName, sp.outputName) for sp, (v, p) in zip(data, res) if p is not None]
            emit("[" + ",\n ".join(seqPairJson(sp) for sp in aligned) + "]\n")

    if encoding or decoding:
        if world > 1:
            raise MachineError("encoding and decoding run on one rank")
        runCoding(args, machine, params, data, emit)
    return 0


def _init_ranks():
    """Launched under torchrun (WORLD_SIZE > 1): bind this rank to its GPU and open the ranks BEFORE the first GPU call, so that
    run() shards the pair list and reduces the counts (shard.RankGroup: rendezvous over gloo, the count reduction over RCCL
    through the C-ABI; MB_DIST_BACKEND = gloo puts several ranks on ONE GPU for the tests).  Returns the group if this call
    opened it (the caller closes it), else None."""
    global _GROUP
    import os
    if int(os.environ.get("WORLD_SIZE", "1")) <= 1 or _dist() is not None:
        return None
    from .shard import RankGroup
    _GROUP = RankGroup.from_env()
    return _GROUP


def main(argv: Optional[List[str]] = None) -> int:
    opened = None
    try:
        opened = _init_ranks()
        return run(argv)
    except (MachineError, OSError, KeyError, ValueError) as e:   # main() of the reference prints what() and fails (boss.cpp:923-926)
        sys.stderr.write(str(e) + "\n")
        return 1
    finally:
        if opened is not None:
            global _GROUP
            opened.close(); _GROUP = None


if __name__ == "__main__":
    sys.exit(main())
