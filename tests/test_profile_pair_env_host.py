"""CPU tests of the two-tape profile sweeps under an envelope (docs/profile_tapes.md, "Pairs under an envelope"): the envelope
builders, the masked restatement profile.PairProfileDP(env=...) against a brute-force sum over paths, its identities, the liveness
of the inputs of test_profile_pair_env_gpu.py, and the command line."""
import io
import math
import os

import numpy as np
import pytest

import pairenvhelpers as eh
import pairprofilehelpers as ph
from machineboss_amd import boss
from machineboss_amd.machine import MachineError
from machineboss_amd.profile import PairProfileDP, Profile
from machineboss_amd.seqpair import Envelope

HERE = os.path.dirname(os.path.abspath(__file__))


# ---- envelope builders ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("I,L,w", [(0, 0, 0), (0, 7, 0), (7, 0, 0), (9, 9, 0), (9, 9, 2), (30, 11, 3), (11, 30, 1)])
def test_band_is_connected_and_monotone(I, L, w):
    e = Envelope.band(I, L, w)
    assert (e.inLen, e.outLen, len(e.inStart), len(e.inEnd)) == (I, L, L + 1, L + 1)
    assert e.connected() and e.monotone()
    assert e.contains(0, 0) and e.contains(I, L)
    for r in range(L + 1):
        if L:
            c = int(math.floor(r * I / L + 0.5))
            assert e.inStart[r] == max(0, c - w) and e.inEnd[r] == min(I, c + w) + 1


def test_band_too_narrow_for_the_slope():
    with pytest.raises(MachineError, match="not connected"):
        Envelope.band(60, 5, 1)


def test_reference_envelopes_are_monotone():
    rng = np.random.RandomState(1)
    for I, L in ((0, 0), (5, 0), (0, 5), (9, 4), (4, 9), (20, 20)):
        cols = eh.random_alignment(rng, I, L)
        for e in (eh.full(I, L), Envelope.pathEnvelope(cols), Envelope.pathAreaEnvelope(cols, 2), eh.staircase(I, L)):
            assert e.connected() and e.monotone() and (e.inLen, e.outLen) == (I, L)
    assert not eh.envelope([0, 2, 1], [3, 4, 4], 3).monotone() and not eh.envelope([0, 0, 0], [3, 2, 4], 3).monotone()


def test_restatement_rejects_what_the_device_rejects():
    em = ph.pair_machine(2, 1, False, 1, 1)
    dp = PairProfileDP(em)
    x, P = np.ones(3, np.int32), np.zeros((2, 2))
    for st, en, msg in (([0, 0], [4, 4], "mismatch"), ([0, 0, 0], [4, 4, 5], "mismatch"), ([-1, 0, 0], [4, 4, 4], "mismatch"),
                        ([0, 2, 3], [1, 3, 4], "not connected"), ([1, 1, 1], [4, 4, 4], "not connected"), ([0, 0, 0], [4, 4, 3], "not connected"),
                        ([0, 1, 0], [4, 4, 4], "not monotone"), ([0, 0, 0], [4, 3, 4], "not monotone")):
        with pytest.raises(MachineError, match=msg):
            dp.forward(x, P, env=(st, en))


# ---- the masked restatement against brute force ------------------------------------------------------------------------------------------
class _TooMany(Exception):
    pass


def _brute_forward(dp, x, P, inside, budget=300000):
    """The sum over all paths from N(0, 0, 0) to W(I, L, S-1) of the UNMASKED recurrence that stay inside the envelope, enumerated
    one by one: the second of the two routes (the other being the composite machine under a transformed envelope).  A path moves
    between N and W nodes by the terms of the recurrence; nothing is shared between paths.  Raises _TooMany past `budget` nodes."""
    I, L, S = len(x), len(P), dp.S
    P = [[float(v) for v in row] for row in P]

    def by_source(tab):
        out = [[] for _ in range(S)]
        _, s, d, w, o = tab
        for k in range(len(s)):
            out[int(s[k])].append((int(d[k]), float(w[k]), int(o[k])))
        return out
    ins = [by_source(t) for t in dp.ins]; match = [by_source(t) for t in dp.match]
    emit = by_source((None, dp.eS, dp.eD, dp.eW, dp.eO)); sil = by_source((None, dp.sS, dp.sD, dp.sW, np.zeros(len(dp.sS), np.int64)))
    inside = inside.tolist()
    total = []
    seen = [0]

    def at_n(i, r, q, w):
        if not inside[i][r] or w == -math.inf:
            return
        at_w(i, r, q, w)                                   # no move
        if r < L:
            at_n(i, r + 1, q, w + P[r][0])                 # the blank reads N

    def at_w(i, r, q, w):
        if not inside[i][r] or w == -math.inf:
            return
        seen[0] += 1
        if seen[0] > budget:
            raise _TooMany()
        if i == I and r == L and q == S - 1:
            total.append(w)
        if i < I:
            for d, ww, _o in ins[x[i]][q]:
                at_w(i + 1, r, d, w + ww)
        for d, ww, _o in sil[q]:
            at_w(i, r, d, w + ww)
        if r < L:
            if i < I:
                for d, ww, o in match[x[i]][q]:
                    at_n(i + 1, r + 1, d, (w + ww) + P[r][o])
            for d, ww, o in emit[q]:
                at_n(i, r + 1, d, (w + ww) + P[r][o])

    at_n(0, 0, 0, 0.0)
    return float(np.logaddexp.reduce(total)) if total else -math.inf


@pytest.mark.parametrize("levels", (True, False))
@pytest.mark.parametrize("S", (5, 8))
def test_masked_forward_is_the_sum_over_paths_inside(S, levels):
    """Lattices up to (5, 4), three seeds, every envelope kind.  An envelope with more paths than the enumeration's budget is left
    out (the whole rectangle beyond (2, 2) runs into the millions); the narrow ones reach (5, 4)."""
    worst, finite, largest, kinds = 0.0, 0, 0, set()
    for seed in range(3):
        em = ph.pair_machine(S, 10 * S + seed, levels, 2, 2)
        dp = PairProfileDP(em)
        for I, L in ((2, 2), (3, 3), (4, 3), (5, 4)):
            rng = np.random.RandomState(100 * seed + 10 * I + L)
            x, P = ph.pair_input(rng, em, I, L, pZero=0.4)
            for kind, env in eh.envelopes(rng, I, L):
                if kind == "full" and I + L > 4:
                    continue
                try:
                    want = _brute_forward(dp, x, P, eh.mask(env, I))
                except _TooMany:
                    continue
                got = dp.forward(x, P, env=env)[0]
                assert ph.logs_close([got], [want]), (S, levels, seed, I, L, kind, got, want)
                if want > -math.inf:
                    finite += 1; kinds.add(kind); largest = max(largest, I + L)
                worst = max(worst, ph.log_dev([got], [want]))
    assert finite >= 12 and kinds == set(eh.ENV_KINDS) and largest == 9, (finite, kinds, largest)      # 12: one per seed and shape
    print("masked Forward against the path sum, worst deviation: %.3g over %d finite cases" % (worst, finite))


# ---- identities -----------------------------------------------------------------------------------------------------------------------
def test_full_envelope_is_no_envelope_bit_for_bit():
    em = ph.pair_machine(8, 5, True, 2, 3)
    dp = PairProfileDP(em)
    for I, L in ((0, 0), (3, 5), (6, 2)):
        x, P = ph.pair_input(np.random.RandomState(I), em, I, L)
        e = eh.full(I, L)
        for a, b in ((dp.forward(x, P), dp.forward(x, P, env=e)), (dp.forward(x, P, "max"), dp.forward(x, P, "max", env=e)),
                     (dp.backward(x, P), dp.backward(x, P, env=(e.inStart, e.inEnd)))):
            assert a[0] == b[0] and np.array_equal(a[1], b[1]) and np.array_equal(a[2], b[2])
        assert np.array_equal(dp.counts(x, P)[0], dp.counts(x, P, env=e)[0])
        va, vb = dp.viterbi(x, P), dp.viterbi(x, P, env=e)
        assert va[0] == vb[0] and np.array_equal(va[1], vb[1]) and np.array_equal(va[2], vb[2])


def test_backward_meets_forward_and_counts_sum_to_the_input_length():
    finite = 0
    for S, levels in ((5, True), (8, False), (8, True)):
        em = ph.pair_machine(S, 30 + S, levels, 2, 3)
        dp = PairProfileDP(em)
        reads = np.nonzero(em.inTok > 0)[0]
        for I, L in ((3, 3), (9, 4), (4, 9), (12, 12)):
            rng = np.random.RandomState(10 * I + L)
            x, P = ph.pair_input(rng, em, I, L)
            for kind, env in eh.envelopes(rng, I, L):
                ll, N, W = dp.forward(x, P, env=env)
                bl, NB, WB = dp.backward(x, P, env=env)
                assert ph.logs_close([bl], [ll]), (kind, bl, ll)
                out = ~eh.mask(env, I)
                assert np.all(N[out] == -math.inf) and np.all(W[out] == -math.inf) and np.all(NB[out] == -math.inf) and np.all(WB[out] == -math.inf)
                c = dp.counts(x, P, env=env)[0]
                if ll > -math.inf:
                    finite += 1
                    assert abs(c[reads].sum() - I) <= 1e-9 * max(1, I), (kind, c[reads].sum(), I)
                else:
                    assert not c.any()
    assert finite >= 30


# ---- the inputs of the GPU suite are live ------------------------------------------------------------------------------------------------
def _live(lls):
    return np.mean(np.asarray(lls) > -math.inf)


def test_env_suite_inputs_are_live():
    """With the seeds of pairenvhelpers, nine in ten banded likelihoods of each GPU case are finite, by the restatement alone (the
    (0, 0) lattice of a machine without levels cannot reach its end state, as in the unbanded suites: it is the tenth)."""
    for S in eh.CELL_STATES:
        lls = [PairProfileDP(em).forward(x, P, env=env)[0] for em, x, P, kind, env in eh.cell_case(S)]
        kinds = {kind for *_, kind, _e in eh.cell_case(S)}
        assert kinds == set(eh.ENV_KINDS)
        assert _live(lls) >= 0.9, (S, _live(lls))
    dp = PairProfileDP(eh.slope_machine())
    for I, L, w in eh.SLOPE_CASES:
        x, P, env = eh.slope_case(I, L, w)
        assert dp.forward(x, P, env=env)[0] > -math.inf and eh.diag_max(env) < min(I, L) + 1
    x, P, env = eh.area_case()
    assert dp.forward(x, P, env=env)[0] > -math.inf and not env.isFull()
    for M in eh.MARK_M:
        assert eh.diag_max(eh.mark_case(M)[2]) == M


def test_tie_batch_shows_every_tie_with_a_loser_outside():
    """tie_machine on tie_pairs under band(w = 1): every kind of tie shows at least once, and at least once each a blank and an
    input-only candidate -- the two whose source cell a band cuts off; a match comes along the band -- loses because its source
    cell lies outside the envelope."""
    dp = PairProfileDP(ph.tie_machine())
    census = {}
    pairs = eh.tie_env_pairs()
    assert len(pairs) >= 10
    for x, P, env in pairs:
        v, edges, rows = dp.viterbi(x, P, census=census, env=env)
        assert v > -math.inf
    ties = {k for k in census if k[0] != "outside"}
    for want in eh.TIE_KINDS:
        assert any(set(want) <= set(k) for k in ties), (want, census)
    for kind in ("blank", "ins"):
        assert census.get(("outside", kind), 0) >= 1, census


# ---- the inputs of test_profile_pair_mixed_gpu.py: one call over plain and enveloped pairs ----------------------------------------------
def _envs(triples):
    return [t[2] for t in triples]


@pytest.mark.parametrize("S", eh.MIXED_STATES)
def test_mixed_batch_composition_and_liveness(S):
    """mixed_case: an enveloped pair first and a plain one last; bands of width 0, 1 and 2, a path-area envelope, a staircase whose
    rows are single cells and full envelopes; (0, 0), no rows, no input and a dead pair of each kind; shapes up to (20, 14).  All
    but the two dead pairs have a finite likelihood and, where I + L > 0, a path."""
    em, triples = eh.mixed_case(S)
    spec = eh.MIXED_SPEC
    envs = _envs(triples)
    assert len(triples) == len(spec) >= 12 and em.nStates == S and eh.silent_levels(em) >= 1
    assert envs[0] is not None and envs[-1] is None
    sl = eh.slots(envs)
    assert sorted(sl) == list(range(len(sl))) and sl[0] == sum(e is None for e in envs) and sl[-1] == sl[0] - 1
    kinds = "".join("E" if e is not None else "P" for e in envs)
    assert "PP" in kinds and "EE" in kinds and "PEP" in kinds and "EPE" in kinds      # (the two kinds alternate irregularly)
    assert {s[2] for s in spec} == {None, "band0", "band1", "band2", "area", "stairs", "full"}
    for (x, P, env), (I, L, kind, dead) in zip(triples, spec):
        assert (len(x), len(P)) == (I, L) and (env is None) == (kind is None)
        if env is not None:
            assert env.connected() and env.monotone() and len(env.inStart) == L + 1
    stairs = triples[[s[2] for s in spec].index("stairs")][2]
    assert all(b - a == 1 for a, b in zip(stairs.inStart, stairs.inEnd))
    area = [t[2] for t, s in zip(triples, spec) if s[2] == "area"][0]
    assert not area.isFull() and eh.n_cells(area) > 20 + 14 + 1
    for kind in (False, True):      # plain, enveloped
        mine = [(s[0], s[1]) for s in spec if (s[2] is not None) == kind and not s[3]]
        assert (0, 0) in mine and any(I > 0 and L == 0 for I, L in mine) and any(I == 0 and L > 0 for I, L in mine)
        assert sum(1 for s in spec if (s[2] is not None) == kind and s[3]) == 1
    assert max(s[0] for s in spec) == 20 and max(s[1] for s in spec) == 14
    dp = PairProfileDP(em)
    lls = np.array([dp.forward(x, P, env=env)[0] for x, P, env in triples])
    assert _live(lls) >= 0.85, _live(lls)
    assert [k for k, v in enumerate(lls) if v == -math.inf] == list(eh.MIXED_DEAD)
    for k, (x, P, env) in enumerate(triples):
        v, edges, rows = dp.viterbi(x, P, env=env)
        assert (len(edges) > 0) == (k not in eh.MIXED_DEAD) or len(x) + len(P) == 0, k
    for name, state in eh.mixed_states(triples):
        assert state is None or len(state) == len(triples)
    swapped = dict(eh.mixed_states(triples))["swapped"]
    assert all((a is None) != (b is None) for a, b in zip(envs, swapped))


@pytest.mark.parametrize("S", eh.MIXED_STATES)
def test_mixed_batch_chunks_hold_every_kind_of_chunk(S):
    """Under 1.8 x the largest pair's bytes each of the four materialised calls cuts the batch into the same five chunks, by the
    restated chunk rule over the restated bytes: a mixed chunk whose first pair is enveloped, a plain one, an enveloped one, a
    mixed one whose first pair is plain, and a mixed one again."""
    em, triples = eh.mixed_case(S)
    envs = _envs(triples)
    assert eh.MIXED_BUDGET_FACTOR >= 1.2
    for call in eh.CALLS[:4]:
        b = eh.call_bytes(call, em, triples)
        assert all(v > 0 for v in b)
        chunks = eh.greedy_chunks(b, eh.mixed_budget(call, em, triples))
        assert chunks == eh.MIXED_CHUNKS and len(chunks) >= 4, (call, chunks)
        assert eh.chunk_kinds(chunks, envs) == eh.MIXED_CHUNK_KINDS and set(eh.MIXED_CHUNK_KINDS) == {"P", "E", "PE", "EP"}
        assert eh.chunk_launches(chunks, envs) == 8
        live = [k for k in range(len(triples)) if k not in eh.MIXED_DEAD]
        sub = [triples[k] for k in live]
        assert len(eh.greedy_chunks(eh.call_bytes(call, em, sub), eh.mixed_budget(call, em, sub))) >= 4
    assert eh.call_bytes("rolling", em, triples) == [0] * len(triples)      # every ring in LDS: the rolling sweeps do not chunk here


def test_rolling_chunks_of_the_scratch_rings():
    """roll_case: eight rings of 187 200 bytes, plain (48 x 13 x 300) and under band(12) (M = 13), past 160 KiB and so in scratch;
    four small pairs whose rings lie in LDS cost nothing and ride in the chunk they fall in.  A budget of 2.5 rings cuts the
    ring-bearing pairs into (E, P), (P, E), (E, E), (P, P); the last two chunks hold one kind only, small pairs included."""
    em, triples = eh.roll_case()
    envs = _envs(triples)
    b = eh.call_bytes("rolling", em, triples)
    assert em.nStates == 300 and [v for v in b if v] == [187200] * 8 and 187200 > eh.LDS_MAX
    assert [eh.diag_max(e) for e, c in zip(envs, eh.ROLL_ORDER) if c == "E"] == [13] * 4
    assert ["E" if e is not None else "P" for e in envs] == [c.upper() for c in eh.ROLL_ORDER]
    chunks = eh.greedy_chunks(b, eh.ROLL_BUDGET)
    assert chunks == [(0, 3), (3, 6), (6, 9), (9, 12)]
    rings = ["".join(c for c in eh.ROLL_ORDER[p0:p1] if c in "EP") for p0, p1 in chunks]
    assert tuple(rings) == eh.ROLL_CHUNKS
    assert eh.chunk_kinds(chunks, envs) == ["EP", "PE", "E", "P"] and eh.chunk_launches(chunks, envs) == 6
    dp = PairProfileDP(em)
    assert all(dp.forward(x, P, env=env)[0] > -math.inf for x, P, env in triples)


def test_seam_batch_puts_dead_pairs_at_the_block_seams_of_both_launches():
    """seam_case: 129 plain and 65 enveloped pairs interleaved; by slot within their launch the dead pairs are 63, 64 and 128 of the
    plain launch and 63 and 64 of the enveloped one; every other pair has a path."""
    em, triples = eh.seam_case()
    envs = _envs(triples)
    assert sum(e is None for e in envs) == eh.SEAM_PLAIN == 129 and sum(e is not None for e in envs) == eh.SEAM_ENV == 65
    assert max(max(len(x), len(P)) for x, P, _ in triples) <= 4
    sl = eh.slots(envs)
    dp = PairProfileDP(em)
    dead = sorted(sl[k] for k, (x, P, env) in enumerate(triples) if dp.forward(x, P, "max", env=env)[0] == -math.inf)
    assert dead == sorted(eh.SEAM_DEAD_PLAIN + tuple(129 + s for s in eh.SEAM_DEAD_ENV))
    assert len(eh.seam_prefix(triples, 64)) == 128 and len(eh.seam_prefix(triples, 65)) == 130
    for n in (64, 65):
        sub = [envs[k] for k in eh.seam_prefix(triples, n)]
        assert sum(e is None for e in sub) == sum(e is not None for e in sub) == n
    kinds = {kind for k, (x, P, env) in enumerate(triples) if env is not None
             for kind, e in eh.envelopes(np.random.RandomState(0), len(x), len(P)) if (e.inStart, e.inEnd) == (env.inStart, env.inEnd)}
    assert {"full", "band0", "stairs"} <= kinds


# ---- the command line ---------------------------------------------------------------------------------------------------------------------
CSV = os.path.join(HERE, "golden", "csv", "tiny_uc.csv")
DNASTORE = os.path.join(HERE, "golden", "machine", "dnastore4.json")


def _run(argv):
    out = io.StringIO()
    boss.run(argv, out)
    return out.getvalue()


@pytest.mark.parametrize("argv", [
    [DNASTORE, "--profile-band", "2", "-L", "--input-chars", "ACGT", "--output-chars", "ACGT"],
    [DNASTORE, "--profile-band", "2", "-L", "--recognize-merge-csv", CSV],
    [DNASTORE, "--profile-band", "2", "-L", "--recognize-csv", CSV, "--recognize-merge-csv", CSV],
    [DNASTORE, "--profile-band", "2", "--recognize-csv", CSV, "--viterbi-decode"],
    [DNASTORE, "--profile-band", "2", "--recognize-csv", CSV, "--prefix-decode"],
    [DNASTORE, "--profile-band", "2", "-L", "--recognize-csv", CSV],
    [DNASTORE, "--profile-band", "2"],
])
def test_profile_band_is_rejected_outside_its_place(argv):
    with pytest.raises(MachineError, match="--profile-band goes with --recognize-csv beside an input sequence"):
        _run(argv)


def test_score_profile_pairs_numpy_band():
    """boss.scoreProfilePairs(band=2) through the numpy backend is PairProfileDP under Envelope.band of each input; an input that
    cannot be tokenised scores -inf; a band does not raise a likelihood."""
    from machineboss_amd.evalmachine import EvaluatedMachine
    from machineboss_amd.machine import Machine
    m = Machine.fromFile(DNASTORE)
    par = m.getParamDefs(True)
    em = EvaluatedMachine.fromMachine(m, par)
    prof = Profile.fromCsv(CSV)
    P = prof.logRows(em)
    dp = PairProfileDP(em)
    seqs = [["0_3", "2_3"], ["0_3", "zz"], ["0_3", "2_3", "1_3"]]
    sc, pc = boss.scoreProfilePairs(m, seqs, prof, backend="numpy", params=par, viterbi=True, counts=True, band=2)
    for k, seq in enumerate(seqs):
        if k == 1:
            assert sc["loglike"][k] == -math.inf and sc["viterbi"][k] == -math.inf
            continue
        x = em.inputTokenizer.tokenize(seq)
        env = Envelope.band(len(x), len(P), 2)
        assert k != 2 or not env.isFull()
        assert sc["loglike"][k] == dp.forward(x, P, env=env)[0] and sc["viterbi"][k] == dp.forward(x, P, "max", env=env)[0]
    assert isinstance(pc, dict)
    full = boss.scoreProfilePairs(m, seqs, prof, backend="numpy", params=par)[0]["loglike"]
    assert all(b <= f + 1e-9 * max(1.0, abs(f)) for b, f in zip(sc["loglike"], full) if f > -math.inf)
    with pytest.raises(MachineError, match="envelopes take plain profiles"):
        boss.scoreProfilePairs(m, seqs, prof, backend="numpy", params=par, merge=True, band=2)
