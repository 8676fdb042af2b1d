"""Profiles and the composite machine for the tests of decoding against a profile (not a test module)."""
import numpy as np

from machineboss_amd import prefixtree
from machineboss_amd.evalmachine import EvaluatedMachine, Tokenizer


def random_profile(rng, L, nOut, pZero=0.2):
    """[L, nOut + 1] log weights: uniform(0.05, 1), symbol entries zeroed with chance ``pZero``, the blank (column 0) always positive."""
    w = rng.uniform(0.05, 1.0, (L, nOut + 1))
    zero = rng.rand(L, nOut + 1) < pZero
    zero[:, 0] = False
    with np.errstate(divide="ignore"):
        return np.log(np.where(zero, 0.0, w))


def hard_profile(y, nOut):
    """The token string y as a profile: weight 1 on its symbol per row, 0 elsewhere, blank 0."""
    P = np.full((len(y), nOut + 1), -np.inf)
    P[np.arange(len(y)), np.asarray(y, np.int64)] = 0.0
    return P


def composite_machine(em, P, origins=False):
    """compose(M, profile recogniser) built directly, no output alphabet.  The composition makes the recogniser a waiting
    machine: a row r = 0..L has an ARRIVED stage, where only the blank may fire, and a WAITING stage, where M moves.  State
    (r*2 + stage)*S + q.  arrived (q, r) -> arrived (q, r+1) is the blank at weight P[r][0], arrived (q, r) -> waiting (q, r) is
    free; an M edge without output stays in the waiting stage of its row, one with output o goes from waiting (s, r) to arrived
    (d, r+1) at weight w + P[r][o].  Edges of weight -inf are left out.  Every silent edge keeps source < destination.
    ``origins``: also return, per edge of the composite, the edge of ``em`` it came from (-1 for a blank or a free move)."""
    P = np.asarray(P, np.float64).reshape(-1, em.nOutTok + 1)
    L, S = len(P), em.nStates
    src, dst, it, ot, w = (em.src.astype(np.int64), em.dst.astype(np.int64), em.inTok.astype(np.int64), em.outTok.astype(np.int64),
                           em.logWeight)
    quiet, loud = ot == 0, ot > 0
    eid = np.arange(len(src))
    q = np.arange(S)
    rows = []
    for r in range(L + 1):
        arrived, waiting = 2 * r * S, (2 * r + 1) * S
        rows.append((arrived + q, waiting + q, np.zeros(S, np.int64), np.zeros(S), np.full(S, -1)))
        rows.append((waiting + src[quiet], waiting + dst[quiet], it[quiet], w[quiet], eid[quiet]))
        if r < L:
            rows.append((waiting + src[loud], arrived + 2 * S + dst[loud], it[loud], w[loud] + P[r][ot[loud]], eid[loud]))
            rows.append((arrived + q, arrived + 2 * S + q, np.zeros(S, np.int64), np.full(S, P[r][0]), np.full(S, -1)))
    cs, cd, ci, cw, co = (np.concatenate(c) for c in zip(*rows))
    keep = cw > -np.inf
    order = np.argsort(cs[keep], kind="stable")
    cs, cd, ci, cw, co = cs[keep][order], cd[keep][order], ci[keep][order], cw[keep][order], co[keep][order]
    n = 2 * (L + 1) * S
    off = np.zeros(n + 1, np.int64)
    np.add.at(off, cs + 1, 1)
    off = np.cumsum(off)
    tidx = (np.arange(len(cs)) - off[cs]).astype(np.uint32)
    C = EvaluatedMachine(n, em.inputTokenizer, Tokenizer([]), cs.astype(np.uint32), cd.astype(np.uint32), ci.astype(np.uint16),
                         np.zeros(len(cs), np.uint16), tidx, cw, off, [None] * n)
    return (C, co) if origins else C


def composite_seq_cells(cells, L, S):
    """W[r][q] out of the token search's lattice on the composite (one row): the seq cells of the waiting stages."""
    return cells[0, 0].reshape(L + 1, 2, S)[:, 1]


def all_paths(nIn, depth=2):
    """Every input prefix up to ``depth`` symbols, shortest first."""
    out = [()]
    for _ in range(depth):
        out += [p + (t,) for p in out if len(p) == len(out[-1]) for t in range(1, nIn + 1)]
    return out


def composite_fills(C, paths):
    """{path: (cells[1][2][(L+1) S], logSeqProb, logPrefixProb)} of the token search on C with an empty output."""
    dp = prefixtree.PrefixDP(C)
    out = {}
    for p in sorted(paths, key=len):
        out[p] = dp.fill([]) if not p else dp.fill([], out[p[:-1]][0], p[-1])
    return out


def profile_fills(em, P, paths, logR=None):
    dp = prefixtree.ProfilePrefixDP(em, logR)
    out = {}
    for p in sorted(paths, key=len):
        out[p] = dp.fill(P) if not p else dp.fill(P, out[p[:-1]][0], p[-1])
    return out


# ---- the edge suite (test_prefix_edges_gpu.py, test_prefix_host.py::test_edge_suite_inputs_are_live) --------------------------------
def edge_profile(S, nOut, L=33):
    """The profile of the case of prefixhelpers.EDGE_CASES with S states."""
    return random_profile(np.random.RandomState(S + L), L, nOut)


def lds_profile_states(nOut, ldsBytes):
    """The largest S with 3 S + nOut + 1 doubles within ``ldsBytes`` (what k_prefix_fill_profile keeps in LDS)."""
    return (ldsBytes // 8 - (nOut + 1)) // 3


def lds_profile(S, nOut, L=4):
    return random_profile(np.random.RandomState(S), L, nOut, pZero=0.0)


def batch_profiles(nOut=5, lengths=tuple(range(10))):
    return [random_profile(np.random.RandomState(20 + L), L, nOut) for L in lengths]


def far_column_profile():
    """Two rows that read mostly a, then mostly b (prefixhelpers.far_column_case)."""
    return np.log(np.array([[0.1, 0.8, 0.1], [0.1, 0.1, 0.8]]))


SPARSE_SEED = 0
DEAD_ROW = 16


def sparse_profile(L, nOut, seed=SPARSE_SEED):
    """About a third of the symbol weights are -inf, and the blank of about a third of the rows."""
    rng = np.random.RandomState(seed)
    w = rng.uniform(0.05, 1.0, (L, nOut + 1))
    with np.errstate(divide="ignore"):
        return np.log(np.where(rng.rand(L, nOut + 1) < 1.0 / 3.0, 0.0, w))


def dead_row_profile(L, nOut, seed=1):
    """A dense profile whose row DEAD_ROW is -inf throughout: nothing passes it."""
    P = random_profile(np.random.RandomState(seed), L, nOut, pZero=0.0)
    P[DEAD_ROW] = -np.inf
    return P


def twin_profiles(em, outs, sharp=0.8):
    """Soft versions of output strings: ``sharp`` on the symbol, the rest spread over the other symbols and the blank."""
    profs = []
    for o in outs:
        y = em.outputTokenizer.tokenize(list(o))
        W = np.full((len(y), em.nOutTok + 1), (1.0 - sharp) / em.nOutTok)
        W[np.arange(len(y)), y] = sharp
        profs.append(np.log(W))
    return profs
