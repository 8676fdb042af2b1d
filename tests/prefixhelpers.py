"""Machines and node families for the prefix-search tests (not a test module)."""
import numpy as np

from machineboss_amd.evalmachine import EvaluatedMachine, Tokenizer


def populated_machine(S, seed, levels, nIn=2, nOut=2):
    """A random transducer whose prefix-search lattices are well populated, with or without silent levels.

    Every state has two input-free emitting edges per output symbol and one matching edge per input symbol, all to random states,
    one inserting edge (input, no output) and now and then an emitting edge to the end state; with ``levels`` also a silent
    backbone s -> s+1 (chance 0.7) and one silent edge further on.  The output-less weights out of a state (inserting and silent
    edges) are scaled to sum to at most 0.8, so that (I - N)^-1 is a convergent sum and the prefix layer is a real probability
    mass: a child's prefix probability cannot exceed its parent's."""
    rng = np.random.RandomState(seed)
    w = lambda lo, hi: float(np.log(rng.uniform(lo, hi)))
    edges = []
    for s in range(S):
        for o in range(1, nOut + 1):
            for _ in range(2):
                edges.append((s, rng.randint(0, S), 0, o, w(0.1, 0.5)))
        for a in range(1, nIn + 1):
            edges.append((s, rng.randint(0, S), a, rng.randint(1, nOut + 1), w(0.1, 0.9)))
        edges.append((s, rng.randint(0, S), rng.randint(1, nIn + 1), 0, w(0.05, 0.4)))
        if rng.rand() < 0.2:
            edges.append((s, S - 1, 0, rng.randint(1, nOut + 1), w(0.1, 0.5)))
        if levels and s + 1 < S:
            if rng.rand() < 0.7:
                edges.append((s, s + 1, 0, 0, w(0.2, 0.6)))
            edges.append((s, rng.randint(s + 1, S), 0, 0, w(0.05, 0.3)))
    edges.sort(key=lambda e: e[0])
    n = len(edges)
    src = np.array([e[0] for e in edges], np.uint32); dst = np.array([e[1] for e in edges], np.uint32)
    it = np.array([e[2] for e in edges], np.uint16); ot = np.array([e[3] for e in edges], np.uint16)
    lw = np.array([e[4] for e in edges], np.float64)
    mass = np.zeros(S)
    np.add.at(mass, src[ot == 0].astype(np.int64), np.exp(lw[ot == 0]))
    scale = np.where(mass > 0.8, 0.8 / np.maximum(mass, 1e-300), 1.0)
    lw = np.where(ot == 0, lw + np.log(scale[src.astype(np.int64)]), lw)
    off = np.zeros(S + 1, np.int64)
    np.add.at(off, src.astype(np.int64) + 1, 1)
    off = np.cumsum(off)
    tidx = (np.arange(n) - off[src]).astype(np.uint32)
    return EvaluatedMachine(S, Tokenizer([chr(65 + k) for k in range(nIn)]), Tokenizer([chr(97 + k) for k in range(nOut)]),
                            src, dst, it, ot, tidx, lw, off, [None] * S)


def family_paths(nIn):
    """The root, its children and one grandchild of each (the grandchild's token differs from child to child)."""
    toks = list(range(1, nIn + 1))
    return [()] + [(t,) for t in toks] + [(t, toks[t % nIn]) for t in toks]
