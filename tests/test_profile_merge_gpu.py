"""GPU tests of CTC-merged profile tapes (mb_profile_merge.hip through capi.DeviceProfiles(colTok=...) and capi.profile_fill_merged):
every device sweep against the numpy restatement profile.MergedProfileDP, in the manner of profhelpers._check_all -- machine sizes on
both sides of the LDS limit, with and without silent edges, three column maps, a batch of unequal lengths, Viterbi ties, bad
arguments."""
import math

import numpy as np
import pytest

from mergehelpers import check_all_merged, merged_rows, quantised_rows
from randmachine import quantised_machine, random_machine
from machineboss_amd import capi
from machineboss_amd.profile import MergedProfileDP

pytestmark = pytest.mark.gpu

PM_LDS_MAX = 160 * 1024                      # mb_profile_merge.hip
LENGTHS = [0, 1, 2, 65, 65]
COLMAPS = {"one": (2, [2]),                  # name: (nOutTok, colTok)
           "four": (4, [1, 2, 3, 4]),        # token order
           "dup5": (4, [3, 1, 4, 1, 2])}     # token 1 heads two columns: they stay two planes


@pytest.fixture(scope="module", autouse=True)
def device():
    if capi.device_count() == 0:
        pytest.fail("no GPU visible")
    capi.set_device(0)
    yield
    capi.set_memory_budget(0)
    capi.set_option("MB_DETERMINISTIC", None)


def machine_for(S, nOut, silent, seed):
    """Cycles, and emitting edges into the end state from a third of the states; with `silent` some silent edges: the default
    silent backbone up to 8 states, a few edges (a handful of levels, a barrier each) beyond."""
    if S <= 8:
        return random_machine(S, 0, nOut, seed, to_end=0.3) if silent else random_machine(S, 0, nOut, seed, silent_density=0.0, backbone=0.0, to_end=0.3)
    return random_machine(S, 0, nOut, seed, density=1.5, silent_density=0.05 if silent else 0.0, backbone=0.0, to_end=0.3)


def batch_for(nCols, seed):
    """Lengths 0, 1, 2, 65, 65 with 20% -inf entries; the blank of the last long profile is kept finite so that it can score."""
    rng = np.random.RandomState(seed)
    profs = [merged_rows(rng, nCols, L, zeros=0.2) for L in LENGTHS]
    profs[-1][:, 0] = np.maximum(profs[-1][:, 0], math.log(0.02))
    return profs


# (S, silent edges, column map, machine seed): seeds at which the restatement scores at least one profile of the batch finite
CASES = [(1, True, "one", 42), (8, True, "four", 52), (8, False, "dup5", 53), (300, True, "dup5", 345), (300, False, "four", 344),
         (300, True, "one", 341), (2000, True, "four", 2044), (2000, False, "four", 2040)]


@pytest.mark.parametrize("S,silent,colmap,seed", CASES, ids=["%d-%s-%s" % (S, "silent" if si else "nosilent", cm) for S, si, cm, _ in CASES])
def test_sweeps_against_restatement(S, silent, colmap, seed):
    """S = 1, 8, 300: the rolling state ((3 (nCols+1) + nCols) S doubles) is in LDS; S = 2 000 at nCols = 4: 304 000 bytes, beyond
    160 KiB -- the per-workgroup slice of global scratch (the rolling Backward's 240 000 bytes too), X of the materialised sweep
    (64 000 bytes) still in LDS."""
    nOut, colTok = COLMAPS[colmap]
    nCols = len(colTok)
    ring = (3 * (nCols + 1) + nCols) * S * 8
    assert (ring > PM_LDS_MAX) == (S == 2000)
    em = machine_for(S, nOut, silent, seed)
    levels = int(em.silentLevels().max(initial=0)) + 1
    assert (levels > 1) == (silent and S > 1) and levels <= 16
    dm, dev, want = check_all_merged(em, colTok, batch_for(nCols, S + nCols))
    assert np.isfinite(want).sum() >= 1


def test_viterbi_ties_first_maximum():
    """Quantised weights ({0, log 1/2, log 1/4, -inf}) at L = 40, token 1 on two columns: the repeat, the blank and the emitting
    candidates tie, and the device traceback must take the documented first maximum as the restatement does."""
    tot = {}
    colTok = [1, 2, 3, 1]
    for seed in range(4):
        em = quantised_machine(12, 0, 3, 600 + seed)
        rng = np.random.RandomState(seed)
        profs = [quantised_rows(rng, len(colTok), 40) for _ in range(12)]
        check_all_merged(em, colTok, profs, fill=(seed == 0))
        dp = MergedProfileDP(em, colTok)
        for P in profs:
            dp.viterbi(P, tot)
    assert tot.get("repeat", 0) >= 5 and tot.get("blank", 0) >= 5 and tot.get("emit", 0) >= 5, tot


def test_bad_arguments():
    em = random_machine(8, 0, 2, 41)
    dm = capi.DeviceMachine(em)
    P = merged_rows(np.random.RandomState(1), 2, 4)
    for colTok in ([0, 1], [1, 3], [-1, 2]):
        with pytest.raises(capi.MbError, match="outside 1..nOutTok"):
            capi.DeviceProfiles(dm, [P], colTok)
        with pytest.raises(capi.MbError, match="outside 1..nOutTok"):
            capi.profile_fill_merged(dm, capi.MB_FORWARD, P, colTok)
    with pytest.raises(capi.MbError, match="columns"):
        capi.DeviceProfiles(dm, [np.zeros((3, 1))], [])
    for bad in (np.nan, np.inf):
        Q = P.copy(); Q[2, 1] = bad
        with pytest.raises(capi.MbError, match="NaN or \\+infinity"):
            capi.DeviceProfiles(dm, [Q], [1, 2])
        with pytest.raises(capi.MbError, match="NaN or \\+infinity"):
            capi.profile_fill_merged(dm, capi.MB_VITERBI, Q, [1, 2])
    with pytest.raises(capi.MbError, match="unknown fill mode"):
        capi.profile_fill_merged(dm, 99, P, [1, 2])
    with pytest.raises(ValueError):
        capi.DeviceProfiles(dm, [np.zeros(7)], [1, 2])      # 7 values are no whole number of 3-column rows
    dev = capi.DeviceProfiles(dm, [P], [1, 2])              # and the library still works
    assert dev.forward().shape == (1,)
