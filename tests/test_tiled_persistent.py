"""Persistent strips of the pipelined materialised Forward (machineboss_amd/csrc/mb_medium.hip forward_persistent, the MED_MAT_PERSIST
kernel of mb_medium_jit.cpp): one grid in which every workgroup takes a (pair, strip) ticket and sweeps the whole strip, halo states
handed over through a halo column per strip.  Checked against the launch-by-launch pipeline (MB_MEDIUM_PERSIST=0) bit for bit, and
the host's plan without a device: a ticket only ever waits for lower tickets."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import golden_path

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def capi():
    from machineboss_amd import capi as c
    if c.device_count() == 0:
        pytest.fail("no GPU visible: -m gpu tests must run on the MI355X box")
    return c


def plan(in_lens, out_lens, C_, n_slots):
    from machineboss_amd import capi
    L = capi.load()
    f = L.mb_debug_persist_plan
    f.restype = C.c_int64
    f.argtypes = [C.c_int64, C.POINTER(C.c_int32), C.POINTER(C.c_int32), C.c_int32, C.c_int64, C.POINTER(C.c_int32), C.c_int64, C.POINTER(C.c_int32)]
    n = len(in_lens)
    a = np.asarray(in_lens, dtype=np.int32); b = np.asarray(out_lens, dtype=np.int32)
    cap = int(sum((x + C_) // C_ for x in in_lens))
    tk = np.zeros(2 * max(cap, 1), dtype=np.int32); w = np.zeros(2 * max(n, 1), dtype=np.int32)
    p32 = C.POINTER(C.c_int32)
    got = f(n, a.ctypes.data_as(p32), b.ctypes.data_as(p32), C_, n_slots, tk.ctypes.data_as(p32), cap, w.ctypes.data_as(p32))
    assert got == cap
    return tk[:2 * got].reshape(-1, 2), w[:2 * n].reshape(-1, 2)


@pytest.mark.parametrize("n_slots", [1, 3, 24])
def test_persistent_plan_waits_on_lower_tickets_only(n_slots):
    rng = np.random.default_rng(n_slots)
    in_lens = [int(x) for x in rng.integers(0, 700, 40)] + [487] * 8
    out_lens = [int(x) for x in rng.integers(0, 3000, 48)]
    C_ = 32
    tk, w = plan(in_lens, out_lens, C_, n_slots)
    index = {(int(p), int(a)): k for k, (p, a) in enumerate(tk)}
    assert len(index) == len(tk) == sum((x + C_) // C_ for x in in_lens)
    finished = {}                                        # slot -> tickets of the pairs dealt to it so far
    for p in range(len(in_lens)):
        slot, need = int(w[p, 0]), int(w[p, 1])
        assert slot == p % n_slots
        before = finished.setdefault(slot, [])
        assert need == len(before)                       # the count the pair waits for is exactly its slot's earlier strips ...
        first = index[(p, 0)]
        assert all(k < first for k in before)            # ... every one of them a lower ticket
        NA = (in_lens[p] + C_) // C_
        for a in range(NA):
            k = index[(p, a)]
            if a > 0:
                assert index[(p, a - 1)] < k             # the strip to the left: a lower ticket
        before.extend(index[(p, a)] for a in range(NA))


def _batch(capi, em, shapes, n_out=None, seed=0):
    from machineboss_amd.seqgen import synth_tokens
    pairs = [synth_tokens(seed + k, i, o, em.nInTok, n_out or em.nOutTok) for k, (i, o) in enumerate(shapes)]
    return capi.DeviceBatch.from_pairs(capi.DeviceMachine(em), pairs)


def _both(capi, b, budget):
    """log-likelihoods launch by launch and through the persistent strips, with the matrices of the batch over the budget"""
    capi.set_memory_budget(budget)
    try:
        capi.set_option("MB_MEDIUM_PERSIST", "0")
        tiles = b.forward(capi.MB_MATERIALISE); n_tiles = capi.last_launch_count()
        capi.set_option("MB_MEDIUM_PERSIST", "1")
        pers = b.forward(capi.MB_MATERIALISE); n_pers = capi.last_launch_count()
    finally:
        capi.set_option("MB_MEDIUM_PERSIST", None)
        capi.set_memory_budget(0)
    return tiles, n_tiles, pers, n_pers


@pytest.mark.gpu
def test_persistent_strips_match_tiles_more_pairs_than_slots(capi, machines):
    m, em = machines("psw2dna", None, useDefaults=True, preset=True)
    b = _batch(capi, em, [(487, 1500)] * 24)
    one = (487 + 1) * (1500 + 1) * em.nStates * 8
    tiles, n_tiles, pers, n_pers = _both(capi, b, 5 * one)     # five matrix slots for 24 pairs
    assert n_tiles > 50 and n_pers == 1, (n_tiles, n_pers)
    assert np.array_equal(tiles, pers) and np.all(np.isfinite(pers))


@pytest.mark.gpu
def test_persistent_strips_match_tiles_ragged(capi, machines):
    """ragged lengths, pairs narrower than one strip, empty outputs, and two pairs through ONE matrix slot"""
    m, em = machines("psw2dna", None, useDefaults=True, preset=True)
    b = _batch(capi, em, [(487, 1500), (20, 900), (100, 1), (5, 3), (300, 1200), (0, 40), (31, 0), (200, 700)], seed=7)
    one = (487 + 1) * (1500 + 1) * em.nStates * 8
    tiles, n_tiles, pers, n_pers = _both(capi, b, int(1.2 * one))    # (the batch's matrices: 1.7 of the largest)
    assert n_pers == 1 and np.array_equal(tiles, pers)
    b2 = _batch(capi, em, [(487, 1500), (400, 1100)], seed=11)
    tiles, n_tiles, pers, n_pers = _both(capi, b2, int(1.5 * one))   # one slot: the second pair waits for every strip of the first
    assert n_pers == 1 and np.array_equal(tiles, pers)


@pytest.mark.gpu
def test_persistent_strips_match_tiles_482_states(capi):
    from machineboss_amd import algebra
    from machineboss_amd.evalmachine import EvaluatedMachine
    em = EvaluatedMachine.fromMachine(algebra.config4bMachine(golden_path("preset")), None, useDefaults=True)
    assert em.nStates == 482
    b = _batch(capi, em, [(300, 600), (150, 500), (300, 300), (64, 600)], n_out=3, seed=3)
    one = (300 + 1) * (600 + 1) * em.nStates * 8
    tiles, n_tiles, pers, n_pers = _both(capi, b, 2 * one)      # (the batch's matrices: 2.9 of the largest)
    assert np.array_equal(tiles, pers) and np.all(np.isfinite(pers))


@pytest.mark.gpu
def test_persistent_strips_fall_back_when_a_row_never_arrives():
    """A wait that runs out (a shared device; here: a bound of one microsecond) raises the call's error word: the host latches the form
    off for the machine, runs the call again launch by launch with the right answer and one warning, and later calls stay there."""
    code = """
import sys, numpy as np
sys.path.insert(0, %r)
from machineboss_amd import capi
from machineboss_amd.machine import Machine
from machineboss_amd.evalmachine import EvaluatedMachine
from machineboss_amd.seqgen import synth_tokens
em = EvaluatedMachine.fromMachine(Machine.fromFile(%r), None, useDefaults=True)
pairs = [synth_tokens(50 + k, 487, 1500, em.nInTok, em.nOutTok) for k in range(12)]
dm = capi.DeviceMachine(em); b = capi.DeviceBatch.from_pairs(dm, pairs)
capi.set_memory_budget(4 * 488 * 1501 * em.nStates * 8)
capi.set_option("MB_MEDIUM_PERSIST", "0"); ref = b.forward(capi.MB_MATERIALISE); n0 = capi.last_launch_count()
capi.set_option("MB_MEDIUM_PERSIST", "1"); ok = b.forward(capi.MB_MATERIALISE); n1 = capi.last_launch_count()
capi.set_option("MB_MEDIUM_PERSIST_TIMEOUT_US", "1")
got = b.forward(capi.MB_MATERIALISE); n2 = capi.last_launch_count()
capi.set_option("MB_MEDIUM_PERSIST_TIMEOUT_US", "0")
again = b.forward(capi.MB_MATERIALISE); n3 = capi.last_launch_count()
assert n0 > 10 and n1 == 1 and n2 > 10 and n3 > 10, (n0, n1, n2, n3)
assert np.array_equal(ref, ok) and np.array_equal(ref, got) and np.array_equal(ref, again)
print("FELL BACK")
""" % (ROOT, golden_path("preset", "psw2dna.json"))
    r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and "FELL BACK" in r.stdout, (r.stdout + r.stderr)[-2000:]
    assert r.stderr.count("run again launch by launch") == 1
