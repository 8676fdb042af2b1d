"""GPU tests of profile tapes (mb_profile.hip through capi.DeviceProfiles and `boss --recognize-csv`): the device sweeps against the
numpy restatement (machineboss_amd/profile.py), one-hot profiles against the token sweeps, the reference's CLI goldens."""
import json
import math
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import ROOT, golden_path, load_json
from profhelpers import _check_all, _close, _profiles
from randmachine import random_machine
from machineboss_amd import algebra, capi
from machineboss_amd.evalmachine import EvaluatedMachine
from machineboss_amd.machine import Machine

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module", autouse=True)
def device():
    if capi.device_count() == 0:
        pytest.fail("no GPU visible")
    capi.set_device(0)
    yield
    capi.set_memory_budget(0)
    capi.set_option("MB_DETERMINISTIC", None)


@pytest.mark.parametrize("S,nOut,seed", [(8, 2, 1), (8, 4, 2), (300, 4, 3), (2000, 4, 4)])
def test_random_generators_against_restatement(S, nOut, seed):
    em = random_machine(S, 0, nOut, seed)
    _check_all(em, _profiles(em, [0, 5, 17, 1, 0, 40, 3], seed))


def test_fn3_translate_against_restatement():
    em = EvaluatedMachine.fromMachine(Machine.fromFile(golden_path("js", "machines", "fn3-3-translate.json")), None, useDefaults=True)
    _check_all(em, _profiles(em, [30, 0, 12], 7, zeros=0.0))


def test_scratch_path_beyond_lds():
    """7 000 states: the three rolling state vectors (168 KB) do not fit 160 KiB of LDS -- per-workgroup global scratch."""
    em = random_machine(7000, 0, 3, 11, density=1.0, silent_density=0.3)
    _check_all(em, _profiles(em, [6, 0, 9], 11), fill=False)


def test_deterministic_counts_and_chunking():
    em = random_machine(300, 0, 4, 21)
    profs = _profiles(em, [25, 0, 14, 30, 7, 19], 21)
    dm = capi.DeviceMachine(em)
    dev = capi.DeviceProfiles(dm, profs)
    capi.set_option("MB_DETERMINISTIC", "1")
    try:
        c1 = dev.counts()[0]; c2 = dev.counts()[0]
    finally:
        capi.set_option("MB_DETERMINISTIC", None)
    assert np.array_equal(c1, c2)
    f0, (v0, o0, e0, r0), c0 = dev.forward(capi.MB_MATERIALISE), dev.viterbi(), dev.counts()[0]
    capi.set_memory_budget(2 * 31 * 2 * 300 * 8 + 300 * 8 * 4)    # two of the longest lattices: several chunks
    try:
        f1, (v1, o1, e1, r1), c1 = dev.forward(capi.MB_MATERIALISE), dev.viterbi(), dev.counts()[0]
    finally:
        capi.set_memory_budget(0)
    assert np.array_equal(f0, f1) and np.array_equal(v0, v1) and np.array_equal(o0, o1) and np.array_equal(e0, e1) and np.array_equal(r0, r1)
    assert np.allclose(c0, c1, rtol=1e-12, atol=1e-15)


def test_one_hot_profiles_equal_token_path():
    em = random_machine(40, 0, 3, 31)
    rng = np.random.RandomState(31)
    seqs = [rng.randint(1, 4, n) for n in (0, 1, 9, 23)]
    profs = []
    for y in seqs:
        P = np.full((len(y), 4), -np.inf)
        P[np.arange(len(y)), y] = 0.0
        profs.append(P)
    dm = capi.DeviceMachine(em)
    dev = capi.DeviceProfiles(dm, profs)
    b = capi.DeviceBatch.from_pairs(dm, [([], y) for y in seqs])
    # (the token sweeps add the log-sum-exp correction term in fp32, mb_device_math.h: a few 1e-8 relative)
    assert _close(dev.forward(), b.forward(capi.MB_ROLLING), 1e-6)
    assert np.array_equal(dev.viterbi(paths=False)[0], b.viterbi(paths=False)[0])
    assert np.allclose(dev.counts()[0], b.counts()[0], rtol=1e-6, atol=1e-9)


def _boss(*args):
    r = subprocess.run([sys.executable, "-m", "machineboss_amd.boss"] + list(args), cwd=ROOT, capture_output=True, text=True, timeout=300)
    return r.returncode, r.stdout, r.stderr


@pytest.mark.parametrize("seq,csv,expect", [("tiny_uc.json", "tiny_uc.csv", "tiny_uc"), ("tiny_lc.json", "tiny_uc.csv", "tiny_uc_fail"),
                                            ("empty.json", "tiny_uc.csv", "tiny_empty"), ("nanopore_test_seq.json", "nanopore_test.csv", "nanopore_test")])
def test_cli_goldens(seq, csv, expect):
    rc, out, err = _boss("-L", "--generate-json", "tests/golden/io/" + seq, "--recognize-csv", "tests/golden/csv/" + csv)
    assert rc == 0, err
    got = [[t[2]] for t in json.loads(out)]     # js/stripnames.js
    want = load_json("expect", expect + ".json")
    if want[0][0] == "-Infinity":
        assert got == want
    else:
        assert abs(got[0][0] - want[0][0]) <= 1e-4 * abs(want[0][0]), (got, want)


def test_cli_counts_profile_equals_tokens():
    rc, a, err = _boss("--generate-chars", "101", "tests/golden/machine/bitnoise.json", "--recognize-csv", "tests/golden/csv/prof001.csv",
                       "-P", "tests/golden/io/params.json", "-C")
    assert rc == 0, err
    rc, b, err = _boss("tests/golden/machine/bitnoise.json", "--input-chars", "101", "--output-chars", "001", "-P", "tests/golden/io/params.json", "-C")
    assert rc == 0, err
    ja, jb = json.loads(a), json.loads(b)
    assert ja.keys() == jb.keys() and all(abs(ja[k] - jb[k]) <= 1e-5 * max(1.0, abs(jb[k])) for k in jb), (ja, jb)
    rc, v, err = _boss("--generate-chars", "101", "tests/golden/machine/bitnoise.json", "--recognize-csv", "tests/golden/csv/prof001.csv",
                       "-P", "tests/golden/io/params.json", "-V")
    assert rc == 0, err
    rc, w, err = _boss("tests/golden/machine/bitnoise.json", "--input-chars", "101", "--output-chars", "001", "-P", "tests/golden/io/params.json", "-V")
    assert rc == 0, err
    assert json.loads(v)[0][2] == json.loads(w)[0][2]


def test_rejections():
    em = random_machine(8, 0, 2, 41)
    dm = capi.DeviceMachine(em)
    bad = _profiles(em, [4], 41)[0]
    bad[2, 1] = np.nan
    with pytest.raises(capi.MbError, match="NaN"):
        capi.DeviceProfiles(dm, [bad])
    with pytest.raises(ValueError):
        capi.DeviceProfiles(dm, [np.zeros(7)])       # 7 values are no whole number of 3-column rows
    with pytest.raises(capi.MbError):
        capi.profile_fill(dm, capi.MB_FORWARD, np.array([[0.0, math.inf, 0.0]]))
    rc, _, err = _boss("tests/golden/machine/bitnoise.json", "--recognize-csv", "tests/golden/csv/prof001.csv", "-L")
    assert rc == 1 and "empty input alphabet" in err
