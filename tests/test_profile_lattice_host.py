"""The cell index of the pair and two-profile sweeps (machineboss_amd/csrc/mb_profile_lattice.h) and the envelope builder beside it,
checked on the host: tests/cxx/test_lattice.cpp compiles the real header with g++ -- it needs no HIP -- and compares RectCells and
EnvCells with a brute-force membership set: the diagonal runs, inside, index / cell, the line orders of the row posteriors and the
ring slots, over every envelope env_add accepts for I, L <= 4 and over bands with i beyond 64.
"""
import os
import re
import subprocess

from conftest import ROOT


def test_lattice_index_against_brute_force(tmp_path):
    exe = str(tmp_path / "test_lattice")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", "-I", os.path.join(ROOT, "machineboss_amd", "csrc"),
                           os.path.join(ROOT, "tests", "cxx", "test_lattice.cpp"), "-o", exe])
    out = subprocess.run([exe], capture_output=True, text=True)
    assert out.returncode == 0 and out.stdout.startswith("LATTICE OK"), out.stdout[-2000:] + out.stderr[-2000:]
    tally = {k.strip(): int(v) for k, v in re.findall(r"  ([^:]+): (\d+)", out.stdout)}
    # every enumerated st / en was either accepted or rejected with one of the three messages, and each of them occurred
    assert set(tally) == {"accepted", "Envelope/sequence mismatch", "Envelope is not connected", "Envelope is not monotone"}
    assert all(v > 0 for v in tally.values())
