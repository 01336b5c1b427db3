"""The box-only separating-axis search (marl-hideandseek_amd/csrc/hs_sat_box.h) on the host, no GPU:
tests/host/sat_box_check.cpp includes the header the kernel includes, runs the two lanes' halves one after the other,
combines them and compares code and axis, bit for bit, with the plain sequential search and with the oracle's
collide_hulls (oracle/hs_ref_phys.hpp).  Built with -ffp-contract=off like both sides of the parity tests, and with the
address and undefined-behaviour sanitizers where the host toolchain has their runtimes (plain host code with its own
main), else without."""
import os
import shutil
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "host", "sat_box_check.cpp")
CSRC = os.path.join(ROOT, "marl-hideandseek_amd", "csrc")
CASES = os.path.join(ROOT, "tests", "golden", "narrowphase_cases.npz")
FLAGS = ["-std=c++17", "-O1", "-g", "-ffp-contract=off", "-Wall", "-Werror", "-I", CSRC, "-I", os.path.join(ROOT, "oracle")]
SANITIZE = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all"]
OBJ_CUBE, OBJ_BOX = 2, 7                       # hs_core.h SimObject; half extents: obj_half_extents
HALF = {OBJ_CUBE: (1.0, 1.0, 1.0), OBJ_BOX: (4.0, 0.75, 1.0)}


@pytest.fixture(scope="module")
def program(tmp_path_factory):
    cxx = shutil.which("g++") or shutil.which("c++")
    assert cxx, "no host C++ compiler"
    out = str(tmp_path_factory.mktemp("sat_box") / "sat_box_check")
    if subprocess.run([cxx] + FLAGS + SANITIZE + [SRC, "-o", out], capture_output=True).returncode != 0:
        subprocess.run([cxx] + FLAGS + [SRC, "-o", out], check=True)          # (no sanitizer runtimes here)
    return out


def run(program, *args):
    r = subprocess.run([program, *args], capture_output=True, text=True, timeout=120)
    print(r.stdout, r.stderr)
    assert r.returncode == 0, r.stdout + r.stderr
    return r.stdout


def test_random_box_pairs_match_the_sequential_search_and_the_oracle(program):
    """240 000 random pairs of cubes, long boxes, agents and walls, centres within 1.2 x the sum of the half diagonals.
    The program fails if a result class — separated on a face, separated on an edge, edge contact, face contact with
    reference A, with reference B, counted by the sequential search alone — holds under 1 % of them."""
    assert "random OK" in run(program, "random")


def test_ties_parallel_axes_and_signed_zeros(program):
    """Yaw-only pairs and bodies against walls (cross(z, z) = 0, tying faces), axis-aligned boxes whose overlaps tie
    exactly across the lane split, and +-0 components in centres and quaternions."""
    assert "special OK" in run(program, "special")


def test_the_stored_box_pairs(program, tmp_path):
    """The pairs of tests/golden/narrowphase_cases.npz without a ramp, as float32 poses."""
    g = np.load(CASES)["cases"]
    rows = [r for r in g if int(r[0]) in HALF and int(r[1]) in HALF]
    assert len(rows) >= 400, len(rows)
    path = tmp_path / "box_pairs.txt"
    with open(path, "w") as f:
        for r in rows:
            v = np.float32(np.concatenate([HALF[int(r[0])], r[2:9], HALF[int(r[1])], r[9:16]]))
            f.write(" ".join(f"{x:.9g}" for x in v) + "\n")
    out = run(program, "file", str(path))
    assert "file OK" in out and f"file: {len(rows)} cases" in out
