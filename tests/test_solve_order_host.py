"""The pure parts of the body-body solve order of k_physics (marl-hideandseek_amd/csrc/hs_solve_order.h) on the host, no
GPU: tests/host/solve_order_check.cpp includes the header the kernel includes and compares it with a restatement of
the key ranking and the lane-by-lane exchange that phase_dd used before.  Built with the address and undefined-behaviour
sanitizers where the host toolchain has their runtimes (plain host code with its own main), else without."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "host", "solve_order_check.cpp")
CSRC = os.path.join(ROOT, "marl-hideandseek_amd", "csrc")
FLAGS = ["-std=c++17", "-O1", "-g", "-ffp-contract=off", "-Wall", "-Werror", "-I", CSRC]
SANITIZE = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all"]


@pytest.fixture(scope="module")
def program(tmp_path_factory):
    cxx = shutil.which("g++") or shutil.which("c++")
    assert cxx, "no host C++ compiler"
    out = str(tmp_path_factory.mktemp("solve_order") / "solve_order_check")
    if subprocess.run([cxx] + FLAGS + SANITIZE + [SRC, "-o", out], capture_output=True).returncode != 0:
        subprocess.run([cxx] + FLAGS + [SRC, "-o", out], check=True)          # (no sanitizer runtimes here)
    return out


def run(program, what):
    r = subprocess.run([program, what], capture_output=True, text=True, timeout=120)
    print(r.stdout, r.stderr)
    assert r.returncode == 0, r.stdout + r.stderr
    return r.stdout


def test_candidates_are_filed_in_pair_order(program):
    """200 000 random sets of overlapping slot pairs with 13 .. 17 slots, filed as phase_detect files them (lanes, slot
    groups, partners above the slot, the capacity of 16): the keys (a, b) ascend along the list."""
    assert "filing OK" in run(program, "filing")


def test_kth_accepted_candidate_equals_the_key_ranking(program):
    """kth_set_bit against its definition for every 16-bit mask and every k; and against the ranking of the keys
    (a << 8) | b for every accepted mask on 24 lists of ascending pair codes from 16 and 17 body slots (the first and the
    last sixteen pairs among them, and lists shorter than sixteen)."""
    assert "order OK" in run(program, "order")


def test_dependency_masks_equal_the_shuffle_form(program):
    """Every batch of four pairs over eight bodies (every equality pattern, 614 656 batches) and 400 000 random batches from
    the 136 pairs, with 0 .. 4 valid manifolds, in either half of a row of 16 lanes with another world in the other half:
    the masks from the row-shifted codes equal those from the bodies of lanes 0, 2, 4; pairs_touch on every two pairs;
    the order word round-trips; the spread mask tests the ballot's pending bits."""
    assert "deps OK" in run(program, "deps")
