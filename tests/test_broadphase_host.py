"""The pure parts of the k_physics broadphase (marl-hideandseek_amd/csrc/hs_broadphase.h) on the host, no GPU:
tests/host/broadphase_check.cpp includes the header the kernel includes, walks phase_detect's data flow for one world and
compares with the plain loops, bit for bit.  Built with the address and undefined-behaviour sanitizers where the host
toolchain has their runtimes (plain host code with its own main), else without."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "host", "broadphase_check.cpp")
CSRC = os.path.join(ROOT, "marl-hideandseek_amd", "csrc")
FLAGS = ["-std=c++17", "-O1", "-g", "-ffp-contract=off", "-Wall", "-Werror", "-I", CSRC]
SANITIZE = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all"]


@pytest.fixture(scope="module")
def program(tmp_path_factory):
    cxx = shutil.which("g++") or shutil.which("c++")
    assert cxx, "no host C++ compiler"
    out = str(tmp_path_factory.mktemp("broadphase") / "broadphase_check")
    if subprocess.run([cxx] + FLAGS + SANITIZE + [SRC, "-o", out], capture_output=True).returncode != 0:
        subprocess.run([cxx] + FLAGS + [SRC, "-o", out], check=True)          # (no sanitizer runtimes here)
    return out


def run(program, what):
    r = subprocess.run([program, what], capture_output=True, text=True, timeout=120)
    print(r.stdout, r.stderr)
    assert r.returncode == 0, r.stdout + r.stderr
    return r.stdout


def test_strip_masks_then_exact_test_equals_exact_test_on_every_wall(program):
    """100 000 (body AABB, wall set) cases with 4, 32, 33 and 36 walls (and 17, 30): boxes wholly outside the outermost
    boundaries (up to 1e6), across every strip, degenerate, inverted, on strip boundaries, with +-0, +-inf and NaN in
    any field of body or wall.  The program also checks the masks against their definition, that hits occur (on the
    walls beyond the staged 32 too) and that the strips leave less than half of the exact tests."""
    assert "walls OK" in run(program, "walls")


def test_pair_schedule_visits_every_pair_once_and_gives_the_double_loops_masks(program):
    """13 .. 17 slots (16 and 17 are what the kernels run with 5 and 6 agents): every unordered pair exactly once, and on
    random presence, dynamic flags and boxes the masks equal the double loop's, the wrapped hits through the exchange
    words included."""
    assert "pairs OK" in run(program, "pairs")
