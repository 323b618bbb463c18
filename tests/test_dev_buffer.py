"""The owning buffer type behind every device and pinned allocation of a context (cmc_fluid_solver_amd/csrc/fs3d_buf.h), on a CPU.

tests/dev_buffer_test.cpp instantiates it on a malloc policy that counts live and total allocations and can fail the N-th one.
It is built once with the address and undefined-behaviour sanitizers and run as a program of its own, one case per run; a
violated statement and any sanitizer report (a leak, a double free, a use after free) end the run with a non-zero status.
"""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

CASES = ["default_and_reset", "reserve_grows_only", "replace_is_exact", "failure_leaves_it_empty", "all_or_nothing", "moves"]


@pytest.fixture(scope="module")
def program(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("dev_buffer") / "dev_buffer_test")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           os.path.join(ROOT, "tests", "dev_buffer_test.cpp"), "-o", exe])
    return exe


@pytest.mark.parametrize("case", range(1, len(CASES) + 1), ids=CASES)
def test_buffer(program, case):
    r = subprocess.run([program, str(case)], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0, r.stdout + r.stderr
    assert r.stdout.startswith("case %d ok" % case), r.stdout      # nothing live after the case went out of scope
