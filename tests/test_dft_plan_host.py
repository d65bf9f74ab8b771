"""CPU: the planner of the matrix-product transforms (os2d_amd/csrc/dft_plan.h) on its own, tests/host/dft_plan_check.cpp: the
plan of every map of a grid (H 1 .. 100 x W 1 .. 260, four maps of 2784 .. 2785 x 3600 .. 3601, the seven levels of the benchmark
pyramid), both size policies, 4 and 8 images per iteration.  The plans are those of the planner before the LDS layout and the
capacities were written once for planner and kernels - the digest below was recorded from that header (profiles/dft_plan/
README.md has the command) - and each of them is consistent with what the kernels declare: every LDS region ends inside what the
plan budgets for it, every tile / position / item count is within the arrays of a wave and a thread."""
import hashlib
import os
import shutil
import subprocess

import pytest

REPO = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))

LINES = 104044          # 2 policies x (100 x 260 + 4 + 7) maps x 2 images-per-iteration
SHA256 = "e379397c5f2c8667ffc83579d15530ce1b2e2b41887a286bd2d14ade3251baa0"


def test_the_planner_keeps_its_plans_and_they_fit_the_kernels(tmp_path):
    cxx = shutil.which("clang++") or "/opt/rocm/lib/llvm/bin/clang++"
    if not os.path.exists(cxx) and shutil.which(cxx) is None:
        pytest.skip("no clang++")
    exe = str(tmp_path / "dft_plan_check")
    subprocess.run([cxx, "-std=c++17", "-O2", "-pthread", "-I", os.path.join(REPO, "os2d_amd", "csrc"),
                    "-I", os.path.join(REPO, "tests", "host"), os.path.join(REPO, "tests", "host", "dft_plan_check.cpp"), "-o", exe],
                   check=True, timeout=300)
    out = subprocess.run([exe], capture_output=True, timeout=600)
    err = out.stderr.decode()
    assert out.returncode == 0 and " 0 failed" in err and "INCONSISTENT" not in err, err[-3000:]
    assert out.stdout.count(b"\n") == LINES
    assert hashlib.sha256(out.stdout).hexdigest() == SHA256, "the planner's output differs from the recorded plans"
