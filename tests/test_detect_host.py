"""CPU: what the detection kernels share (os2d_amd/csrc/detect_common.h - score key, bitonic sort, in-order NMS resolve, IoU
test) compiled for the host and run on the SPMD emulator of tests/host/spmd_emu.h: the sort with the kernels' 1024-thread
work-group against std::stable_sort by descending score (equal scores, +0 / -0, negative scores, invalid entries; 8, 64, 512 and
8192 keys), the resolve of 64 candidates against a scalar greedy NMS on the rounded quotient inter / union > thr, including
pairs that sit at the threshold and all-dead / all-alive masks."""
import os
import shutil
import subprocess

import pytest

REPO = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))


def test_detect_common_on_the_host_emulator(tmp_path):
    cxx = shutil.which("clang++") or "/opt/rocm/lib/llvm/bin/clang++"
    if not os.path.exists(cxx) and shutil.which(cxx) is None:
        pytest.skip("no clang++")
    exe = str(tmp_path / "detect_check")
    # -ffp-contract=off: the scalar reference of the check rounds every product and sum on its own, like the tensor expressions
    # it stands for (the header under test says so itself, per function)
    subprocess.run([cxx, "-std=c++17", "-O1", "-pthread", "-ffp-contract=off", "-DOS2D_HOST_EMU", "-I", os.path.join(REPO, "os2d_amd", "csrc"),
                    "-I", os.path.join(REPO, "tests", "host"), os.path.join(REPO, "tests", "host", "detect_check.cpp"), "-o", exe],
                   check=True, timeout=300)
    out = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0 and out.stdout.strip().endswith("ok"), out.stdout[-3000:] + out.stderr[-2000:]
    assert "sort: 12 cases, 0 failed" in out.stdout and "resolve: 80 batches" in out.stdout
