"""CPU: the register hand-over of the 64-row forward kernel (os2d_amd/csrc/dft_mfma.h: step 1's accumulators are the B operand
of step 2, the complex combination is a lane swap) compiled for the host and run on the SPMD emulator of tests/host/spmd_emu.h
(tests/host/dft_chain_check.cpp): the permuted row operand as dft_matrix_unit builds it, every bin of a 5-channel call (two
iterations of one work-group, the second with one live channel) against a float64 DFT, and the 4-channel call bit-equal to the
first four channels of it."""
import os
import shutil
import subprocess

import pytest

REPO = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))


def test_chained_forward_on_the_host_emulator(tmp_path):
    cxx = shutil.which("clang++") or "/opt/rocm/lib/llvm/bin/clang++"      # ext_vector_type + _Float16: clang
    if not os.path.exists(cxx) and shutil.which(cxx) is None:
        pytest.skip("no clang++")
    exe = str(tmp_path / "dft_chain_check")
    subprocess.run([cxx, "-std=c++17", "-O1", "-pthread", "-Wno-psabi", "-I", os.path.join(REPO, "os2d_amd", "csrc"),
                    "-I", os.path.join(REPO, "tests", "host"), os.path.join(REPO, "tests", "host", "dft_chain_check.cpp"), "-o", exe],
                   check=True, timeout=300)
    out = subprocess.run([exe], capture_output=True, text=True, timeout=600)
    assert out.returncode == 0 and out.stdout.strip().endswith("ok"), out.stdout[-3000:] + out.stderr[-2000:]
    for part in ("operand:", "forward:", "0 bins differ"):
        assert part in out.stdout
