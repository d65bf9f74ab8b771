"""CPU: the 64-row plan of os2d_amd/csrc/dft_mfma.h - the forward kernel with the radix-2 column transform (two 32-point
products and a butterfly in step 2) and the inverse kernel - compiled for the host and run on the SPMD emulator of
tests/host/spmd_emu.h against float64 DFTs: each half on its own and the round trip (tests/host/dft_radix2_check.cpp).

Only the FORWARD kernel has the radix-2 step.  The inverse kernel is the dense product: its radix-2 form (a butterfly in front of
step A) was measured slower and lives in tools/patches/dft_inverse_radix2.patch.  The spectrum with Y[u] = -Y[u + 32] at the
largest magnitude - the image that drives such a butterfly to the largest components it can form - is fed to the dense kernel
here all the same (range flag clear, output against float64): the case is kept for the day that patch is revived."""
import os
import shutil
import subprocess

import pytest

REPO = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))


def test_radix2_transforms_on_the_host_emulator(tmp_path):
    cxx = shutil.which("clang++") or "/opt/rocm/lib/llvm/bin/clang++"      # ext_vector_type + _Float16: clang
    if not os.path.exists(cxx) and shutil.which(cxx) is None:
        pytest.skip("no clang++")
    exe = str(tmp_path / "dft_radix2_check")
    subprocess.run([cxx, "-std=c++17", "-O1", "-pthread", "-Wno-psabi", "-I", os.path.join(REPO, "os2d_amd", "csrc"),
                    "-I", os.path.join(REPO, "tests", "host"), os.path.join(REPO, "tests", "host", "dft_radix2_check.cpp"), "-o", exe],
                   check=True, timeout=300)
    out = subprocess.run([exe], capture_output=True, text=True, timeout=600)
    assert out.returncode == 0 and out.stdout.strip().endswith("ok"), out.stdout[-3000:] + out.stderr[-2000:]
    for part in ("forward:", "inverse:", "round trip:"):
        assert part in out.stdout
    assert "flag 0" in out.stdout and "flag 1" not in out.stdout
