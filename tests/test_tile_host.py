"""CPU: the strip-plane geometry and the XCD order the kernels compile (os2d_amd/csrc/tile_common.h: os2d_conv_tiles,
os2d_strip_origin, os2d_strip_cell, os2d_tile_cell, os2d_xcd_logical) built for the host and walked tile by tile, cell by cell
(tests/host/tile_check.cpp): R = 2 and 3, widths 1 .. 3600 including 316 | 317 (the first width in strips) and 509 | 510 (the
strip count changes), heights 1 .. 33.  Every data cell is produced by exactly one (tile, cell) with `valid` set, no pad cell is
valid, and os2d_strip_cell of every slab index a tile loads is 0 or the cell the numpy model of test_conv_strips_model.py names."""
import os
import shutil
import subprocess

import numpy as np
import pytest

import test_conv_strips_model as M

REPO = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))


@pytest.fixture(scope="module")
def tile_check(tmp_path_factory):
    cxx = shutil.which("clang++") or "/opt/rocm/lib/llvm/bin/clang++"
    if not os.path.exists(cxx) and shutil.which(cxx) is None:
        pytest.skip("no clang++")
    exe = str(tmp_path_factory.mktemp("tile") / "tile_check")
    subprocess.run([cxx, "-std=c++17", "-O1", "-Wall", "-Werror", "-Wno-unused-function", "-DOS2D_HOST_EMU", "-I", os.path.join(REPO, "os2d_amd", "csrc"),
                    os.path.join(REPO, "tests", "host", "tile_check.cpp"), "-o", exe], check=True, timeout=300)
    return exe


def test_tile_common_geometry_on_the_host(tile_check):
    out = subprocess.run([tile_check], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0 and out.stdout.strip().endswith("ok"), out.stdout[-3000:] + out.stderr[-2000:]
    assert "tile geometry: 144 launches, 0 failed checks" in out.stdout


@pytest.mark.parametrize("H,W,R,halo_round", [(1, 317, 2, 1), (7, 317, 3, 4), (2, 509, 2, 4), (7, 510, 2, 1), (2, 1000, 3, 1), (1, 3600, 2, 4),
                                              (5, 3600, 2, 1)])
def test_strip_cell_of_every_slab_index_is_the_models(tile_check, tmp_path, H, W, R, halo_round):
    path = str(tmp_path / "cells.bin")
    subprocess.run([tile_check, "dump", str(H), str(W), str(R), str(halo_round), path], check=True, timeout=300)
    got = np.fromfile(path, dtype=np.int32)
    NS, SP = M.conv_strips(W, R)
    HALO = (R * SP + R + halo_round - 1) // halo_round * halo_round
    SLAB = M.NT + 2 * HALO
    TPS = (H * SP + M.NT - 1) // M.NT
    want = []
    for tile in range(NS * TPS):
        strip = tile // TPS
        c0mR = strip * (SP - 2 * R) - R
        n0 = (tile - strip * TPS) * M.NT
        want += [M.strip_cell(n0 - HALO + i, SP, c0mR, H, W) for i in range(SLAB)]
    assert got.size == len(want) and (got == np.array(want, dtype=np.int32)).all()
    assert (got != 0).any()
