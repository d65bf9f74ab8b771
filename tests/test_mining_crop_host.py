"""CPU: the crop placement of hard-patch mining (os2d_amd/csrc_train/mining_crop.h: os2d_floor_div, os2d_crop_axis,
os2d_mine_crop_box with the box-op chains of csrc/detect_common.h) compiled for the host and run over every geometry of
tests/mining_stage_cases.py - strides that are no power of two, odd crops, images that are no multiple of the stride, crops larger
than the image on one axis, a 3,600 px level, chains of up to six ops - against the fixture recorded from the reference
(tests/golden/mining_geometry.npz) and the loop model (tests/mining_stage_model.py), bit for bit."""
import os
import shutil
import subprocess

import numpy as np
import pytest

import mining_stage_cases as SC

REPO = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))


def bits(v):
    return "{:08x}".format(int(np.float32(v).view(np.uint32)))


def table_text():
    lines = [str(len(SC.GEOMETRIES))]
    for g in SC.GEOMETRIES:
        ops, _ = SC.chain_ops(g["steps"], g["img"])
        lines.append(" ".join(str(v) for v in (g["H"], g["W"], g["stride"], g["box"], g["img"][0], g["img"][1], g["crop"][0], g["crop"][1],
                                                len(ops))))
        lines.extend("{} {} {}".format(kind, bits(ax), bits(ay)) for kind, ax, ay in ops)
    return "\n".join(lines) + "\n"


def test_mining_crop_header_on_the_host(tmp_path):
    cxx = shutil.which("clang++") or "/opt/rocm/lib/llvm/bin/clang++"
    if not os.path.exists(cxx) and shutil.which(cxx) is None:
        pytest.skip("no clang++")
    exe, table, out = str(tmp_path / "mining_crop_check"), str(tmp_path / "table.txt"), str(tmp_path / "boxes.bin")
    # -ffp-contract=off: every product and difference of the placement is rounded on its own (the header says so per function)
    subprocess.run([cxx, "-std=c++17", "-O1", "-ffp-contract=off", "-DOS2D_HOST_EMU", "-I", os.path.join(REPO, "os2d_amd", "csrc_train"),
                    os.path.join(REPO, "tests", "host", "mining_crop_check.cpp"), "-o", exe], check=True, timeout=300)
    with open(table, "w") as f:
        f.write(table_text())
    run = subprocess.run([exe, table, out], capture_output=True, text=True, timeout=300)
    assert run.returncode == 0 and run.stdout.strip().endswith("ok"), run.stdout[-3000:] + run.stderr[-2000:]
    got = np.fromfile(out, np.float32).reshape(-1, 8)
    assert got.shape[0] == sum(g["H"] * g["W"] for g in SC.GEOMETRIES)
    fx = np.load(os.path.join(REPO, "tests", "golden", "mining_geometry.npz"), allow_pickle=False)
    assert fx["names"].tolist() == [g["name"] for g in SC.GEOMETRIES]
    pos, chained, wrong = 0, 0, []
    for g in SC.GEOMETRIES:
        n = g["H"] * g["W"]
        crops, anchors = got[pos:pos + n, :4], got[pos:pos + n, 4:]
        pos += n
        model_crops, model_anchors, _, _ = SC.geometry_model(g["name"])
        same = (SC.same_bits(crops, fx["crop_" + g["name"]]) and SC.same_bits(anchors, fx["anchor_" + g["name"]])       # the reference
                and SC.same_bits(crops, model_crops) and SC.same_bits(anchors, model_anchors))                         # the loop model
        if not same:
            wrong.append(g["name"])
        chained += len(g["steps"]) == SC.MAX_OPS
    assert not wrong, wrong
    assert chained >= 4 and SC.EXCLUDED == 0
