"""CPU: the float64 model of the device range plan (tests/range_plan_model.py) against ``TransformationNet.range_plan`` - integer
for integer on the plain, adversarial and degenerate nets, each behind a fairness condition that keeps floor(log2) away from
rounding noise - and the scalar rules of os2d_amd/csrc_train/range_plan_math.h, compiled into a host program, against the model."""
import os
import shutil
import struct
import subprocess

import numpy as np
import pytest

import range_plan_model as RP

REPO = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
FAIR = 1e-6         # log2 distance of every quotient from an integer; float64 summation-order noise is about 1e-12


def check_model_equals_range_plan(net, bounds=True):
    model = RP.plan(*RP.params_of(net))
    assert RP.fairness(model) >= FAIR, RP.fairness(model)          # the fairness condition: a mismatch below is a bug, not a boundary flip
    ref_ints, ref_bounds = RP.reference(net)
    assert RP.ints(model).shape == (RP.INTS,) and np.array_equal(RP.ints(model), ref_ints)
    if bounds:
        np.testing.assert_allclose(RP.doubles(model), ref_bounds, rtol=1e-11, atol=0)
    return model


@pytest.mark.parametrize("kind,P,seed", RP.SEEDED)
def test_model_equals_range_plan(kind, P, seed):
    check_model_equals_range_plan(RP.seeded_net(kind, P, seed))


@pytest.mark.parametrize("kind", RP.DEGENERATE)
def test_model_equals_range_plan_on_degenerate_nets(kind):
    model = check_model_equals_range_plan(RP.degenerate_net(kind))
    assert all(int(np.abs(model[name]).max()) <= 60 for name in ("wexp1", "e1", "wexp2", "e2", "wexp3")) and not model["wexp3"].any()
    if kind != "zero_linear":
        assert model["e1"][3] == 0 and model["wexp1"][3] == 0
    if kind == "huge_conv2":
        assert int(model["e2"].min()) == -60          # the clamp


@pytest.mark.parametrize("kind", RP.NONFINITE)
def test_model_equals_range_plan_on_nonfinite_nets(kind):
    """A NaN or Inf anywhere in a row comes out as the integers ``range_plan`` gives for that row."""
    model = check_model_equals_range_plan(RP.nonfinite_net(kind), bounds=False)
    assert not np.isfinite(RP.doubles(model)).all() or kind == "inf_running_var"        # (an infinite variance folds to a zero scale)
    assert int(np.abs(RP.ints(model)).max()) <= 75          # unit_exp = e1 - 15


def test_route_follows_the_attribute_then_the_environment(monkeypatch):
    from os2d_amd.modeling import head
    monkeypatch.delenv("OS2D_RANGE_PLAN", raising=False)
    assert head.TransformationNet.range_plan_route is None and head.RANGE_PLAN_ROUTES == ("device", "torch")
    assert head.resolve_range_plan_route(None) == head.DEFAULT_RANGE_PLAN == "device"
    monkeypatch.setenv("OS2D_RANGE_PLAN", "torch")
    assert head.resolve_range_plan_route(None) == "torch" and head.resolve_range_plan_route("device") == "device"
    for bad in ("gpu", "", "Device", 1):
        with pytest.raises(ValueError, match="range plan route"):
            head.resolve_range_plan_route(bad)
    monkeypatch.setenv("OS2D_RANGE_PLAN", "host")
    with pytest.raises(ValueError, match="range plan route"):
        head.resolve_range_plan_route(None)


def _bits(x):
    return "{:016x}".format(struct.unpack("<Q", struct.pack("<d", x))[0])


def test_header_rules_equal_the_model(tmp_path):
    """floor_log2 / out_exp / weight_exp of range_plan_math.h as a host program: exact powers of two, one ulp above and below
    them, 0, -1, NaN, +Inf, 1e-300, a subnormal and 1e300 (the clamp), and the layout of the two buffers."""
    cxx = shutil.which("clang++") or "/opt/rocm/lib/llvm/bin/clang++"
    if not os.path.exists(cxx) and shutil.which(cxx) is None:
        pytest.skip("no clang++")
    exe = str(tmp_path / "range_plan_math_check")
    subprocess.run([cxx, "-std=c++17", "-O2", "-I", os.path.join(REPO, "os2d_amd", "csrc_train"),
                    os.path.join(REPO, "tests", "host", "range_plan_math_check.cpp"), "-o", exe], check=True, timeout=120)
    values = []
    for e in (-70, -61, -60, -59, -15, -1, 0, 1, 14, 15, 16, 52, 59, 60, 61, 75, 90):
        p = float(2.0 ** e)
        values += [p, float(np.nextafter(p, np.inf)), float(np.nextafter(p, 0.0))]
    values += [0.0, -1.0, float("nan"), float("inf"), 1e-300, 5e-324, 2.0 ** -1060, 1e300, 3.0, 0.7, 32768.0 / 3.0]
    out = subprocess.run([exe] + [_bits(v) for v in values], capture_output=True, timeout=60, check=True).stdout.decode().split("\n")
    offsets, at = [], 0
    for _, n in RP.INT_FIELDS:
        offsets.append(at)
        at += n
    assert [int(t) for t in out[0].split()] == offsets + [RP.INTS, 0, 128, RP.DOUBLES]
    got = np.array([[int(t) for t in line.split()] for line in out[1:1 + len(values)]])
    x = np.array(values)
    want = np.stack([RP.floor_log2(x), RP.out_exp(x), RP.weight_exp(x)], axis=1)
    assert np.array_equal(got, want), [(v, g, w) for v, g, w in zip(values, got.tolist(), want.tolist()) if g != w]
    # the model itself, spelled out where it matters
    assert RP.floor_log2([1.0, np.nextafter(1.0, 0.0), np.nextafter(1.0, 2.0), 0.0, -1.0, np.nan, np.inf, 1e300, 1e-300, 5e-324]).tolist() == \
        [0, -1, 0, 0, 0, 0, 0, 60, -60, -60]
    assert RP.out_exp([32768.0, 1.0, np.inf, np.nan, 0.0, 1e-300]).tolist() == [0, 15, 0, 0, 0, 60]
    assert RP.weight_exp([16384.0, np.nextafter(16384.0, np.inf), 1.0]).tolist() == [0, -1, 14]
