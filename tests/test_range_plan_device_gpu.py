"""GPU: the range plan of the split-fp16 path computed on the device (os2d_train_range_plan, os2d_amd/csrc_train/range_plan.hip) and the host
route built on it (``TransformationNet.range_plan_device``, ``range_plan_route``).

References: the numpy float64 model (tests/range_plan_model.py) and ``TransformationNet.range_plan`` on the CPU, each computed once
per net.  Integers must be equal - every net first passes the fairness condition of test_range_plan_device_model.py, so a
mismatch is a bug and no boundary flip.  Bounds: relative 1e-11 - the longest sum has 11,025 terms, worst case n * 2^-53 =
1.2e-12, which leaves about 8x for the nested sums of layer 2.  The largest error seen on an MI355X is in
profiles/range_plan_device/test_errors.txt ($OS2D_TEST_ERRORS_FILE names a file the figures are appended to)."""
import copy
import ctypes
import functools
import os

import numpy as np
import pytest
import torch
from torch.utils._python_dispatch import TorchDispatchMode

import range_plan_model as RP
import util
from os2d_amd import _lib, _train_lib
from os2d_amd.utils import synthetic

pytestmark = pytest.mark.gpu

FAIR = 1e-6
BOUND_RTOL = 1e-11
FINITE = [("seeded",) + case for case in RP.SEEDED] + [("degenerate", kind) for kind in RP.DEGENERATE]
NONFINITE = [("nonfinite", kind) for kind in RP.NONFINITE]


def _id(case):
    return "-".join(str(c) for c in case[1:])


@functools.lru_cache(maxsize=None)
def cpu_case(case):
    """(CPU net, model, integers of range_plan(), bounds of range_plan()) - computed once, never written."""
    net = {"seeded": RP.seeded_net, "degenerate": RP.degenerate_net, "nonfinite": RP.nonfinite_net}[case[0]](*case[1:])
    model = RP.plan(*RP.params_of(net))
    assert RP.fairness(model) >= FAIR, RP.fairness(model)
    return (net, model) + RP.reference(net)


def device_net(case, device):
    return copy.deepcopy(cpu_case(case)[0]).to(device).eval()


def call_abi(net, device, stream=None):
    """os2d_train_range_plan through ctypes on the raw parameters -> (rc, exps int32 [520], bounds float64 [192]) device tensors, both
    pre-filled with a pattern no result has."""
    lib = _train_lib.load()
    exps = torch.full((lib.os2d_train_range_plan_ints(),), -12345, dtype=torch.int32, device=device)
    bounds = torch.full((lib.os2d_train_range_plan_doubles(),), -7.0, dtype=torch.float64, device=device)
    args = [net.output_dim]
    for conv, bn in ((net.conv[0], net.conv[1]), (net.conv[3], net.conv[4])):
        args += [_lib.ptr(t.detach()) for t in (conv.weight, conv.bias, bn.weight, bn.bias, bn.running_mean, bn.running_var)]
        args.append(ctypes.c_double(bn.eps))
    with torch.cuda.device(device):
        rc = lib.os2d_train_range_plan(*args, _lib.ptr(net.linear.weight.detach()), _lib.ptr(exps), _lib.ptr(bounds),
                                 stream if stream is not None else _lib.current_stream(device))
    return rc, exps, bounds


def plan_ints(plan, P):
    """The integers of a plan dict in the layout of os2d_train_range_plan."""
    w3 = torch.zeros(8, dtype=torch.int32, device=plan["unit_exp"].device)
    w3[:P] = plan["weight_exp"][2]
    assert plan["in_exp"][0].dtype == torch.int32 and plan["in_exp"][0].cpu().tolist() == [RP.RNORM_EXP] * 225 and plan["out_exp"][2] is None
    assert plan["in_exp"][1] is plan["out_exp"][0] and plan["in_exp"][2] is plan["out_exp"][1]
    return torch.cat([plan["weight_exp"][0], plan["out_exp"][0], plan["unit_exp"], plan["weight_exp"][1], plan["out_exp"][1], w3]).cpu().numpy()


def record(case, err):
    print("range_plan_device bounds: {} max relative error {:.3e} (bound {:.0e})".format(_id(case), err, BOUND_RTOL))
    path = os.environ.get("OS2D_TEST_ERRORS_FILE")
    if path:
        with open(path, "a") as f:
            f.write("{} {:.3e}\n".format(_id(case), err))


@pytest.mark.parametrize("case", FINITE, ids=_id)
def test_abi_and_host_agree_with_model_and_range_plan(case, device):
    _, model, ref_ints, ref_bounds = cpu_case(case)
    net = device_net(case, device)
    rc, exps, bounds = call_abi(net, device)
    assert rc == 0, _train_lib.load().os2d_train_last_error()
    plan = net.range_plan_device()
    torch.cuda.synchronize(device)
    got_ints, got_bounds = exps.cpu().numpy(), bounds.cpu().numpy()
    host_ints, host_bounds = plan_ints(plan, net.output_dim), torch.cat(plan["bounds"]).cpu().numpy()
    assert plan["bounds"][0].dtype == torch.float64 and plan["bounds"][0].shape == (128,) and plan["bounds"][1].shape == (64,)
    assert np.array_equal(got_ints, host_ints) and got_bounds.tobytes() == host_bounds.tobytes()      # ctypes and the method: one kernel
    assert np.array_equal(got_ints, RP.ints(model)), np.nonzero(got_ints != RP.ints(model))
    assert np.array_equal(got_ints, ref_ints), np.nonzero(got_ints != ref_ints)
    want = RP.doubles(model)
    err = float(np.max(np.abs(got_bounds - want) / np.where(want != 0, np.abs(want), 1.0)))
    record(case, err)
    assert err <= BOUND_RTOL and np.array_equal(got_bounds == 0, want == 0)
    np.testing.assert_allclose(got_bounds, ref_bounds, rtol=BOUND_RTOL, atol=0)
    if case[0] == "degenerate":
        assert int(np.abs(got_ints).max()) <= 75 and not got_ints[-8:].any()


@pytest.mark.parametrize("case", NONFINITE, ids=_id)
def test_nonfinite_parameters_give_the_models_integers_and_no_error(case, device):
    _, model, ref_ints, _ = cpu_case(case)
    net = device_net(case, device)
    rc, exps, bounds = call_abi(net, device)
    assert rc == 0, _train_lib.load().os2d_train_last_error()
    host_ints = plan_ints(net.range_plan_device(), net.output_dim)
    torch.cuda.synchronize(device)                                    # no error status: the launches completed
    got = exps.cpu().numpy()
    assert np.array_equal(got, RP.ints(model)) and np.array_equal(got, ref_ints) and np.array_equal(got, host_ints)
    fields = np.split(got, np.cumsum([n for _, n in RP.INT_FIELDS])[:-1])
    for (name, _), values in zip(RP.INT_FIELDS, fields):
        assert int(np.abs(values).max()) <= (75 if name == "unit_exp" else 60), name
    want, have = RP.doubles(model), bounds.cpu().numpy()
    assert np.array_equal(np.isnan(want), np.isnan(have)) and np.array_equal(np.isinf(want), np.isinf(have))


def test_two_calls_give_identical_bytes(device):
    net = device_net(("seeded", "adversarial", 6, 12), device)
    _, e1, b1 = call_abi(net, device)
    _, e2, b2 = call_abi(net, device)
    torch.cuda.synchronize(device)
    assert e1.cpu().numpy().tobytes() == e2.cpu().numpy().tobytes() and b1.cpu().numpy().tobytes() == b2.cpu().numpy().tobytes()
    assert int(e1.min()) > -12345 and float(b1.min()) >= 0.0           # every entry was written


def test_route_switch_and_its_refusal(device, monkeypatch):
    from os2d_amd.modeling import head as head_mod
    net = device_net(("seeded", "plain", 6, 5), device)
    assert net.range_plan_route is None and head_mod.resolve_range_plan_route(None) in head_mod.RANGE_PLAN_ROUTES
    monkeypatch.setenv("OS2D_RANGE_PLAN", "device")
    assert head_mod.resolve_range_plan_route(net.range_plan_route) == "device"
    monkeypatch.setenv("OS2D_RANGE_PLAN", "torch")
    assert head_mod.resolve_range_plan_route(net.range_plan_route) == "torch"
    net.range_plan_route = "device"
    assert head_mod.resolve_range_plan_route(net.range_plan_route) == "device"          # the attribute wins
    monkeypatch.setenv("OS2D_RANGE_PLAN", "host")
    net.range_plan_route = None
    with pytest.raises(ValueError, match="range plan route"):
        net.packed("f16x3")
    net.range_plan_route = "gpu"
    with pytest.raises(ValueError, match="range plan route"):
        net.packed("f16x3")


@pytest.mark.parametrize("kind", ["plain", "adversarial"])
def test_both_routes_give_the_same_packing_spectra_and_head_outputs(kind, device):
    state = cpu_case(("seeded", kind, 6, 11))[0].state_dict()
    outs = {}
    fm = synthetic.make_feature_map(32, 12, 14, seed=3).to(device)
    class_maps = [m.to(device) for m in synthetic.make_class_feature_maps(2, 32, sizes=[(15, 15), (13, 17)], seed=103)]
    for route in ("device", "torch"):
        creator = util.make_head_creator(6, False, state, device)
        net = creator.aligner.parameter_regressor
        net.range_plan_route = route
        with torch.no_grad():
            head = creator.create_os2d_head(class_maps)
            loc, cls, _, corners = head(fm, precision="f16x3")
        outs[route] = dict(packed=net.packed("f16x3"), act=net.activation_exponents(), spectra2=net.spectra2(38, 38), head=(loc, cls, corners))
        assert ("range_plan" in net._packed_cache) == (route == "device")              # the route that ran is the one asked for
    torch.cuda.synchronize(device)
    a, b = outs["device"], outs["torch"]
    assert len(a["packed"]) == 6 and len(a["act"]) == 3
    for name in ("packed", "act", "head"):
        for x, y in zip(a[name], b[name]):
            assert x.dtype == y.dtype and torch.equal(x, y), name
    assert torch.equal(a["spectra2"], b["spectra2"])
    assert bool(torch.isfinite(a["head"][0]).all())


class _OutputDtypes(TorchDispatchMode):
    """Records the dtype of every tensor an aten operator returns."""

    def __init__(self):
        super().__init__()
        self.seen = []

    def __torch_dispatch__(self, func, types, args=(), kwargs=None):
        out = func(*args, **(kwargs or {}))
        for t in (out if isinstance(out, (tuple, list)) else (out,)):
            if isinstance(t, torch.Tensor):
                self.seen.append((str(func), t.dtype))
        return out


def _bump(net):
    with torch.no_grad():
        net.linear.bias.add_(0.0)          # in place: the version changes, the values do not


def test_repack_on_the_device_route_creates_no_float64_tensor(device):
    """What the device route exists for: after a parameter change the next ``packed("f16x3")`` runs no float64 torch operator."""
    net = device_net(("seeded", "plain", 6, 11), device)
    seen = {}
    for route in ("device", "torch"):
        net.range_plan_route = route
        net.packed("f16x3")
        key = net._state_key()
        _bump(net)
        assert net._state_key() != key
        with _OutputDtypes() as mode:
            net.packed("f16x3")
        seen[route] = mode.seen
    torch.cuda.synchronize(device)
    assert seen["device"] and not [s for s in seen["device"] if s[1] == torch.float64], seen["device"]
    assert [s for s in seen["torch"] if s[1] == torch.float64]          # the recorder does see the float64 chain of the torch route


def test_plan_from_a_side_stream_is_consumed_through_its_cache_entry(device):
    case = ("seeded", "adversarial", 4, 13)
    one = device_net(case, device)
    one.range_plan_route = "device"
    want = [t.clone() for t in one.packed("f16x3")] + [t.clone() for t in one.activation_exponents()]
    want_plan = [t.clone() for t in one._range_plan_buffers()]
    two = device_net(case, device)
    two.range_plan_route = "device"
    torch.cuda.synchronize(device)
    side = torch.cuda.Stream(device)
    with torch.cuda.stream(side):
        plan = two.range_plan_device()
    entry = two._packed_cache["range_plan"]
    got = list(two.packed("f16x3")) + list(two.activation_exponents())          # the default stream: waits for the entry's event
    assert two._packed_cache["range_plan"] is entry
    got_plan = list(two._range_plan_buffers())
    torch.cuda.synchronize(device)
    assert plan["unit_exp"].data_ptr() == got_plan[0][256:384].data_ptr()
    for x, y in zip(got + got_plan, want + want_plan):
        assert x.dtype == y.dtype and torch.equal(x, y)
