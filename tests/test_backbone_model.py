"""CPU: the float64 models of the backbone's fused inference route (tests/backbone_model.py) against the torch module, the BatchNorm
fold, which calls take the route, what the fold cache leaves alone, and libos2d_backbone.so held to what every library of the
project is held to (tests/test_native_libs.py): record, header, binding and exports agree, bad arguments are refused before any
launch."""
import ctypes
import os
import re
import subprocess

import pytest
import torch

import backbone_model as B

REPO = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
fake = ctypes.c_void_p(4096)          # never dereferenced: the calls below are refused by their argument checks


@pytest.fixture(scope="module")
def extractor():
    from os2d_amd.modeling.feature_extractor import resnet50_c4
    torch.manual_seed(0)
    ex = resnet50_c4().eval()
    B.perturb_batchnorms(ex, seed=1)
    return ex


def test_fold_is_the_float64_formula_rounded_once(extractor):
    from os2d_amd.modeling import backbone_fused
    layers = backbone_fused.norm_layers(extractor)
    assert len(layers) == 43 and layers[0] is extractor.bn1 and sum(m.num_features for m in layers) == 15296
    folds = extractor.fused_backbone().folds(torch.device("cpu"))
    buffer = extractor.fused_backbone()._buffer
    assert buffer.dtype == torch.float32 and tuple(buffer.shape) == (2, 15296)
    for m in layers:
        s64, t64 = B.fold64(m.weight.detach(), m.bias.detach(), m.running_mean, m.running_var, m.eps)
        s, t = backbone_fused.fold_batchnorm(m.weight.detach(), m.bias.detach(), m.running_mean, m.running_var, m.eps)
        assert s.dtype == t.dtype == torch.float32
        assert bool(((s.double() - s64).abs() <= B.ulp32(s64)).all()) and bool(((t.double() - t64).abs() <= B.ulp32(t64)).all())
        # all layers live in the one buffer, and the views are this fold
        vs, vt = folds[id(m)]
        assert torch.equal(vs, s) and torch.equal(vt, t)
        assert vs.untyped_storage().data_ptr() == vt.untyped_storage().data_ptr() == buffer.untyped_storage().data_ptr()


def test_chained_models_reproduce_the_float64_module(extractor):
    """The chain with unrounded folds IS the module in other words: only float64 rounding separates them.  Bound: about 50 layers,
    each a sum of at most 4608 products rounded to 2^-53 relative, is 3e-11 of the sum of magnitudes; a factor 40 for cancellation
    gives 1e-9 of the largest output - four orders below one fp32 rounding, which is what the GPU tests resolve."""
    x = torch.randn(2, 3, 64, 96, generator=torch.Generator().manual_seed(2))
    want = B.module_forward64(extractor, x)
    got = B.extractor_forward64(extractor, x, fold32=B.fold_exact)
    assert tuple(got.shape) == tuple(want.shape) == (2, 1024, 4, 6)
    err, top = float((got - want).abs().max()), float(want.abs().max())
    print("float64 chain against float64 module: {:.3g} at max |y| {:.4g}".format(err, top))
    assert top > 1.0 and err <= 1e-9 * top
    # fp32 folds move the result by fp32 roundings of s and t, no more: 43 folds, each 2^-24 relative, amplified like the signal
    rounded = B.extractor_forward64(extractor, x)
    assert 0 < float((rounded - want).abs().max()) <= 1e-4 * top


def test_models_special_values():
    x = torch.tensor([[[[-1.0, -2.0, -3.0], [-4.0, float("nan"), -6.0], [-7.0, -8.0, -9.0], [-1.0, -1.0, -1.0], [-1.0, -1.0, -1.0]]]])
    one, zero = torch.ones(1), torch.zeros(1)
    y, _ = B.bn_relu_maxpool(x, one, zero)
    assert tuple(y.shape) == (1, 1, 3, 2) and torch.isnan(y[0, 0, :2]).all() and torch.equal(y[0, 0, 2], torch.zeros(2, dtype=torch.float64))
    y, _ = B.bn_relu(torch.tensor([[[[float("nan"), -1.0, 2.0]]]]), one, zero)
    assert torch.isnan(y[0, 0, 0, 0]) and y[0, 0, 0, 1:].tolist() == [0.0, 2.0]


def test_group_norm_cannot_take_the_fused_route(monkeypatch):
    from os2d_amd.modeling.feature_extractor import resnet50_c4
    ex = resnet50_c4(use_group_norm=True)
    assert ex.inference_route == "torch"
    with pytest.raises(ValueError, match="GroupNorm"):
        ex.inference_route = "fused"
    assert ex.inference_route == "torch"
    with pytest.raises(ValueError, match="one of"):
        ex.inference_route = "miopen"
    monkeypatch.setenv("OS2D_BACKBONE_ROUTE", "fused")
    with pytest.raises(ValueError, match="GroupNorm"):
        resnet50_c4(use_group_norm=True)


def test_environment_sets_the_initial_route(monkeypatch):
    from os2d_amd.modeling.feature_extractor import resnet50_c4
    from os2d_amd.modeling.model import Os2dModel
    monkeypatch.delenv("OS2D_BACKBONE_ROUTE", raising=False)
    assert resnet50_c4().inference_route == "torch"
    monkeypatch.setenv("OS2D_BACKBONE_ROUTE", "fused")
    assert resnet50_c4().inference_route == "fused"
    net = Os2dModel(merge_branch_parameters=False)
    assert net.net_feature_maps.inference_route == net.net_label_features.net_class_features.inference_route == "fused"
    monkeypatch.setenv("OS2D_BACKBONE_ROUTE", "torch")
    assert resnet50_c4().inference_route == "torch"
    monkeypatch.setenv("OS2D_BACKBONE_ROUTE", "fast")
    with pytest.raises(ValueError, match="one of"):
        resnet50_c4()


def test_calls_that_stay_on_the_torch_route(extractor, monkeypatch):
    """With "fused" set: grad mode, a BatchNorm in training mode and a CPU tensor each take the module path, bit for bit."""
    from os2d_amd.modeling import backbone_fused
    x = torch.randn(1, 3, 64, 64, generator=torch.Generator().manual_seed(3))
    with torch.no_grad():
        want = extractor(x)
    assert extractor.inference_route == "torch"

    def never(self, x):
        raise AssertionError("the fused route was taken")
    monkeypatch.setattr(backbone_fused.FusedBackbone, "forward", never)
    extractor.inference_route = "fused"
    try:
        with torch.no_grad():
            assert not backbone_fused.eligible(extractor, x) and torch.equal(extractor(x), want)              # a CPU tensor
        assert torch.equal(extractor(x), want)                                                               # grad mode
        # what `eligible` looks at besides the device: answered for a tensor that claims to be on one
        assert backbone_fused.frozen(extractor)
        extractor.layer2[1].bn2.train()
        assert not backbone_fused.frozen(extractor)
        extractor.layer2[1].bn2.eval()
        extractor.train()
        extractor.freeze_bn()
        assert backbone_fused.frozen(extractor)
        with torch.enable_grad():
            assert not backbone_fused.eligible(extractor, x)
    finally:
        extractor.eval()
        extractor.inference_route = "torch"


def test_fold_cache_adds_nothing_to_the_module_and_follows_the_statistics():
    from os2d_amd.modeling.feature_extractor import resnet50_c4
    from os2d_amd.modeling.model import Os2dModel
    ex = resnet50_c4().eval()
    keys, params, modules = list(ex.state_dict()), [id(p) for p in ex.parameters()], [n for n, _ in ex.named_modules()]
    buffers = [n for n, _ in ex.named_buffers()]
    runner = ex.fused_backbone()
    assert runner is ex.fused_backbone() and not isinstance(runner, torch.nn.Module)
    cpu = torch.device("cpu")
    first = runner.folds(cpu)
    assert runner.folds(cpu) is first and runner.rebuilds == 1
    assert list(ex.state_dict()) == keys and [id(p) for p in ex.parameters()] == params and [n for n, _ in ex.named_modules()] == modules
    assert [n for n, _ in ex.named_buffers()] == buffers
    net = Os2dModel()
    reference_keys = list(net.state_dict())
    net.net_feature_maps.fused_backbone().folds(cpu)
    assert list(net.state_dict()) == reference_keys
    # written in place (_version), replaced (data_ptr), loaded: each one rebuilds, and the new fold is the new statistics'
    bn = ex.layer3[2].bn2
    bn.running_var.mul_(2)
    s, _ = runner.folds(cpu)[id(bn)]
    assert runner.rebuilds == 2 and torch.equal(s, B.fold32(bn)[0]) and not torch.equal(s, first[id(bn)][0])
    bn.bias.data = bn.bias.data + 1
    assert torch.equal(runner.folds(cpu)[id(bn)][1], B.fold32(bn)[1]) and runner.rebuilds == 3
    ex.load_state_dict(ex.state_dict())
    runner.folds(cpu)
    assert runner.rebuilds == 4 and runner.folds(cpu) is runner.folds(cpu) and runner.rebuilds == 4


def test_backbone_library_record_header_binding_and_exports_agree():
    from os2d_amd import build, _backbone_lib
    rec = build.BACKBONE
    assert rec not in build.LIBRARIES and rec not in build.ALL_LIBRARIES and _backbone_lib.LIBRARY.record is rec
    assert build.BUILT_LIBRARIES == build.ALL_LIBRARIES + [rec]
    assert (rec.name, rec.env, rec.header) == ("libos2d_backbone.so", "OS2D_BACKBONE_LIB", "os2d_backbone.h")
    assert build.build(verbose=False) == build.LIB_PATH                  # what a clean checkout runs builds it as well
    assert build.up_to_date(rec) and os.path.exists(build.BACKBONE_LIB_PATH + ".srchash") and build.lib_path(rec) == build.BACKBONE_LIB_PATH
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(REPO, "include", rec.header)).read(), flags=re.S)
    assert sorted(set(re.findall(r"\b(os2d_[a-z0-9_]+)\s*\(", text))) == sorted(_backbone_lib.SIGNATURES)
    assert re.search(r"^#define OS2D_BACKBONE_ABI_VERSION (\d+)$", text, flags=re.M).group(1) == str(_backbone_lib.ABI_VERSION) == "1"
    assert re.search(r"^#define OS2D_BACKBONE_MAX_GROUPS {}\b".format(_backbone_lib.MAX_GROUPS), text, flags=re.M)
    out = subprocess.check_output(["nm", "-D", "--defined-only", build.BACKBONE_LIB_PATH]).decode()
    assert set(re.findall(r" T (os2d_\w+)", out)) == set(_backbone_lib.SIGNATURES)
    assert "os2d_error_text" not in out and "os2d_set_error" not in out
    lib = _backbone_lib.load()
    assert lib.os2d_backbone_abi_version() == 1
    assert set(_backbone_lib.SIGNATURES) == {"os2d_backbone_abi_version", "os2d_backbone_last_error", "os2d_backbone_bn_relu", "os2d_backbone_bn_add_relu",
                                             "os2d_backbone_bn_relu_maxpool"}


def test_backbone_library_flags_includes_and_stamp(tmp_path):
    from os2d_amd import build
    rec = build.BACKBONE
    for s in rec.sources:           # no packed FP32: the kernels run next to other streams' MFMA waves
        assert build.unit_flags(rec, s) == build.FLAGS + build.PACKED_OFF and os.path.exists(os.path.join(rec.csrc, s))
    assert all(not set(rec.sources) & set(other.sources) and rec.csrc != other.csrc for other in build.ALL_LIBRARIES)
    assert [os.path.basename(d) for d in rec.header_dirs] == ["csrc_backbone", "csrc_shared"]
    names = {os.path.basename(h) for h in build.headers(rec)}
    assert {"backbone_common.h", "abi_common.h", "os2d_backbone.h"} <= names
    for path in [os.path.join(rec.csrc, s) for s in rec.sources] + build.headers(rec):
        for inc in build.local_includes(path):
            assert os.path.basename(inc) in names, (path, inc)
    h0 = build.source_hash(rec)
    assert build.source_hash(rec._replace(flags=rec.flags + ["-DX"])) != h0
    (tmp_path / "new_header.h").write_text("// new\n")
    assert build.source_hash(rec._replace(header_dirs=rec.header_dirs + [str(tmp_path)])) != h0


def test_missing_backbone_library_fails_loudly(monkeypatch, tmp_path):
    from os2d_amd import _backbone_lib
    from os2d_amd._native import Os2dLibraryError
    monkeypatch.setattr(_backbone_lib.LIBRARY, "_handle", None)
    monkeypatch.setenv("OS2D_BACKBONE_LIB", str(tmp_path / "nope.so"))
    with pytest.raises(Os2dLibraryError, match="no CPU or PyTorch fallback"):
        _backbone_lib.load()


# every class of bad argument: (entry point, arguments, text).  Sizes in the order of the header; `fake` pointers are far apart
# unless the case is about overlap.
def _at(offset):
    return ctypes.c_void_p(1 << 20 | offset)


X, S, T, R, Y = _at(0), ctypes.c_void_p(1 << 30), ctypes.c_void_p((1 << 30) + 4096), ctypes.c_void_p(1 << 24), ctypes.c_void_p(1 << 28)
REFUSALS = [
    ("bn_relu", (None, S, T, Y, 1, 4, 9), "null pointer"),
    ("bn_relu", (X, S, None, Y, 1, 4, 9), "null pointer"),
    ("bn_relu", (X, S, T, None, 1, 4, 9), "null pointer"),
    ("bn_relu", (_at(2), S, T, Y, 1, 4, 9), "not aligned"),
    ("bn_relu", (X, S, T, Y, 0, 4, 9), "bad shape"),
    ("bn_relu", (X, S, T, Y, 1, 0, 9), "bad shape"),
    ("bn_relu", (X, S, T, Y, 1, 4, -1), "bad shape"),
    ("bn_relu", (X, S, T, Y, 1 << 16, 1 << 15, 1), "too large"),                 # N * C = 2^31
    ("bn_relu", (X, S, T, Y, 1, 1, (1 << 30) + 1), "too large"),                 # HW
    ("bn_relu", (X, S, T, Y, 1 << 10, 1 << 10, 1 << 21), "too large"),           # N * C * HW = 2^41
    ("bn_relu", (X, S, T, _at(16), 1, 4, 9), "overlaps x"),                      # shifted by 4 elements: neither x nor apart
    ("bn_add_relu", (X, S, T, None, None, None, Y, 1, 4, 9), "null pointer"),
    ("bn_add_relu", (X, S, T, R, S, None, Y, 1, 4, 9), "both given or both NULL"),
    ("bn_add_relu", (X, S, T, R, None, T, Y, 1, 4, 9), "both given or both NULL"),
    ("bn_add_relu", (X, S, T, R, ctypes.c_void_p((1 << 30) + 1), T, Y, 1, 4, 9), "not aligned"),
    ("bn_add_relu", (X, S, T, R, None, None, Y, 1, 4, 0), "bad shape"),
    ("bn_add_relu", (X, S, T, R, None, None, Y, 1 << 16, 1 << 15, 1), "too large"),
    ("bn_add_relu", (X, S, T, R, None, None, R, 1, 4, 9), "overlaps r"),
    ("bn_add_relu", (X, S, T, X, None, None, X, 1, 4, 9), "overlaps r"),         # in place is fine for x, never for r
    ("bn_add_relu", (X, S, T, R, None, None, ctypes.c_void_p((1 << 24) + 4 * 35), 1, 4, 9), "overlaps r"),      # the last element of r
    ("bn_add_relu", (X, S, T, R, None, None, _at(4), 1, 4, 9), "overlaps x"),
    ("bn_relu_maxpool", (X, None, T, Y, 1, 4, 5, 5), "null pointer"),
    ("bn_relu_maxpool", (X, S, T, ctypes.c_void_p((1 << 28) + 3), 1, 4, 5, 5), "not aligned"),
    ("bn_relu_maxpool", (X, S, T, Y, 1, 4, 0, 5), "bad shape"),
    ("bn_relu_maxpool", (X, S, T, Y, 1, 4, 5, -2), "bad shape"),
    ("bn_relu_maxpool", (X, S, T, Y, 1, 1, 1 << 15, (1 << 15) + 1), "too large"),
    ("bn_relu_maxpool", (X, S, T, X, 1, 4, 5, 5), "overlaps x"),
    ("bn_relu_maxpool", (X, S, T, _at(4 * 99), 1, 4, 5, 5), "overlaps x"),        # y starts on the last element of x
]


@pytest.mark.parametrize("k", range(len(REFUSALS)))
def test_bad_arguments_are_refused_before_any_launch(k):
    """No device here and the pointers lead nowhere: a call that got as far as a launch would not return -1 with its own text."""
    from os2d_amd import _backbone_lib
    name, args, text = REFUSALS[k]
    lib = _backbone_lib.load()
    assert getattr(lib, "os2d_backbone_" + name)(*(list(args) + [None])) == -1
    message = lib.os2d_backbone_last_error().decode()
    assert message.startswith(name + ":") and text in message, message
    with pytest.raises(RuntimeError, match=re.escape(message)):
        _backbone_lib.check(-1, name)
