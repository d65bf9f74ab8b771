"""CPU: the float64 model of os2d_backbone_conv1x1 (tests/backbone_conv_model.py) against the torch modules, which calls take the
inference route "fused_conv1x1" and what it leaves alone, and libos2d_backbone_conv.so held to what every library of the project is
held to (tests/test_native_libs.py, tests/test_backbone_model.py): record, header, binding and exports agree, bad arguments are refused
before any launch."""
import copy
import ctypes
import os
import re
import subprocess

import pytest
import torch

import backbone_conv_model as C
import backbone_model as B

REPO = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))


@pytest.fixture(scope="module")
def extractor():
    from os2d_amd.modeling.feature_extractor import resnet50_c4
    torch.manual_seed(0)
    ex = resnet50_c4().eval()
    B.perturb_batchnorms(ex, seed=1)
    return ex


@pytest.mark.parametrize("stride,with_downsample", [(1, False), (1, True), (2, True)])
def test_model_is_a_bottleneck_in_float64(stride, with_downsample):
    """conv2d + BatchNorm2d (+ add) + relu of the torch module in float64 against the chain of the models with unrounded folds: only
    float64 rounding separates them (sums of at most 9 * 16 products: 1e-12 of the largest output is generous)."""
    from os2d_amd.modeling.feature_extractor import Bottleneck
    torch.manual_seed(3 + stride)
    inplanes, planes = (64, 16) if not with_downsample else (24, 16)
    down = None
    if with_downsample:
        down = torch.nn.Sequential(torch.nn.Conv2d(inplanes, 4 * planes, kernel_size=1, stride=stride, bias=False), torch.nn.BatchNorm2d(4 * planes))
    block = Bottleneck(inplanes, planes, stride, down).eval()
    B.perturb_batchnorms(block, seed=5)
    x = torch.randn(2, inplanes, 7, 9, generator=torch.Generator().manual_seed(6))
    with torch.no_grad():
        want = copy.deepcopy(block).double()(x.double())
    got = C.bottleneck64(block, x, fold=B.fold_exact)
    assert tuple(got.shape) == tuple(want.shape) == (2, 64, (7 - 1) // stride + 1, (9 - 1) // stride + 1)
    assert float(want.abs().max()) > 1 and float((got - want).abs().max()) <= 1e-12 * float(want.abs().max())
    assert bool((want == 0).any()) and bool((want > 0).any())          # the ReLU is in it


def test_model_pieces_and_special_values():
    g = torch.Generator().manual_seed(7)
    x, w = torch.randn(2, 5, 4, 5, generator=g), torch.randn(3, 5, generator=g)
    s, t, sr, tr = torch.randn(3, generator=g), torch.randn(3, generator=g), torch.randn(3, generator=g), torch.randn(3, generator=g)
    r = torch.randn(2, 3, 2, 3, generator=g)
    y, S, v, d = C.conv1x1(x, w, s, t, r, sr, tr, stride=2, relu=False)
    n, co, i, j = 1, 2, 1, 2
    col = x[n, :, 2 * i, 2 * j].double()
    acc = float((w[co].double() * col).sum())
    assert abs(float(v[n, co, i, j]) - (acc * float(s[co]) + float(t[co]))) < 1e-12
    assert abs(float(S[n, co, i, j]) - float((w[co].double() * col).abs().sum())) < 1e-12
    assert abs(float(d[n, co, i, j]) - (float(r[n, co, i, j]) * float(sr[co]) + float(tr[co]))) < 1e-12
    assert float(y[n, co, i, j]) == float(v[n, co, i, j] + d[n, co, i, j])
    assert torch.equal(C.conv1x1(x, w, s, t, r, stride=2, relu=False)[3], r.double())
    assert torch.equal(C.conv1x1(x, w, s, t, r, sr, tr, stride=2, relu=True)[0], B.relu_nan(y))
    # a NaN and an Inf * 0 poison their own column, every output channel of it, and nothing else
    x[0, 1, 3, 4] = float("nan")
    x[1, 2, 0, 0] = float("inf")
    w[1, 2] = 0.0
    y = C.conv1x1(x, w, s, t)[0]
    assert torch.isnan(y[0, :, 3, 4]).all() and torch.isnan(y[1, 1, 0, 0]) and int(torch.isnan(y).sum()) == 3 + 1


def test_chained_models_reproduce_the_float64_module(extractor):
    """As tests/test_backbone_model.py's check of the "fused" chain, with its bound: 1e-9 of the largest output."""
    x = torch.randn(2, 3, 64, 96, generator=torch.Generator().manual_seed(2))
    want = B.module_forward64(extractor, x)
    got = C.extractor_forward64(extractor, x, fold=B.fold_exact)
    assert tuple(got.shape) == tuple(want.shape) == (2, 1024, 4, 6)
    err, top = float((got - want).abs().max()), float(want.abs().max())
    print("float64 chain against float64 module: {:.3g} at max |y| {:.4g}".format(err, top))
    assert top > 1.0 and err <= 1e-9 * top
    rounded = C.extractor_forward64(extractor, x)
    assert 0 < float((rounded - want).abs().max()) <= 1e-4 * top


def test_resnet_layer_table():
    layers = C.resnet_c4_layers()
    assert len(layers) == 12 and len({c[1:] for c in layers}) == 11
    assert {c[1:] for c in layers if c[3] == 2} == {(256, 512, 2), (512, 1024, 2)}             # the stride-2 gathers: two layers per network
    assert {c[2] for c in layers} == {64, 128, 256, 512, 1024} and {c[1] for c in layers} == {64, 128, 256, 512, 1024}


def test_environment_and_setter_take_the_new_route(monkeypatch):
    from os2d_amd.modeling import backbone_fused
    from os2d_amd.modeling.feature_extractor import resnet50_c4
    from os2d_amd.modeling.model import Os2dModel
    assert backbone_fused.ROUTES == ("torch", "fused", "fused_conv1x1")
    monkeypatch.delenv("OS2D_BACKBONE_ROUTE", raising=False)
    assert resnet50_c4().inference_route == "torch"                     # the default is what it was
    monkeypatch.setenv("OS2D_BACKBONE_ROUTE", "fused_conv1x1")
    assert resnet50_c4().inference_route == "fused_conv1x1"
    net = Os2dModel(merge_branch_parameters=False)
    assert net.net_feature_maps.inference_route == net.net_label_features.net_class_features.inference_route == "fused_conv1x1"
    with pytest.raises(ValueError, match="GroupNorm"):
        resnet50_c4(use_group_norm=True)
    monkeypatch.delenv("OS2D_BACKBONE_ROUTE")
    ex = resnet50_c4(use_group_norm=True)
    with pytest.raises(ValueError, match="GroupNorm"):
        ex.inference_route = "fused_conv1x1"
    assert ex.inference_route == "torch"


def test_a_convolution_that_is_not_plain_is_refused():
    from os2d_amd.modeling import backbone_fused
    from os2d_amd.modeling.feature_extractor import resnet50_c4
    ex = resnet50_c4().eval()
    assert len(backbone_fused.pointwise_convs(ex)) == 2 * 13 + 3 and all(backbone_fused.plain_conv1x1(c) for c in backbone_fused.pointwise_convs(ex))
    block = ex.layer2[1]
    plain = block.conv3
    others = [torch.nn.Conv2d(128, 512, 1, bias=True), torch.nn.Conv2d(128, 512, 1, groups=2, bias=False), torch.nn.Conv2d(128, 512, 1, padding=1, bias=False),
              torch.nn.Conv2d(128, 512, 1, stride=3, bias=False), torch.nn.Conv2d(128, 512, 1, stride=(1, 2), bias=False),
              torch.nn.Conv2d(128, 512, 1, bias=False).double(), torch.nn.Conv2d(128, 512, 3, padding=1, bias=False)]
    others.append(torch.nn.Conv2d(128, 512, 1, bias=False))
    others[-1].weight.data = torch.randn(128, 512, 1, 1).permute(1, 0, 2, 3)          # not contiguous
    try:
        for conv in others:
            assert not backbone_fused.plain_conv1x1(conv)
            block.conv3 = conv
            with pytest.raises(ValueError, match="plain 1x1 convolutions"):
                ex.inference_route = "fused_conv1x1"
            assert ex.inference_route == "torch"
            ex.inference_route = "fused"                                 # the other routes do not mind
            ex.inference_route = "torch"
    finally:
        block.conv3 = plain
    ex.inference_route = "fused_conv1x1"


def test_calls_that_stay_on_the_torch_route(extractor, monkeypatch):
    """With "fused_conv1x1" set: a CPU tensor, grad mode and a BatchNorm in training mode each take the module path, bit for bit."""
    from os2d_amd.modeling import backbone_fused
    x = torch.randn(1, 3, 64, 64, generator=torch.Generator().manual_seed(3))
    with torch.no_grad():
        want = extractor(x)
    assert extractor.inference_route == "torch"

    def never(self, x):
        raise AssertionError("a fused route was taken")
    monkeypatch.setattr(backbone_fused.FusedBackbone, "forward", never)
    monkeypatch.setattr(backbone_fused.FusedBackbone, "forward_conv1x1", never)
    extractor.inference_route = "fused_conv1x1"
    try:
        with torch.no_grad():
            assert not backbone_fused.eligible(extractor, x) and torch.equal(extractor(x), want)              # a CPU tensor
        assert torch.equal(extractor(x), want)                                                               # grad mode
        extractor.layer2[1].bn2.train()
        assert not backbone_fused.frozen(extractor)
        with torch.no_grad():
            assert not backbone_fused.eligible(extractor, x)
        extractor.layer2[1].bn2.eval()
        assert backbone_fused.frozen(extractor)
    finally:
        extractor.eval()
        extractor.inference_route = "torch"


def test_route_adds_nothing_to_the_module_tree():
    from os2d_amd.modeling.feature_extractor import resnet50_c4
    ex = resnet50_c4().eval()
    keys, params, modules = list(ex.state_dict()), [id(p) for p in ex.parameters()], [n for n, _ in ex.named_modules()]
    buffers = [n for n, _ in ex.named_buffers()]
    ex.inference_route = "fused_conv1x1"
    runner = ex.fused_backbone()
    runner.folds(torch.device("cpu"))
    ex.inference_route = "fused"
    assert ex.fused_backbone() is runner and runner.rebuilds == 1       # one runner, one fold cache for both routes
    assert list(ex.state_dict()) == keys and [id(p) for p in ex.parameters()] == params and [n for n, _ in ex.named_modules()] == modules
    assert [n for n, _ in ex.named_buffers()] == buffers


def test_library_record_header_binding_and_exports_agree():
    from os2d_amd import build, _backbone_conv_lib as L
    rec = build.BACKBONE_CONV
    assert rec not in build.LIBRARIES and rec not in build.ALL_LIBRARIES and rec not in build.BUILT_LIBRARIES and L.LIBRARY.record is rec
    assert build.EVERY_LIBRARY == build.BUILT_LIBRARIES + [rec]
    assert (rec.name, rec.env, rec.header) == ("libos2d_backbone_conv.so", "OS2D_BACKBONE_CONV_LIB", "os2d_backbone_conv.h")
    assert build.build(verbose=False) == build.LIB_PATH                  # what a clean checkout runs builds it as well
    assert build.up_to_date(rec) and os.path.exists(build.BACKBONE_CONV_LIB_PATH + ".srchash") and build.lib_path(rec) == build.BACKBONE_CONV_LIB_PATH
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(REPO, "include", rec.header)).read(), flags=re.S)
    assert sorted(set(re.findall(r"\b(os2d_[a-z0-9_]+)\s*\(", text))) == sorted(L.SIGNATURES)
    assert re.search(r"^#define OS2D_BACKBONE_CONV_ABI_VERSION (\d+)$", text, flags=re.M).group(1) == str(L.ABI_VERSION) == "1"
    # the tile sizes and the cap on work-groups of header and binding agree
    for name, value in (("TILE_M", L.TILE_M), ("TILE_N", L.TILE_N), ("TILE_K", L.TILE_K), ("SMALL_TILE_M", L.SMALL_TILE_M), ("SMALL_TILE_N", L.SMALL_TILE_N),
                        ("MAX_GROUPS", L.MAX_GROUPS)):
        assert re.search(r"^#define OS2D_BACKBONE_CONV_{} {}\b".format(name, value), text, flags=re.M), name
    assert L.TILE_M % 32 == 0 and L.TILE_N % 32 == 0 and L.TILE_K % 2 == 0 and L.SMALL_TILE_M < L.TILE_M
    out = subprocess.check_output(["nm", "-D", "--defined-only", build.BACKBONE_CONV_LIB_PATH]).decode()
    assert set(re.findall(r" T (os2d_\w+)", out)) == set(L.SIGNATURES)
    assert "os2d_error_text" not in out and "os2d_set_error" not in out
    assert L.load().os2d_backbone_conv_abi_version() == 1
    assert set(L.SIGNATURES) == {"os2d_backbone_conv_abi_version", "os2d_backbone_conv_last_error", "os2d_backbone_conv1x1"}
    # the entry point is declared with 8 pointers, 7 sizes and the stream
    assert len(L.SIGNATURES["os2d_backbone_conv1x1"][1]) == 16


def shared_conv_header(rec, source):
    """-> the text of csrc_backbone/conv1x1_common.h, after checking that the unit `source` of the record takes the epilogue and the
    argument contract from it: the unit includes it and defines neither of them, the header is among the record's headers and holds them."""
    from os2d_amd import build
    path = os.path.join(build.BACKBONE_CSRC, "conv1x1_common.h")
    assert "conv1x1_common.h" in [os.path.basename(inc) for inc in build.local_includes(os.path.join(rec.csrc, rec.sources[0]))]
    assert all(path in build.headers(lib) for lib in (rec, build.BACKBONE, build.BACKBONE_CONV, build.BACKBONE_CONV_BF16))
    assert [os.path.basename(inc) for inc in build.local_includes(path)] == ["backbone_common.h"]          # and no library's public header
    common = open(path).read()
    for name in ("conv_out", "conv_epilogue", "too_large"):
        assert not re.search(r"\b\w*{}\s*[<(]".format(name), source), name
        assert len(re.findall(r"^[\w \t]*\b\w*{}\(.*\) {{$".format(name), common, flags=re.M)) == 1, name
    return common


def test_library_flags_includes_and_stamp(tmp_path):
    from os2d_amd import build
    rec = build.BACKBONE_CONV
    for s in rec.sources:           # no packed FP32: the kernel runs next to other streams' MFMA waves
        assert build.unit_flags(rec, s) == build.FLAGS + build.PACKED_OFF and os.path.exists(os.path.join(rec.csrc, s))
    assert all(not set(rec.sources) & set(other.sources) and rec.csrc != other.csrc for other in build.BUILT_LIBRARIES)
    assert [os.path.basename(d) for d in rec.header_dirs] == ["csrc_backbone_conv", "csrc_backbone", "csrc_shared"]
    names = {os.path.basename(h) for h in build.headers(rec)}
    assert {"backbone_common.h", "abi_common.h", "os2d_backbone_conv.h"} <= names
    # every quoted include resolves in the record's headers; backbone_common.h, which is reused and not copied, also pulls in the public
    # header of ITS library, of which this unit uses nothing
    names.add(build.BACKBONE.header)
    for path in [os.path.join(rec.csrc, s) for s in rec.sources] + build.headers(rec):
        for inc in build.local_includes(path):
            assert os.path.basename(inc) in names, (path, inc)
    source = open(os.path.join(rec.csrc, "conv1x1.hip")).read()
    # the fold, the ReLU and the overlap predicate are those of conv1x1_common.h, which the unit includes and does not restate
    common = shared_conv_header(rec, source)
    assert "bb_bn(" in common and "bb_relu_nan(" in common and "bb_overlap(" in common and "__builtin_amdgcn_mfma_f32_32x32x2f32" in source
    assert not re.search(r"\basm\b", source) and not re.search(r"\basm\b", common)              # no inline assembly
    h0 = build.source_hash(rec)
    assert build.source_hash(rec._replace(flags=rec.flags + ["-DX"])) != h0
    (tmp_path / "new_header.h").write_text("// new\n")
    assert build.source_hash(rec._replace(header_dirs=rec.header_dirs + [str(tmp_path)])) != h0


def test_missing_library_fails_loudly(monkeypatch, tmp_path):
    from os2d_amd import _backbone_conv_lib as L
    from os2d_amd._native import Os2dLibraryError
    monkeypatch.setattr(L.LIBRARY, "_handle", None)
    monkeypatch.setenv("OS2D_BACKBONE_CONV_LIB", str(tmp_path / "nope.so"))
    with pytest.raises(Os2dLibraryError, match="no CPU or PyTorch fallback"):
        L.load()


# every class of bad argument: (arguments in the order of the header, text).  The fake pointers are far apart unless the case is about
# overlap; none is ever dereferenced.
def _p(v):
    return ctypes.c_void_p(v)


X, WT, S, T, R, Y = _p(1 << 20), _p(1 << 22), _p(1 << 30), _p((1 << 30) + 4096), _p(1 << 24), _p(1 << 28)
SIZES = (1, 4, 8, 3, 3, 1, 1)               # N, Cin, Cout, H, W, stride, relu: x has 36 floats, w 32, y 72
REFUSALS = [
    ((None, WT, S, T, None, None, None, Y) + SIZES, "null pointer"),
    ((X, None, S, T, None, None, None, Y) + SIZES, "null pointer"),
    ((X, WT, None, T, None, None, None, Y) + SIZES, "null pointer"),
    ((X, WT, S, None, None, None, None, Y) + SIZES, "null pointer"),
    ((X, WT, S, T, None, None, None, None) + SIZES, "null pointer"),
    ((X, WT, S, T, R, S, None, Y) + SIZES, "both given or both NULL"),
    ((X, WT, S, T, R, None, T, Y) + SIZES, "both given or both NULL"),
    ((X, WT, S, T, None, S, T, Y) + SIZES, "only together with r"),
    ((_p((1 << 20) + 2), WT, S, T, None, None, None, Y) + SIZES, "not aligned"),
    ((X, _p((1 << 22) + 1), S, T, None, None, None, Y) + SIZES, "not aligned"),
    ((X, WT, S, T, _p((1 << 24) + 3), None, None, Y) + SIZES, "not aligned"),
    ((X, WT, S, T, None, None, None, _p((1 << 28) + 2)) + SIZES, "not aligned"),
    ((X, WT, S, T, None, None, None, Y, 0, 4, 8, 3, 3, 1, 1), "bad shape"),
    ((X, WT, S, T, None, None, None, Y, 1, 0, 8, 3, 3, 1, 1), "bad shape"),
    ((X, WT, S, T, None, None, None, Y, 1, 4, -8, 3, 3, 1, 1), "bad shape"),
    ((X, WT, S, T, None, None, None, Y, 1, 4, 8, 0, 3, 1, 1), "bad shape"),
    ((X, WT, S, T, None, None, None, Y, 1, 4, 8, 3, -1, 1, 1), "bad shape"),
    ((X, WT, S, T, None, None, None, Y, 1, 4, 8, 3, 3, 0, 1), "stride is 1 or 2"),
    ((X, WT, S, T, None, None, None, Y, 1, 4, 8, 3, 3, 3, 1), "stride is 1 or 2"),
    ((X, WT, S, T, None, None, None, Y, 1, 4, 8, 3, 3, 1, 2), "relu is 0 or 1"),
    ((X, WT, S, T, None, None, None, Y, 1, 4, 8, 3, 3, 1, -1), "relu is 0 or 1"),
    ((X, WT, S, T, None, None, None, Y, 1, (1 << 20) + 1, 8, 1, 1, 1, 1), "too large"),              # Cin
    ((X, WT, S, T, None, None, None, Y, 1, 4, (1 << 20) + 1, 1, 1, 1, 1), "too large"),              # Cout
    ((X, WT, S, T, None, None, None, Y, 1 << 12, 1 << 19, 1, 1, 1, 1, 1), "too large"),              # N * Cin = 2^31
    ((X, WT, S, T, None, None, None, Y, 1 << 12, 1, 1 << 19, 1, 1, 1, 1), "too large"),              # N * Cout = 2^31: y alone
    ((X, WT, S, T, None, None, None, Y, 1, 1, 1, 1 << 15, (1 << 15) + 1, 1, 1), "too large"),        # H * W of x
    ((X, WT, S, T, None, None, None, Y, 1 << 10, 1 << 10, 1, 1 << 11, 1 << 10, 2, 1), "too large"),  # N * Cin * H * W = 2^41, y is small
    ((X, WT, S, T, None, None, None, Y, 1 << 10, 1, 1 << 10, 1 << 11, 1 << 10, 1, 1), "too large"),  # N * Cout * Ho * Wo = 2^41, x is small
    ((X, WT, S, T, None, None, None, X) + SIZES, "overlaps x"),
    ((X, WT, S, T, None, None, None, _p((1 << 20) + 4 * 35)) + SIZES, "overlaps x"),                 # y starts on the last element of x
    ((X, WT, S, T, None, None, None, _p((1 << 20) - 4 * 71)) + SIZES, "overlaps x"),                 # y ends on the first
    ((X, WT, S, T, None, None, None, _p((1 << 22) + 4 * 31)) + SIZES, "overlaps w"),
    ((X, WT, S, T, R, None, None, R) + SIZES, "overlaps r"),
    ((X, WT, S, T, R, S, T, _p((1 << 24) + 4 * 71)) + SIZES, "overlaps r"),
]


@pytest.mark.parametrize("k", range(len(REFUSALS)))
def test_bad_arguments_are_refused_before_any_launch(k):
    """No device here and the pointers lead nowhere: a call that got as far as a launch would not return -1 with its own text."""
    from os2d_amd import _backbone_conv_lib as L
    args, text = REFUSALS[k]
    assert len(args) == 15
    lib = L.load()
    assert lib.os2d_backbone_conv1x1(*(list(args) + [None])) == -1
    message = lib.os2d_backbone_conv_last_error().decode()
    assert message.startswith("conv1x1:") and text in message, message
    with pytest.raises(RuntimeError, match=re.escape(message)):
        L.check(-1, "conv1x1")
