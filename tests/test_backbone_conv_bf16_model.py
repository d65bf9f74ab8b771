"""CPU: the split of an fp32 value into three bf16 values - os2d_amd/csrc_backbone_conv_bf16/bf16x3_split.h compiled into a host program
against the numpy model (tests/backbone_conv_bf16_model.py), bit for bit, and the properties the arithmetic rests on; the setting
``conv1x1_precision`` and what it leaves alone; and libos2d_backbone_conv_bf16.so held to what every library of the project is held to:
record, header, binding and exports agree, bad arguments of its three entry points are refused before any launch."""
import ctypes
import os
import re
import shutil
import subprocess

import numpy as np
import pytest
import torch

import backbone_conv_bf16_model as M
import backbone_model as B
import test_backbone_conv_model as F

REPO = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
FLT_MAX_BITS, BF16_MAX_BITS = 0x7F7FFFFF, 0x7F7F0000


def values():
    """Bit patterns: random values over 80 binades, powers of two and their neighbours, subnormals, +-0, +-Inf, NaNs, and what lies between
    bf16's largest finite number and FLT_MAX."""
    rng = np.random.default_rng(0)
    rand = (rng.standard_normal(20000) * np.exp2(rng.integers(-40, 40, 20000))).astype(np.float32).view(np.uint32)
    pows = np.array([np.float32(2.0) ** e for e in range(-126, 128)], dtype=np.float32).view(np.uint32)
    pows = np.concatenate([pows, pows + 1, pows - 1, pows | 0x80000000, pows + 0x8000, pows + 0x7FFF, pows + 0x8001, pows + 0x18000])
    subnormal = np.concatenate([np.arange(1, 64, dtype=np.uint32), rng.integers(1, 0x00800000, 2000).astype(np.uint32),
                                np.array([0x007FFFFF, 0x00010000, 0x00008000, 0x00018000, 0x00007FFF], dtype=np.uint32)])
    top = np.concatenate([np.arange(BF16_MAX_BITS - 4, BF16_MAX_BITS + 5, dtype=np.uint32), np.arange(M.TOP - 4, M.TOP + 5, dtype=np.uint32),
                          np.arange(FLT_MAX_BITS - 8, FLT_MAX_BITS + 1, dtype=np.uint32),
                          rng.integers(BF16_MAX_BITS, FLT_MAX_BITS + 1, 500).astype(np.uint32)])
    special = np.array([0, 0x80000000, 0x7F800000, 0xFF800000, 0x7FC00000, 0xFFC00000, 0x7F800001, 0x7FFFFFFF, 0xFFA00000], dtype=np.uint32)
    u = np.concatenate([rand, pows, subnormal, subnormal | 0x80000000, top, top | 0x80000000, special]).astype(np.uint32)
    return u


@pytest.fixture(scope="module")
def host_split(tmp_path_factory):
    """(bit patterns, parts [n, 3], special [n], parts of an activation [n, 3]) of the header compiled as a plain C++ host program"""
    cxx = shutil.which("g++") or shutil.which("clang++") or "/opt/rocm/lib/llvm/bin/clang++"
    if not os.path.exists(cxx) and shutil.which(cxx) is None:
        pytest.skip("no C++ compiler")
    exe = str(tmp_path_factory.mktemp("bf16x3") / "bf16x3_split_check")
    subprocess.run([cxx, "-std=c++17", "-O2", "-Wall", "-Werror", "-I", os.path.join(REPO, "os2d_amd", "csrc_backbone_conv_bf16"),
                    os.path.join(REPO, "tests", "host", "bf16x3_split_check.cpp"), "-o", exe], check=True, timeout=120)
    u = values()
    out = subprocess.run([exe], input="\n".join("{:08x}".format(v) for v in u).encode(), capture_output=True, timeout=60, check=True).stdout.decode().split()
    got = np.array([int(t, 16) for t in out]).reshape(len(u), 7)
    return u, got[:, :3].astype(np.uint16), got[:, 3].astype(bool), got[:, 4:].astype(np.uint16)


def test_header_equals_the_model_bit_for_bit(host_split):
    u, parts, special, parts_x = host_split
    want = np.stack(M.split(u.view(np.float32)), axis=1)
    bad = np.nonzero((parts != want).any(axis=1))[0]
    assert len(bad) == 0, [(hex(u[i]), parts[i].tolist(), want[i].tolist()) for i in bad[:10]]
    assert np.array_equal(special, (u & 0x7FFFFFFF) >= M.TOP)
    # the activation's split: the same for a finite value, a non-finite one in the last part alone
    assert np.array_equal(parts_x, np.stack(M.split_x(u.view(np.float32)), axis=1))
    finite = np.isfinite(u.view(np.float32))
    assert np.array_equal(parts_x[finite], parts[finite]) and not parts_x[~finite, :2].any() and np.array_equal(parts_x[~finite, 2], parts[~finite, 0])


def test_model_rounds_as_torch_does():
    """The leading part of the model is torch's round-to-nearest-even conversion wherever that is finite; every NaN becomes the one quiet
    NaN 0x7FC0 (torch keeps a payload)."""
    u = values()
    x = torch.from_numpy(u.view(np.float32).copy())
    b0 = M.split(x.numpy())[0]
    t = x.to(torch.bfloat16).view(torch.int16).numpy().view(np.uint16)
    finite_result = ((t & 0x7FFF) != 0x7F80) & ~np.isnan(x.numpy())
    assert np.array_equal(b0[finite_result], t[finite_result]) and int(finite_result.sum()) > 20000
    assert bool(np.isnan(M.widen(b0[np.isnan(x.numpy())])).all()) and set(b0[np.isnan(x.numpy())].tolist()) == {0x7FC0}


def test_split_is_exact_and_finite(host_split):
    u, parts, _, _ = host_split
    x = u.view(np.float32)
    finite = np.isfinite(x)
    p = [M.widen(parts[:, i]).astype(np.float64) for i in range(3)]
    assert np.isfinite(p[0][finite]).all() and np.isfinite(p[1][finite]).all() and np.isfinite(p[2][finite]).all()      # no Inf from a finite value
    total = p[0] + p[1] + p[2]                                            # exact in float64: three values of 8 bits within 2^-24 of each other
    # bf16's smallest subnormal is 2^-133: a value whose last bit lies below it cannot be three bf16 values, whatever the rule.  Every
    # fp32 value of magnitude >= 2^-109 has its last bit at or above 2^-133.
    representable = finite & (np.abs(x) >= 2.0 ** -109)
    assert int(representable.sum()) > 20000 and np.array_equal(total[representable], x[representable].astype(np.float64))
    tiny = finite & ~representable
    assert (np.abs(total[tiny] - x[tiny].astype(np.float64)) <= 2.0 ** -134).all()                # half of that subnormal, once
    # the values between bf16's largest finite number and FLT_MAX are in it, and FLT_MAX itself splits into three finite parts
    i = int(np.nonzero(u == FLT_MAX_BITS)[0][0])
    assert parts[i].tolist() == [0x7F7F, 0x7B80, 0xF380] and representable[i]
    # magnitudes: |b1| <= 2^-8 |x|, |b2| <= 2^-16 |x|
    # (where the leading part is truncated, above bf16's largest finite number, one bit more is left over)
    top = (u & 0x7FFFFFFF) >= M.TOP
    for sel, shift in ((finite & ~top & (np.abs(x) >= 2.0 ** -100), 0), (finite & top, 1)):
        ax = np.abs(x[sel]).astype(np.float64)
        assert len(ax) > 500 and (np.abs(p[1][sel]) <= 2.0 ** (shift - 8) * ax).all() and (np.abs(p[2][sel]) <= 2.0 ** (shift - 16) * ax).all()
    # a non-finite value keeps its kind in the leading part and has no others
    nonfinite = ~finite
    assert (parts[nonfinite, 1] == 0).all() and (parts[nonfinite, 2] == 0).all()
    assert np.array_equal(np.isnan(M.widen(parts[nonfinite, 0])), np.isnan(x[nonfinite]))
    assert np.array_equal(M.widen(parts[np.isinf(x), 0]), x[np.isinf(x)])
    assert parts[u == 0].tolist() == [[0, 0, 0]] and parts[u == 0x80000000][0, 0] == 0x8000


def test_six_products_reproduce_the_product():
    """The arithmetic the kernel rests on: every bf16 x bf16 product is exact in fp32, and the six products kept differ from w * x by at
    most (2^-23 + 2^-32) |w x|."""
    rng = np.random.default_rng(1)
    x = (rng.standard_normal(100000) * np.exp2(rng.integers(-20, 20, 100000))).astype(np.float32)
    w = (rng.standard_normal(100000) * np.exp2(rng.integers(-20, 20, 100000))).astype(np.float32)
    xp, wp = [M.widen(b) for b in M.split(x)], [M.widen(b) for b in M.split(w)]
    six = np.zeros(len(x))
    for i, j in ((2, 0), (1, 1), (0, 2), (1, 0), (0, 1), (0, 0)):
        prod32 = xp[i] * wp[j]
        assert np.array_equal(prod32.astype(np.float64), xp[i].astype(np.float64) * wp[j].astype(np.float64))          # exact in fp32
        six += prod32
    exact = x.astype(np.float64) * w.astype(np.float64)
    assert (np.abs(six - exact) <= (2.0 ** -23 + 2.0 ** -32) * np.abs(exact)).all()
    three = sum(xp[i].astype(np.float64) * wp[j] for i, j in ((0, 0), (0, 1), (1, 0)))
    assert (np.abs(three - exact) / np.abs(exact)).max() > 2.0 ** -17          # three products would not do


def test_pack_layout_of_the_model():
    from os2d_amd import _backbone_conv_bf16_lib as L
    w = torch.randn(5, 35, generator=torch.Generator().manual_seed(0)).numpy()
    wp = M.pack(w, L.TILE_K)
    assert wp.shape == (3, 8, 5, 8) and wp.size == L.packed_elems(5, 35) == 3 * 64 * 5
    parts = M.split(w)
    for p, co, k in ((0, 0, 0), (1, 4, 34), (2, 2, 17), (0, 3, 8)):
        assert wp.reshape(-1)[((p * 8 + k // 8) * 5 + co) * 8 + k % 8] == parts[p][co, k]
    assert not wp[:, 4, :, 3:].any() and not wp[:, 5:].any()              # k >= 35 is zeros


def test_library_record_header_binding_and_exports_agree():
    from os2d_amd import build, _backbone_conv_bf16_lib as L
    rec = build.BACKBONE_CONV_BF16
    assert all(rec not in group for group in (build.LIBRARIES, build.ALL_LIBRARIES, build.BUILT_LIBRARIES, build.EVERY_LIBRARY)) and L.LIBRARY.record is rec
    assert build.EVERYTHING == build.EVERY_LIBRARY + [rec]
    assert (rec.name, rec.env, rec.header) == ("libos2d_backbone_conv_bf16.so", "OS2D_BACKBONE_CONV_BF16_LIB", "os2d_backbone_conv_bf16.h")
    assert build.build(verbose=False) == build.LIB_PATH                  # what a clean checkout runs builds it as well
    assert build.up_to_date(rec) and os.path.exists(build.BACKBONE_CONV_BF16_LIB_PATH + ".srchash") and build.lib_path(rec) == build.BACKBONE_CONV_BF16_LIB_PATH
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(REPO, "include", rec.header)).read(), flags=re.S)
    assert sorted(set(re.findall(r"\b(os2d_[a-z0-9_]+)\s*\(", text))) == sorted(L.SIGNATURES)
    assert re.search(r"^#define OS2D_BACKBONE_CONV_BF16_ABI_VERSION (\d+)$", text, flags=re.M).group(1) == str(L.ABI_VERSION) == "1"
    for name, value in (("TILE_M", L.TILE_M), ("TILE_N", L.TILE_N), ("TILE_K", L.TILE_K), ("SMALL_TILE_M", L.SMALL_TILE_M), ("SMALL_TILE_N", L.SMALL_TILE_N),
                        ("MAX_GROUPS", L.MAX_GROUPS)):
        assert re.search(r"^#define OS2D_BACKBONE_CONV_BF16_{} {}\b".format(name, value), text, flags=re.M), name
    assert L.TILE_M % 32 == 0 and L.TILE_N % 32 == 0 and L.TILE_K % 16 == 0 and L.SMALL_TILE_M < L.TILE_M
    out = subprocess.check_output(["nm", "-D", "--defined-only", build.BACKBONE_CONV_BF16_LIB_PATH]).decode()
    assert set(re.findall(r" T (os2d_\w+)", out)) == set(L.SIGNATURES)
    assert "os2d_error_text" not in out and "os2d_set_error" not in out
    lib = L.load()
    assert lib.os2d_backbone_conv_bf16_abi_version() == 1
    assert set(L.SIGNATURES) == {"os2d_backbone_conv_bf16_abi_version", "os2d_backbone_conv_bf16_last_error", "os2d_backbone_conv_bf16_packed_elems",
                                 "os2d_backbone_conv_bf16_pack_weights", "os2d_backbone_conv1x1_bf16x3"}
    # the GEMM takes the arguments of the fp32 entry point, the packed weights in place of w
    from os2d_amd import _backbone_conv_lib
    assert L.SIGNATURES["os2d_backbone_conv1x1_bf16x3"] == _backbone_conv_lib.SIGNATURES["os2d_backbone_conv1x1"]
    # the size is 3 planes of Cout x Kp, Kp = Cin rounded up to the k-step; nothing for a size outside 1 ... 2^20
    for cout, cin in ((1, 1), (5, 35), (64, 32), (1024, 256), (7, 33), (1 << 20, 1 << 20)):
        assert lib.os2d_backbone_conv_bf16_packed_elems(cout, cin) == 3 * cout * M.padded_k(cin, L.TILE_K) == L.packed_elems(cout, cin)
    for cout, cin in ((0, 4), (4, 0), (-1, 4), (4, -3), ((1 << 20) + 1, 4), (4, (1 << 20) + 1)):
        assert lib.os2d_backbone_conv_bf16_packed_elems(cout, cin) == 0
        with pytest.raises(ValueError, match="no packed weights"):
            L.packed_elems(cout, cin)


def test_library_flags_includes_and_stamp(tmp_path):
    from os2d_amd import build
    rec = build.BACKBONE_CONV_BF16
    for s in rec.sources:           # no packed FP32: the kernel runs next to other streams' MFMA waves
        assert build.unit_flags(rec, s) == build.FLAGS + build.PACKED_OFF and os.path.exists(os.path.join(rec.csrc, s))
    assert all(not set(rec.sources) & set(other.sources) and rec.csrc != other.csrc for other in build.EVERY_LIBRARY)
    assert [os.path.basename(d) for d in rec.header_dirs] == ["csrc_backbone_conv_bf16", "csrc_backbone", "csrc_shared"]
    names = {os.path.basename(h) for h in build.headers(rec)}
    assert {"bf16x3_split.h", "backbone_common.h", "abi_common.h", "os2d_backbone_conv_bf16.h"} <= names
    names.add(build.BACKBONE.header)                                     # backbone_common.h pulls in the public header of ITS library
    for path in [os.path.join(rec.csrc, s) for s in rec.sources] + build.headers(rec):
        for inc in build.local_includes(path):
            assert os.path.basename(inc) in names, (path, inc)
    source = open(os.path.join(rec.csrc, "conv1x1_bf16x3.hip")).read()
    common = F.shared_conv_header(rec, source)                           # the fp32 GEMM's epilogue and contract: the same text, not a copy
    assert "bb_bn(" in common and "bb_relu_nan(" in common and "bb_overlap(" in common and "__builtin_amdgcn_mfma_f32_32x32x16_bf16" in source
    assert "bf16x3_split(" in source and not re.search(r"\basm\b", source + common) and not re.search(r"atomic\w*\s*\(", source + common)
    h0 = build.source_hash(rec)
    assert build.source_hash(rec._replace(flags=rec.flags + ["-DX"])) != h0
    (tmp_path / "new_header.h").write_text("// new\n")
    assert build.source_hash(rec._replace(header_dirs=rec.header_dirs + [str(tmp_path)])) != h0
    # the fp32 library is built from what it was built from
    assert build.BACKBONE_CONV.sources == ["conv1x1.hip"] and "csrc_backbone_conv_bf16" not in " ".join(build.BACKBONE_CONV.header_dirs)


def test_kernels_do_not_spill_and_fit_two_waves_per_simd():
    """As tests/test_codeobj.py holds the head's kernels: no spilled register, no scratch memory, at most 256 registers (the kernel asks
    for two work-groups per CU), and the two tile shapes' LDS images side by side twice in a CU's 160 KB."""
    pytest.importorskip("msgpack")
    from os2d_amd import build, codeobj
    if not build.up_to_date(build.BACKBONE_CONV_BF16):
        build.build_library(build.BACKBONE_CONV_BF16, verbose=False)
    kernels = codeobj.kernels(build.BACKBONE_CONV_BF16_LIB_PATH)
    gemms = {n: k for n, k in kernels.items() if "conv1x1_bf16x3_kernel" in n}
    assert len(kernels) == 5 and len(gemms) == 4 and any("pack_kernel" in n for n in kernels)
    for name, k in kernels.items():
        assert k["vgpr_spills"] == 0 and k["scratch_bytes"] == 0 and k["vgprs"] + k["agprs"] <= 256, (name, k)
    print({n: (k["vgprs"], k["agprs"], k["lds_bytes"]) for n, k in kernels.items()})
    assert sorted(k["lds_bytes"] for k in gemms.values()) == [49152, 49152, 61440, 61440]


def test_missing_library_fails_loudly(monkeypatch, tmp_path):
    from os2d_amd import _backbone_conv_bf16_lib as L
    from os2d_amd._native import Os2dLibraryError
    monkeypatch.setattr(L.LIBRARY, "_handle", None)
    monkeypatch.setenv("OS2D_BACKBONE_CONV_BF16_LIB", str(tmp_path / "nope.so"))
    with pytest.raises(Os2dLibraryError, match="no CPU or PyTorch fallback"):
        L.load()


def test_setting_default_environment_and_bad_values(monkeypatch):
    from os2d_amd.modeling import backbone_fused
    from os2d_amd.modeling.feature_extractor import resnet50_c4
    from os2d_amd.modeling.model import Os2dModel
    assert backbone_fused.PRECISIONS == ("f32", "bf16x3") and backbone_fused.ROUTES == ("torch", "fused", "fused_conv1x1")
    assert backbone_fused.FOLDING_ROUTES == ("fused", "fused_conv1x1")
    monkeypatch.delenv("OS2D_BACKBONE_CONV_PRECISION", raising=False)
    monkeypatch.delenv("OS2D_BACKBONE_ROUTE", raising=False)
    ex = resnet50_c4()
    assert ex.conv1x1_precision == "f32" and ex.inference_route == "torch"
    for bad in ("bf16", "f16x3", "", None, "BF16X3"):
        with pytest.raises(ValueError, match="conv1x1_precision is one of"):
            ex.conv1x1_precision = bad
        assert ex.conv1x1_precision == "f32"
    ex.conv1x1_precision = "bf16x3"
    assert ex.conv1x1_precision == "bf16x3" and ex.inference_route == "torch"        # it selects no route
    monkeypatch.setenv("OS2D_BACKBONE_CONV_PRECISION", "bf16x3")
    assert resnet50_c4().conv1x1_precision == "bf16x3" and resnet50_c4().inference_route == "torch"
    assert resnet50_c4(use_group_norm=True).conv1x1_precision == "bf16x3"            # read on "fused_conv1x1" alone: no complaint here
    monkeypatch.setenv("OS2D_BACKBONE_ROUTE", "fused_conv1x1")
    net = Os2dModel(merge_branch_parameters=False)
    for branch in (net.net_feature_maps, net.net_label_features.net_class_features):
        assert branch.inference_route == "fused_conv1x1" and branch.conv1x1_precision == "bf16x3"
    monkeypatch.setenv("OS2D_BACKBONE_CONV_PRECISION", "fast")
    with pytest.raises(ValueError, match="conv1x1_precision is one of"):
        resnet50_c4()


def test_calls_that_stay_on_the_torch_route(monkeypatch):
    """With "fused_conv1x1" and "bf16x3" set: a CPU tensor, grad mode and a BatchNorm in training mode each take the module path, bit for
    bit, and no weight is packed."""
    from os2d_amd.modeling import backbone_fused
    from os2d_amd.modeling.feature_extractor import resnet50_c4
    torch.manual_seed(0)
    ex = resnet50_c4().eval()
    B.perturb_batchnorms(ex, seed=1)
    x = torch.randn(1, 3, 64, 64, generator=torch.Generator().manual_seed(3))
    with torch.no_grad():
        want = ex(x)

    def never(self, *a, **k):
        raise AssertionError("a fused route was taken")
    for name in ("forward", "forward_conv1x1", "packed_weights"):
        monkeypatch.setattr(backbone_fused.FusedBackbone, name, never)
    ex.inference_route, ex.conv1x1_precision = "fused_conv1x1", "bf16x3"
    with torch.no_grad():
        assert not backbone_fused.eligible(ex, x) and torch.equal(ex(x), want)              # a CPU tensor
    assert torch.equal(ex(x), want)                                                         # grad mode
    ex.layer2[1].bn2.train()
    with torch.no_grad():
        assert not backbone_fused.eligible(ex, x)
        mid = ex(x)                                                                          # runs the module path (and updates the statistics)
    assert mid.shape == want.shape


def test_setting_adds_nothing_to_the_module_tree():
    from os2d_amd.modeling.feature_extractor import resnet50_c4
    ex = resnet50_c4().eval()
    keys, params, modules = list(ex.state_dict()), [id(p) for p in ex.parameters()], [n for n, _ in ex.named_modules()]
    buffers = [n for n, _ in ex.named_buffers()]
    ex.inference_route, ex.conv1x1_precision = "fused_conv1x1", "bf16x3"
    runner = ex.fused_backbone()
    assert runner.weight_packs == 0 and runner.rebuilds == 0
    assert ex.fused_backbone() is runner                                  # one runner per extractor
    assert list(ex.state_dict()) == keys and [id(p) for p in ex.parameters()] == params and [n for n, _ in ex.named_modules()] == modules
    assert [n for n, _ in ex.named_buffers()] == buffers
    twin = resnet50_c4()
    twin.load_state_dict(ex.state_dict())                                 # and a state dict travels between the settings
    assert twin.conv1x1_precision == "f32"


# every class of bad argument of the GEMM: those of the fp32 entry point (tests/test_backbone_conv_model.py), the packed weights in the
# place of w, and what the packed weights add.  The fake pointers are far apart unless the case is about overlap; none is dereferenced.
_p = F._p
X, WP, S, T, R, Y, SIZES = F.X, F.WT, F.S, F.T, F.R, F.Y, F.SIZES          # Cin 4, Cout 8: wp has 3 * 32 * 8 elements, 1536 bytes
GEMM_REFUSALS = list(F.REFUSALS) + [
    ((X, _p((1 << 22) + 4), S, T, None, None, None, Y) + SIZES, "wp not aligned (16 bytes)"),
    ((X, _p((1 << 22) + 8), S, T, None, None, None, Y) + SIZES, "wp not aligned (16 bytes)"),
    ((X, _p((1 << 22) + 2), S, T, None, None, None, Y) + SIZES, "wp not aligned (16 bytes)"),
    ((X, WP, S, T, None, None, None, _p((1 << 22) + 1532)) + SIZES, "overlaps wp"),                   # y starts on the last bytes of wp
    ((X, WP, S, T, None, None, None, _p((1 << 22) - 4 * 71)) + SIZES, "overlaps wp"),                 # y ends on the first
]
W = _p(1 << 26)
PACK_REFUSALS = [
    ((None, WP, 8, 4), "null pointer"),
    ((W, None, 8, 4), "null pointer"),
    ((_p((1 << 26) + 2), WP, 8, 4), "w not aligned (4 bytes)"),
    ((W, _p((1 << 22) + 8), 8, 4), "wp not aligned (16 bytes)"),
    ((W, _p((1 << 22) + 2), 8, 4), "wp not aligned (16 bytes)"),
    ((W, WP, 0, 4), "bad shape"),
    ((W, WP, 8, 0), "bad shape"),
    ((W, WP, -8, 4), "bad shape"),
    ((W, WP, 8, -1), "bad shape"),
    ((W, WP, (1 << 20) + 1, 4), "too large"),
    ((W, WP, 8, (1 << 20) + 1), "too large"),
    ((W, W, 8, 4), "overlaps w"),
    ((W, _p((1 << 26) + 112), 8, 4), "overlaps w"),                        # wp starts on the last 16 bytes of w (32 floats)
    ((W, _p((1 << 26) - 1536 + 16), 8, 4), "overlaps w"),                  # wp ends on the first
]


def test_the_cases_are_those_of_the_fp32_entry_point_and_more():
    assert len(F.REFUSALS) == 34 and len(GEMM_REFUSALS) == 39


@pytest.mark.parametrize("k", range(len(GEMM_REFUSALS)))
def test_bad_arguments_are_refused_before_any_launch(k):
    """No device here and the pointers lead nowhere: a call that got as far as a launch would not return -1 with its own text."""
    from os2d_amd import _backbone_conv_bf16_lib as L
    args, text = GEMM_REFUSALS[k]
    assert len(args) == 15
    lib = L.load()
    assert lib.os2d_backbone_conv1x1_bf16x3(*(list(args) + [None])) == -1
    message = lib.os2d_backbone_conv_bf16_last_error().decode()
    assert message.startswith("conv1x1_bf16x3:") and text in message, message
    with pytest.raises(RuntimeError, match=re.escape(message)):
        L.check(-1, "conv1x1_bf16x3")


@pytest.mark.parametrize("k", range(len(PACK_REFUSALS)))
def test_bad_arguments_of_pack_weights_are_refused_before_any_launch(k):
    from os2d_amd import _backbone_conv_bf16_lib as L
    args, text = PACK_REFUSALS[k]
    lib = L.load()
    assert lib.os2d_backbone_conv_bf16_pack_weights(*(list(args) + [None])) == -1
    message = lib.os2d_backbone_conv_bf16_last_error().decode()
    assert message.startswith("pack_weights:") and text in message, message
