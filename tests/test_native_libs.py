"""CPU: what holds for each of the four HIP libraries alike - the build record (os2d_amd/build.py), the public header, the
ctypes binding and the built file agree, the build stamp reacts to everything a unit is compiled from, the loader refuses a
missing file, and every library keeps the calling thread's error text to itself (os2d_amd/csrc_shared/abi_common.h).  What is
specific to one library (refusal tables, size helpers, kernel lists) is in its own test_*_abi.py."""
import ctypes
import importlib
import os
import re
import subprocess
import threading

import pytest

from os2d_amd import build
from os2d_amd._native import Os2dLibraryError

REPO = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
fake = ctypes.c_void_p(256)      # never dereferenced: the calls below are refused by their argument checks


def _refuse_hip(lib):
    return lib.os2d_head_workspace_bytes(1, 1, 0, 60, 80, 6, ctypes.byref(ctypes.c_size_t())), b"C"


def _refuse_train(lib):
    return lib.os2d_train_params_backward(fake, 4, 5, 9, 13, fake, None, None), b"os2d_train_params_backward: bad shape"


def _refuse_eval(lib):
    return lib.os2d_eval_count_gt(fake, fake, 3, 0, fake, fake, None), b"count_gt: bad shape"


def _refuse_image(lib):
    args = [None, 1, 64, 48, 192, 192 * 48, 0, 0, 64, 48, 0, 0, fake, fake, fake, 5, fake, fake, fake, 5, 32, 24, fake, fake, 0, None]
    return lib.os2d_image_resample(*args), b"resample: null pointer"


# key -> (record, binding module, version #define, ABI version, exports must EQUAL the binding (else: contain it), a call that
#         is refused before any launch, headers its units are known to include)
CASES = {
    "hip": (build.HIP, "_lib", "OS2D_ABI_VERSION", 9, False, _refuse_hip, {"fft_regs.h", "os2d_common.h", "abi_common.h", "os2d_hip.h"}),
    "train": (build.TRAIN, "_train_lib", "OS2D_TRAIN_ABI_VERSION", 2, True, _refuse_train, {"os2d_common.h", "abi_common.h", "os2d_train.h"}),
    "eval": (build.EVAL, "_eval_lib", "OS2D_EVAL_ABI_VERSION", 1, True, _refuse_eval, {"detect_common.h", "abi_common.h", "os2d_eval.h"}),
    "image": (build.IMAGE, "_image_lib", "OS2D_IMAGE_ABI_VERSION", 1, True, _refuse_image, {"image_common.h", "abi_common.h", "os2d_image.h"}),
}
KEYS = sorted(CASES)


def binding(key):
    return importlib.import_module("os2d_amd." + CASES[key][1])


def last_error(key):
    b = binding(key)
    return getattr(b.load(), b.LIBRARY.error_fn)()


@pytest.fixture(scope="module")
def built():
    """build() is what a clean checkout runs: afterwards every library is there and up to date."""
    assert build.build(verbose=False) == build.LIB_PATH
    return True


def test_the_table_is_the_four_libraries():
    assert [c[0] for c in CASES.values()] == build.LIBRARIES and len({lib.name for lib in build.LIBRARIES}) == 4
    assert [build.lib_path(lib) for lib in build.LIBRARIES] == [build.LIB_PATH, build.TRAIN_LIB_PATH, build.EVAL_LIB_PATH, build.IMAGE_LIB_PATH]
    assert [lib.env for lib in build.LIBRARIES] == ["OS2D_HIP_LIB", "OS2D_TRAIN_LIB", "OS2D_EVAL_LIB", "OS2D_IMAGE_LIB"]
    for key in KEYS:
        assert binding(key).LIBRARY.record is CASES[key][0]


@pytest.mark.parametrize("key", KEYS)
def test_build_leaves_the_library_up_to_date(built, key):
    lib = CASES[key][0]
    assert os.path.exists(build.lib_path(lib)) and build.up_to_date(lib)
    assert os.path.exists(build.lib_path(lib) + ".srchash")                       # one stamp, next to the library
    assert build.up_to_date() == build.up_to_date(build.HIP)                      # no argument: the forward library


@pytest.mark.parametrize("key", KEYS)
def test_header_and_binding_agree(key):
    lib, _, define, version = CASES[key][:4]
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(REPO, "include", lib.header)).read(), flags=re.S)
    assert sorted(set(re.findall(r"\b(os2d_[a-z0-9_]+)\s*\(", text))) == sorted(binding(key).SIGNATURES)
    assert re.search(r"^#define {} (\d+)$".format(define), text, flags=re.M).group(1) == str(binding(key).ABI_VERSION) == str(version)


@pytest.mark.parametrize("key", KEYS)
def test_library_exports_the_declared_symbols_and_reports_its_abi(built, key):
    lib, _, _, version, exact = CASES[key][:5]
    out = subprocess.check_output(["nm", "-D", "--defined-only", build.lib_path(lib)]).decode()
    exported = set(re.findall(r" T (os2d_\w+)", out))
    names = set(binding(key).SIGNATURES)
    assert not names - exported, "not exported: {}".format(sorted(names - exported))
    if exact:
        assert exported == names
    assert "os2d_error_text" not in out and "os2d_set_error" not in out        # the error text is nobody else's to bind to
    b = binding(key)
    assert getattr(b.load(), b.LIBRARY.version_fn)() == b.ABI_VERSION == version


@pytest.mark.parametrize("key", KEYS)
def test_flags_and_headers_are_part_of_the_build_stamp(tmp_path, key):
    """Object files carry no record of their flags and a header can be edited without its includers: the stamp covers the
    flags of every unit (OS2D_EXTRA_HIPCC_FLAGS is part of them), the per-unit ones, and every header a unit may include."""
    lib = CASES[key][0]
    h0 = build.source_hash(lib)
    assert build.source_hash(lib) == h0
    assert build.source_hash(lib._replace(flags=lib.flags + ["-DOS2D_SOME_EXPERIMENT"])) != h0
    unit = lib.sources[-1]
    assert build.source_hash(lib._replace(unit_flags=dict(lib.unit_flags, **{unit: ["-DOS2D_ONE_UNIT"]}))) != h0
    (tmp_path / "new_header.h").write_text("// new\n")
    assert build.source_hash(lib._replace(header_dirs=lib.header_dirs + [str(tmp_path)])) != h0


def test_extra_flags_from_the_environment_reach_every_library():
    script = "from os2d_amd import build; print(all('-DOS2D_DIAG_X' in build.unit_flags(l, s) for l in build.LIBRARIES for s in l.sources))"
    out = subprocess.check_output([os.sys.executable, "-c", script], cwd=REPO, env=dict(os.environ, OS2D_EXTRA_HIPCC_FLAGS="-DOS2D_DIAG_X"))
    assert out.decode().strip() == "True"


def test_unit_flags_of_every_library():
    """No packed-FP32 instructions anywhere; no fused multiply-adds in the evaluation and in objective.hip, and nowhere else."""
    contract = {(lib.name, s) for lib in build.LIBRARIES for s in lib.sources if "-ffp-contract=off" in build.unit_flags(lib, s)}
    assert contract == {("libos2d_eval.so", s) for s in build.EVAL.sources} | {("libos2d_train.so", "objective.hip")}
    for lib in build.LIBRARIES:
        for s in lib.sources:
            flags = build.unit_flags(lib, s)
            assert all(f in flags for f in build.PACKED_OFF) and "--offload-arch=gfx950" in flags, (lib.name, s)
            assert [f for f in flags if f not in build.PACKED_OFF + ["-ffp-contract=off"]] == build.FLAGS
    assert build.unit_flags(build.IMAGE, "resample.hip") == build.FLAGS + build.PACKED_OFF
    assert all(build.flags_for(s) == build.unit_flags(build.HIP, s) for s in build.SOURCES) and build.HIP.sources is build.SOURCES


def test_sources_are_disjoint_and_present():
    for i, a in enumerate(build.LIBRARIES):
        assert all(os.path.exists(os.path.join(a.csrc, s)) for s in a.sources)
        for b in build.LIBRARIES[i + 1:]:
            assert not set(a.sources) & set(b.sources) and a.csrc != b.csrc


@pytest.mark.parametrize("key", KEYS)
def test_every_quoted_include_is_part_of_the_build_stamp(key):
    """fft_regs.h (all the register DFTs) was in neither the hash nor the object dependencies, so editing it left a
    stale library in use.  Headers are globbed per directory; every quoted #include of every source and header of a library
    must resolve to one of them."""
    lib, known = CASES[key][0], CASES[key][6]
    names = {os.path.basename(h) for h in build.headers(lib)}
    assert known <= names
    for path in [os.path.join(lib.csrc, s) for s in lib.sources] + build.headers(lib):
        for inc in build.local_includes(path):
            assert os.path.basename(inc) in names, (path, inc)
    forward_only = {os.path.basename(h) for h in build.headers(build.HIP)} - {"abi_common.h"}
    assert bool(forward_only & names) == (key != "image")             # the image library includes none of csrc/*.h


@pytest.mark.parametrize("key", KEYS)
def test_missing_library_fails_loudly(monkeypatch, tmp_path, key):
    b = binding(key)
    monkeypatch.setattr(b.LIBRARY, "_handle", None)
    monkeypatch.setenv(CASES[key][0].env, str(tmp_path / "nope.so"))           # the override skips the stale check
    assert b.lib_path() == str(tmp_path / "nope.so")
    with pytest.raises(Os2dLibraryError, match="no CPU or PyTorch fallback"):
        b.load()


@pytest.mark.parametrize("key", KEYS)
def test_each_library_keeps_its_own_error_text_per_thread(built, key):
    others = [k for k in KEYS if k != key]
    before = {k: last_error(k) for k in others}
    rc, message = CASES[key][5](binding(key).load())
    assert rc == -1 and message in last_error(key)
    assert {k: last_error(k) for k in others} == before
    mine = last_error(key)
    seen = {}

    def second_thread():
        seen["start"] = {k: last_error(k) for k in KEYS}
        seen["rc"], _ = CASES[key][5](binding(key).load())
        seen["after"] = {k: last_error(k) for k in KEYS}

    t = threading.Thread(target=second_thread)
    t.start()
    t.join()
    assert seen["start"] == {k: b"" for k in KEYS}                   # a new thread's texts start empty
    assert seen["rc"] == -1 and message in seen["after"][key] and all(seen["after"][k] == b"" for k in others)
    assert last_error(key) == mine and {k: last_error(k) for k in others} == before
    with pytest.raises(RuntimeError, match=re.escape(mine.decode())):
        binding(key).check(rc, "the call")
