"""In-tree build of the eight HIP libraries for gfx950 with hipcc (no JIT cache: the .so files travel with the tree).

    python -m os2d_amd.build                      # build what is stale
    python -m os2d_amd.build --force
    python -m os2d_amd.build --train              # only libos2d_train.so (the head's backward pass)
    python -m os2d_amd.build --eval               # only libos2d_eval.so (the VOC detection metric)
    python -m os2d_amd.build --image              # only libos2d_image.so (the image pyramid from uint8 images)
    python -m os2d_amd.build --augment            # only libos2d_augment.so (padded crops and colour distortion of training images)
    python -m os2d_amd.build --backbone           # only libos2d_backbone.so (the frozen-BatchNorm epilogues of the backbone's inference route)
    python -m os2d_amd.build --backbone-conv      # only libos2d_backbone_conv.so (the backbone's 1x1 convolutions as fp32 MFMA GEMMs with folded-BatchNorm epilogues)
    python -m os2d_amd.build --backbone-conv-bf16 # only libos2d_backbone_conv_bf16.so (the same 1x1 convolutions in split-bf16 arithmetic on the bf16 MFMA)
    python -m os2d_amd.build --variant TAG [--packed on|off|fft] [-DFLAG ...]
                                                  # diagnostic copy under tools/diag_libs/TAG/ (run with OS2D_HIP_LIB=...)
"""
import collections
import functools
import glob
import hashlib
import os
import re
import shutil
import subprocess
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(HERE, "csrc")
SHARED = os.path.join(HERE, "csrc_shared")        # abi_common.h: the error text and launch check of every library
INCLUDE = os.path.join(HERE, "..", "include")
LIB_DIR = os.path.join(HERE, "lib")
VARIANT_DIR = os.path.join(HERE, "..", "tools", "diag_libs")
SOURCES = ["abi.hip", "head_call.hip", "prep.hip", "corr_mfma.hip", "conv_mfma.hip", "conv_f16x3.hip", "conv3_f16x3.hip", "corr_f16x3.hip", "sample_decode.hip", "nms.hip", "detect.hip", "detect_pyramid.hip", "spectral.hip", "spectral_f16.hip", "spectra_pack.hip", "fft.hip", "dft_mfma.hip"]
ARCH = "gfx950"
FLAGS = ["--offload-arch=" + ARCH, "-O3", "-std=c++17", "-fPIC", "-fno-gpu-rdc", "-Wall", "-Wno-unused-function"]
# No packed-FP32 VALU instructions (v_pk_add_f32 / v_pk_mul_f32 / v_pk_fma_f32) in the translation units listed in
# NO_PACKED_FP32 - all of them.  Measured on MI355X (docs/DESIGN_HISTORY_r1-r3.md section 8, profiles/r03_packed_fp32/): such instructions
# occasionally return wrong values in lanes 48 - 63 of a wave while waves of ANOTHER kernel on the same CU issue fp16 MFMA
# instructions at full rate (other HIP streams); a register-only victim without LDS, barriers or memory accesses reproduces
# it (tools/repro_packed_fp32.hip), scalar v_fma_f32 code never does, fp32-MFMA / plain-VALU neighbours never trigger it, and
# the library's transforms fail identically with full __syncthreads() barriers - it is not a race of ours.  Any kernel of the
# library can meet another stream's conv / correlation / spectral-GEMM waves under the per-level-stream pyramid runner.
PACKED_OFF = ["-Xclang", "-target-feature", "-Xclang", "-packed-fp32-ops"]
NO_PACKED_FP32 = set(SOURCES)             # which translation units are compiled without the packed instructions
FLAGS += os.environ.get("OS2D_EXTRA_HIPCC_FLAGS", "").split()      # kernel experiments (-DOS2D_DIAG_...); part of the source hash

# A library is a record; headers(), source_hash(), up_to_date() and build_library() are the whole build, for any of them.
#   flags        of every unit
#   unit_flags   {source: flags of that unit on top}
#   header_dirs  the directories whose *.h its units may include: all of them are hashed, and a quoted #include that resolves
#                nowhere in them fails the tests
#   header       the public C ABI under include/
#   env          the environment variable that names another file to load instead (os2d_amd/_native.py)
Library = collections.namedtuple("Library", "name csrc sources flags unit_flags header_dirs header env")

HIP = Library("libos2d_hip.so", CSRC, SOURCES, FLAGS, {s: PACKED_OFF for s in NO_PACKED_FP32}, [CSRC, SHARED], "os2d_hip.h", "OS2D_HIP_LIB")
# The backward pass of the head is a library of its own (include/os2d_train.h): libos2d_hip.so keeps exactly the sources and
# kernels above.  Its units may include the forward's headers (csrc/*.h) to share the sampling and decode arithmetic.
# objective.hip restates the reference's IoU and box encoding operation for operation: a fused multiply-add would round
# differently from the CPU reference
TRAIN_CSRC = os.path.join(HERE, "csrc_train")
# train.hip: the C ABI of the backward pass and its per-location kernels
# train_gemm.hip: the GEMMs in fp32 and in split-fp16 arithmetic and their five launch sites (the `arith` of the *_ex entry points)
# decode_backward.hip: the resample / pool / box decode backward, float-atomic and order-independent
# mining.hip needs no flag: every function of it that rounds (csrc/detect_common.h, mining_crop.h) switches contraction off itself
# shb_planes.hip: the split-half blocked activations of an f16x3 training forward as the fp32 planes the backward reads
# bn_live.hip: batch-statistics BatchNorm of the TransformNet (statistics, normalise + ReLU, backward through the statistics)
# optim.hip: gradient norm, clip, NaN guard and the step of all eight methods as multi-tensor kernels; needs no flag either: every function
#            of it that rounds switches contraction off itself
# range_plan.hip: BatchNorm fold, bounds and exponents of the f16x3 packing in float64 - what a parameter change makes stale every
#                 step (here and not in libos2d_hip.so, whose kernel set is pinned); contraction off in its own functions as well
TRAIN = Library("libos2d_train.so", TRAIN_CSRC, ["train.hip", "train_gemm.hip", "decode_backward.hip", "objective.hip", "mining.hip", "shb_planes.hip", "bn_live.hip",
                                                 "optim.hip", "range_plan.hip"],
                FLAGS + PACKED_OFF,
                {"objective.hip": ["-ffp-contract=off"]},
                [TRAIN_CSRC, CSRC, SHARED], "os2d_train.h", "OS2D_TRAIN_LIB")
# The VOC evaluation (include/os2d_eval.h): the kernel list of libos2d_hip.so and the ABI of libos2d_train.so stay what they
# are.  Its units may include csrc/detect_common.h for the score sort key.  The IoU of the match step must have the bits of the
# reference's CPU arithmetic, and the area under the curve is a sum of separately rounded products: no fused multiply-adds in
# any unit
EVAL_CSRC = os.path.join(HERE, "csrc_eval")
EVAL = Library("libos2d_eval.so", EVAL_CSRC, ["match.hip", "sort.hip", "metric.hip"], FLAGS + PACKED_OFF + ["-ffp-contract=off"], {},
               [EVAL_CSRC, CSRC, SHARED], "os2d_eval.h", "OS2D_EVAL_LIB")
# The image pyramid from uint8 images (include/os2d_image.h).  Integer arithmetic and a table lookup: no floating-point
# operation whose rounding a flag could change.  Its units include none of csrc/*.h.  The kernel is a template in
# csrc_image/resample_kernel.h, instantiated here for windows inside the image.
IMAGE_CSRC = os.path.join(HERE, "csrc_image")
IMAGE = Library("libos2d_image.so", IMAGE_CSRC, ["resample.hip"], FLAGS + PACKED_OFF, {}, [IMAGE_CSRC, SHARED], "os2d_image.h", "OS2D_IMAGE_LIB")
# The training images (include/os2d_augment.h): the same resample template instantiated for windows that leave the image, and
# PIL's colour operations.  A fifth library, because the kernel set and the ABI of libos2d_image.so are what they are (its two
# kernels are pinned by its tests).  color.hip restates PIL's float arithmetic and every function of it that rounds switches
# contraction off itself; the units include csrc_image/*.h and none of csrc/*.h.
AUGMENT_CSRC = os.path.join(HERE, "csrc_augment")
AUGMENT = Library("libos2d_augment.so", AUGMENT_CSRC, ["resample_padded.hip", "color.hip"], FLAGS + PACKED_OFF, {}, [AUGMENT_CSRC, IMAGE_CSRC, SHARED],
                  "os2d_augment.h", "OS2D_AUGMENT_LIB")
# The backbone's frozen-inference route (include/os2d_backbone.h): what runs between the convolutions of a
# ResNet with folded BatchNorms.  Its kernels run next to MIOpen's convolutions and, under the pyramid runner, next to other
# streams' MFMA waves: no packed FP32 (the finding above).  The units include none of csrc/*.h.
BACKBONE_CSRC = os.path.join(HERE, "csrc_backbone")
BACKBONE = Library("libos2d_backbone.so", BACKBONE_CSRC, ["pointwise.hip"], FLAGS + PACKED_OFF, {}, [BACKBONE_CSRC, SHARED],
                   "os2d_backbone.h", "OS2D_BACKBONE_LIB")
LIBRARIES = [HIP, TRAIN, EVAL, IMAGE]          # forward, backward, evaluation, image pyramid
ALL_LIBRARIES = LIBRARIES + [AUGMENT]          # the libraries of the head, the metric and the images
BUILT_LIBRARIES = ALL_LIBRARIES + [BACKBONE]   # the six that tests/test_backbone_model.py pins
# The backbone's 1x1 convolutions as fp32 GEMMs on the fp32-input MFMA with the fold, residual and ReLU as the epilogue
# (include/os2d_backbone_conv.h).  A library of its own: the exports and the ABI version of
# libos2d_backbone.so are what they are.  Its unit includes csrc_backbone/conv1x1_common.h - the epilogue, the argument contract
# and the tile plan of a 1x1 GEMM, on top of backbone_common.h's fold - and keeps the main loop; no packed FP32, as for every kernel
# that runs next to other streams.
BACKBONE_CONV_CSRC = os.path.join(HERE, "csrc_backbone_conv")
BACKBONE_CONV = Library("libos2d_backbone_conv.so", BACKBONE_CONV_CSRC, ["conv1x1.hip"], FLAGS + PACKED_OFF, {},
                        [BACKBONE_CONV_CSRC, BACKBONE_CSRC, SHARED], "os2d_backbone_conv.h", "OS2D_BACKBONE_CONV_LIB")
EVERY_LIBRARY = BUILT_LIBRARIES + [BACKBONE_CONV]      # the seven that tests/test_backbone_conv_model.py pins
# The same 1x1 convolutions in split-bf16 arithmetic: three bf16 parts per fp32 operand, six products on the bf16 MFMA
# (include/os2d_backbone_conv_bf16.h).  An eighth library: the exports, the ABI version and the signature of
# libos2d_backbone_conv.so are what they are.  bf16x3_split.h of its directory is the split, for the device and for a host program; the
# epilogue, the argument contract and the tile plan are csrc_backbone/conv1x1_common.h, the text the fp32 unit includes.  No packed FP32.
BACKBONE_CONV_BF16_CSRC = os.path.join(HERE, "csrc_backbone_conv_bf16")
BACKBONE_CONV_BF16 = Library("libos2d_backbone_conv_bf16.so", BACKBONE_CONV_BF16_CSRC, ["conv1x1_bf16x3.hip"], FLAGS + PACKED_OFF, {},
                             [BACKBONE_CONV_BF16_CSRC, BACKBONE_CSRC, SHARED], "os2d_backbone_conv_bf16.h", "OS2D_BACKBONE_CONV_BF16_LIB")
EVERYTHING = EVERY_LIBRARY + [BACKBONE_CONV_BF16]      # what build() makes


def lib_path(lib):
    return os.path.join(LIB_DIR, lib.name)


LIB_PATH, TRAIN_LIB_PATH, EVAL_LIB_PATH, IMAGE_LIB_PATH, AUGMENT_LIB_PATH, BACKBONE_LIB_PATH, BACKBONE_CONV_LIB_PATH = [lib_path(lib) for lib in EVERY_LIBRARY]
BACKBONE_CONV_BF16_LIB_PATH = lib_path(BACKBONE_CONV_BF16)


def headers(lib=HIP):
    """Every header a unit of the library can include: *.h of its header directories + its public ABI header.  Globbed, not
    listed: a new header (fft_regs.h was missed in round 2) is part of the source hash from the day it exists."""
    return [h for d in lib.header_dirs for h in sorted(glob.glob(os.path.join(d, "*.h")))] + [os.path.join(INCLUDE, lib.header)]


def local_includes(path):
    """Names of the quoted #include files of a source (used by the tests: each must be in headers())."""
    with open(path) as f:
        return re.findall(r'^\s*#\s*include\s+"([^"]+)"', f.read(), flags=re.M)


def unit_flags(lib, source):
    """hipcc flags of one translation unit of a library."""
    return lib.flags + lib.unit_flags.get(source, [])


def flags_for(source, packed=None):
    """hipcc flags of one unit of the forward library.  packed: None = the product setting, 'on' / 'off' = every unit with /
    without packed-FP32 instructions, 'fft' = only fft.hip without them (diagnostic variants, build_variant)."""
    if packed is None:
        return unit_flags(HIP, source)
    return HIP.flags + (PACKED_OFF if packed == "off" or (packed == "fft" and source == "fft.hip") else [])


def _hipcc():
    for cand in (os.environ.get("HIPCC"), shutil.which("hipcc"), "/opt/rocm/bin/hipcc"):
        if cand and os.path.exists(cand):
            return cand
    raise RuntimeError("hipcc not found (set HIPCC or install ROCm under /opt/rocm)")


def source_hash(lib=HIP):
    """sha256 over every source, header and the compiler flags of every unit: what decides whether the library is up to
    date (mtimes do not survive a copy of the tree to another machine, contents do)."""
    h = hashlib.sha256()
    for s in lib.sources:
        h.update((s + ":" + " ".join(unit_flags(lib, s)) + "\n").encode())
    for path in [os.path.join(lib.csrc, s) for s in lib.sources] + headers(lib):
        h.update(os.path.basename(path).encode())
        with open(path, "rb") as f:
            h.update(f.read())
    return h.hexdigest()


def up_to_date(lib=HIP):
    """True when the library exists and was built from exactly the sources in the tree (the .srchash next to it)."""
    if not (os.path.exists(lib_path(lib)) and os.path.exists(lib_path(lib) + ".srchash")):
        return False
    with open(lib_path(lib) + ".srchash") as f:
        return f.read().strip() == source_hash(lib)


def _jobs():
    """Compilers started at once: 16 at the most, fewer when MAX_JOBS says so (a shared host reports far more CPUs than a
    command may use)."""
    return max(1, min(16, int(os.environ.get("MAX_JOBS") or 16)))


def _compile(hipcc, csrc, units, build_dir, verbose):
    """units: [(source, flags)].  Compiles every one of them, _jobs() at a time; returns the objects."""
    os.makedirs(build_dir, exist_ok=True)
    objs, procs = [], []
    for s, flags in units:
        objs.append(os.path.join(build_dir, s.replace(".hip", ".o")))
        cmd = [hipcc] + flags + ["-c", os.path.join(csrc, s), "-o", objs[-1]]
        if verbose:
            print("[os2d_amd.build]", " ".join(cmd), flush=True)
        procs.append((cmd, subprocess.Popen(cmd)))
        if len(procs) >= _jobs():
            _wait(procs)
    _wait(procs)
    return objs


def _wait(procs):
    failed = [cmd for cmd, p in procs if p.wait() != 0]
    del procs[:]
    if failed:
        raise subprocess.CalledProcessError(1, failed[0])


def _link(hipcc, objs, out, verbose):
    cmd = [hipcc, "--offload-arch=" + ARCH, "-shared", "-fPIC", "-o", out] + objs
    if verbose:
        print("[os2d_amd.build]", " ".join(cmd), flush=True)
    subprocess.check_call(cmd)


def build_library(lib, force=False, verbose=True):
    """Compile every unit of the library for gfx950 and link it, unless its stamp matches the tree.  Object files carry no
    record of the flags they were compiled with, so a stale stamp recompiles all of them.  Returns the library's path."""
    path = lib_path(lib)
    if not force and up_to_date(lib):
        return path
    hipcc = _hipcc()
    os.makedirs(LIB_DIR, exist_ok=True)
    digest = source_hash(lib)
    objs = _compile(hipcc, lib.csrc, [(s, unit_flags(lib, s)) for s in lib.sources], os.path.join(lib.csrc, "build"), verbose)
    tmp = path + ".tmp.{}".format(os.getpid())          # link aside, then rename: a concurrent loader never maps a
    _link(hipcc, objs, tmp, verbose)                    # half-written file
    os.replace(tmp, path)
    with open(path + ".srchash.tmp", "w") as f:
        f.write(digest + "\n")
    os.replace(path + ".srchash.tmp", path + ".srchash")
    return path


def build(force=False, verbose=True):
    """Build every library that is stale (force: all of them).  Returns the forward library's path."""
    for lib in EVERYTHING:
        build_library(lib, force=force, verbose=verbose)
    return LIB_PATH


# The names the per-library test fixtures call: each is the record's field or the one function bound to the record.
TRAIN_SOURCES, EVAL_SOURCES, IMAGE_SOURCES, AUGMENT_SOURCES, BACKBONE_SOURCES = TRAIN.sources, EVAL.sources, IMAGE.sources, AUGMENT.sources, BACKBONE.sources
build_train, build_eval, build_image, build_augment, build_backbone, build_backbone_conv = [functools.partial(build_library, lib) for lib in (TRAIN, EVAL, IMAGE, AUGMENT, BACKBONE,
                                                                                                                                              BACKBONE_CONV)]
build_backbone_conv_bf16 = functools.partial(build_library, BACKBONE_CONV_BF16)
train_up_to_date = functools.partial(up_to_date, TRAIN)


def build_variant(tag, packed=None, extra=(), verbose=False):
    """A DIAGNOSTIC copy of the library (other flags, -DOS2D_DIAG_... switches) under tools/diag_libs/<tag>/; the product
    library is untouched.  Built HERE (hipcc cross-compiles) so that a GPU call spends its minutes measuring:
    OS2D_HIP_LIB=tools/diag_libs/<tag>/libos2d_hip.so selects it at run time (os2d_amd/_lib.py)."""
    hipcc = _hipcc()
    out = os.path.join(VARIANT_DIR, tag)
    objs = _compile(hipcc, CSRC, [(s, flags_for(s, packed) + list(extra)) for s in SOURCES], os.path.join(out, "build"), verbose)
    lib = os.path.join(out, "libos2d_hip.so")
    _link(hipcc, objs, lib, False)
    shutil.rmtree(os.path.join(out, "build"))
    with open(os.path.join(out, "FLAGS.txt"), "w") as f:
        f.write("packed={} extra={}\n".format(packed, " ".join(extra)))
    return lib


if __name__ == "__main__":
    argv = sys.argv[1:]
    if "--variant" in argv:
        i = argv.index("--variant")
        tag = argv[i + 1]
        packed = argv[argv.index("--packed") + 1] if "--packed" in argv else None
        print(build_variant(tag, packed, [a for a in argv if a.startswith("-D")], verbose=True))
    else:
        only = [lib for lib, switch in ((TRAIN, "--train"), (EVAL, "--eval"), (IMAGE, "--image"), (AUGMENT, "--augment"), (BACKBONE, "--backbone"),
                                         (BACKBONE_CONV, "--backbone-conv"), (BACKBONE_CONV_BF16, "--backbone-conv-bf16")) if switch in argv]
        if only:
            print(build_library(only[0], force="--force" in argv))
        else:
            print(build(force="--force" in argv))
