"""CPU: the host-side helpers of libos2d_hip.so (sizes, argument checks, transform plans; no compute calls) and its packed-FP32
setting.  What the four libraries have in common - header, binding, exports, build stamp - is in test_native_libs.py."""
import ctypes

import pytest


@pytest.fixture(scope="module")
def lib_path():
    from os2d_amd import build
    return build.build(verbose=False)




def test_library_loads_and_reports_abi(lib_path):
    from os2d_amd import _lib
    lib = _lib.load()
    assert lib.os2d_abi_version() == _lib.ABI_VERSION
    # pure host-side helpers (no device needed)
    assert lib.os2d_packed_conv_floats(1) == 113 * 49 * 2 * 128
    assert lib.os2d_packed_conv_floats(2) == 64 * 25 * 2 * 64
    assert lib.os2d_packed_conv_floats(3) == 32 * 25 * 2 * 32
    assert lib.os2d_packed_bias_floats(1) == 3 * 128      # folded bias | 2^-weight_exp | 2^out_exp per row
    assert lib.os2d_plane_floats(60, 80) % 64 == 0 and lib.os2d_plane_floats(60, 80) >= 63 * 83
    n = ctypes.c_size_t()
    assert lib.os2d_head_workspace_bytes(1, 64, 1024, 60, 80, 6, ctypes.byref(n)) == 0 and n.value > 0
    one = ctypes.c_size_t()
    assert lib.os2d_head_workspace_bytes(1, 1, 1024, 60, 80, 6, ctypes.byref(one)) == 0 and one.value < n.value
    # argument errors are reported through return codes + os2d_last_error, never exceptions
    assert lib.os2d_head_workspace_bytes(1, 1, 0, 60, 80, 6, ctypes.byref(n)) == -1 and b"C" in lib.os2d_last_error()
    assert lib.os2d_head_workspace_bytes(1, 1, 1023, 60, 80, 6, ctypes.byref(n)) == 0      # any channel count (round 6; the reference has no constraint)
    assert lib.os2d_head_workspace_bytes(1, 1, 1024, 60, 80, 5, ctypes.byref(n)) == -1
    # widest map: 3600 columns (the transform planner's 48 tiles per axis); the direct 7x7 kernels stop at 209 - beyond that the head
    # runs the layer in the frequency domain (tiled) whatever the batch - and the 5x5 kernels' linear slabs at 316: column strips
    assert lib.os2d_head_workspace_bytes(1, 1, 1024, 60, 316, 6, ctypes.byref(n)) == 0
    assert lib.os2d_head_workspace_bytes(1, 1, 1024, 60, 640, 6, ctypes.byref(n)) == 0
    assert lib.os2d_head_workspace_bytes(1, 1, 1024, 4, 3600, 6, ctypes.byref(n)) == 0
    assert lib.os2d_head_workspace_bytes(1, 1, 1024, 4, 3601, 6, ctypes.byref(n)) == -1 and b"width" in lib.os2d_last_error()
    # tallest map: 2784 rows (48 tiles of 58 rows); one more fails in the argument check, and both frequency-domain planners have a
    # plan for every height up to the limit at the benchmark's width (a taller map used to fail inside the planner)
    assert lib.os2d_head_workspace_bytes(1, 1, 1024, 2784, 4, 6, ctypes.byref(n)) == 0
    assert lib.os2d_head_workspace_bytes(1, 1, 1024, 2785, 4, 6, ctypes.byref(n)) == -1 and b"height" in lib.os2d_last_error()
    for prec in (3, 4, 5):       # OS2D_PRECISION_FFT, FFTX3, FFT32
        for h in (1, 61, 64, 65, 117, 1000, 2784):
            assert lib.os2d_head_workspace_bytes_ex(1, 1, 64, h, 80, 6, prec, ctypes.byref(n)) == 0, (prec, h, lib.os2d_last_error())



def test_packed_fp32_setting_is_per_translation_unit():
    """docs/DESIGN_HISTORY_r1-r3.md section 8: v_pk_*_f32 results were wrong in 16-lane groups next to MFMA-heavy kernels of other streams.
    The switch is per translation unit (build.NO_PACKED_FP32); the transforms - the kernels it was found in - are always in."""
    from os2d_amd import build
    assert "fft.hip" in build.NO_PACKED_FP32
    assert "-packed-fp32-ops" in build.flags_for("fft.hip")
    for s in build.SOURCES:
        assert ("-packed-fp32-ops" in build.flags_for(s)) == (s in build.NO_PACKED_FP32)
    assert "-packed-fp32-ops" not in build.flags_for("fft.hip", packed="on")
    assert "-packed-fp32-ops" in build.flags_for("nms.hip", packed="off")
    assert "-packed-fp32-ops" not in build.flags_for("nms.hip", packed="fft")




def test_fft_plan_host_logic():
    """os2d_fft_sizes / os2d_fft_tiles are host code: transform sizes of the frequency-domain 7x7 layer for the pyramid
    levels of BASELINE.json configs[4] (the 96 x 128 level is cut into overlap-save tiles), the invariants every plan must
    satisfy for every map (the in-LDS FFTs serve precisions "fft" / "fft32"), and the fp16 scale of the input spectra."""
    from freq_util import fft_sizes, fft_tiles
    from os2d_amd import _lib
    lib = _lib.load()

    def plan(h, w):          # both calls raise unless they return 0
        return (0,) + fft_sizes(h, w) + fft_tiles(h, w)

    expected = {(30, 40): (36, 48), (38, 50): (42, 54), (48, 64): (54, 72), (60, 80): (64, 84), (72, 96): (84, 108), (84, 112): (96, 128)}
    for (h, w), (p, q) in expected.items():
        rc, P, Q, nb, ty, tx, th, tw = plan(h, w)
        assert rc == 0 and (P, Q) == (p, q) and nb == (p * (q // 2 + 1) + 7) // 8 * 8
        assert (ty, tx, th, tw) == (1, 1, h, w)              # these fit one in-LDS transform
    # the largest level of the 7-scale pyramid (reference os2d/config.py:194): 108 x 144 would need 177 KB of LDS -> four
    # tiles of 48 x 64 outputs, each a 54 x 72 transform (the size the 48 x 64 level uses: one set of weight spectra)
    assert plan(96, 128) == (0, 54, 72, 2000, 2, 2, 48, 64)
    for h in list(range(1, 100, 7)) + [120, 157, 300]:
        for w in list(range(1, 130, 9)) + [150, 209]:
            rc, P, Q, nb, ty, tx, th, tw = plan(h, w)
            assert rc == 0, (h, w)                           # every map the head accepts has a plan
            assert ty >= 1 and tx >= 1 and ty * th >= h and tx * tw >= w and (ty - 1) * th < h and (tx - 1) * tw < w
            assert P >= (th + 6 if ty > 1 else h + 3) and Q >= (tw + 6 if tx > 1 else w + 3)
            assert P % 2 == 0 and Q % 2 == 0 and nb % 8 == 0 and nb >= P * (Q // 2 + 1)
            for n in (P, Q):            # 2^a 3^b, or one of the sizes with a factor 7 that have a two-stage form
                m = n
                while m % 2 == 0:
                    m //= 2
                while m % 3 == 0:
                    m //= 3
                assert m == 1 or n in (42, 84)
    # |X| <= samples of one window: 60 x 80 -> 2^3 * 4800 <= 65504; a 96 x 128 map's window is a 54 x 70 tile + halo -> 2^4
    assert lib.os2d_spectral_xscale(60, 80) == 8.0 and lib.os2d_spectral_xscale(96, 128) == 16.0


def test_dft_plan_host_logic():
    """os2d_dft_sizes (precision "fftx3": the transforms as matrix products, dft_mfma.hip) is host code.  Any P % 4 == 0 <= 64
    and even Q <= 94 could be a transform size; the default policy plans every map on SIX canonical sizes - the exact transforms
    of the 7-scale pyramid of a 1280 x 960 image - through overlap-save tiles, so that the weight spectra of a whole dataset are
    2.4 GB, not one 0.2 - 0.7 GB set per map shape; every map up to the head's width limit has a plan."""
    from freq_util import dft_sizes
    from os2d_amd import _lib
    lib = _lib.load()

    def plan(h, w):          # the call raises unless it returns 0
        P, Q, nb, tiles = dft_sizes(h, w)
        return (0, P, Q, nb) + tiles

    canonical = {(36, 46), (44, 54), (48, 62), (52, 68), (56, 70), (64, 84)}
    assert plan(60, 80) == (0, 64, 84, 2752, 1, 1, 60, 80, 60, 80)
    assert plan(30, 40)[:4] == (0, 36, 46, 864) and plan(38, 50)[:4] == (0, 44, 54, 1232) and plan(48, 64)[:4] == (0, 52, 68, 52 * 35 + 4)
    assert plan(72, 96)[1:8] == (44, 54, 1232, 2, 2, 36, 48) and plan(84, 112)[1:8] == (48, 62, 1536, 2, 2, 42, 56)
    assert plan(96, 128)[1:8] == (56, 70, 2016, 2, 2, 48, 64)
    assert sum(p * (q // 2 + 1) for p, q in canonical) * 128 * 232 * 8 < 2.5e9          # all six sets of weight spectra
    for h in list(range(1, 100, 7)) + [120, 157, 300]:
        for w in list(range(1, 130, 9)) + [150, 209, 260, 316, 317, 400, 640, 1000, 3600]:
            rc, P, Q, nb, ty, tx, th, tw, lh, lw = plan(h, w)
            assert rc == 0, (h, w)
            assert ty >= 1 and tx >= 1 and ty * th >= h and tx * tw >= w and (ty - 1) * th < h and (tx - 1) * tw < w
            assert (lh, lw) == (th + 6 if ty > 1 else h, tw + 6 if tx > 1 else w)
            assert P >= (th + 6 if ty > 1 else h + 3) and Q >= (tw + 6 if tx > 1 else w + 3)
            assert (P, Q) in canonical and nb % 8 == 0 and nb >= P * (Q // 2 + 1)
    assert lib.os2d_dft_channel_stride(225) == 232 and lib.os2d_dft_matrices_bytes(64, 84) > 0
    assert lib.os2d_dft_xscale(60, 80) == 8.0


# ---- refusals: every argument check of abi.hip and head_call.hip that fires before any launch, as (entry point, arguments, return
# code, os2d_last_error()).  The expected values were recorded from the library BEFORE the head call moved into a unit of its own and
# the checks became one-statement refusals; a call that is wrong in two ways (marked 2x) pins the ORDER of the checks.
_OK, _ODD = 0x10000, 0x10008      # a non-null address nobody dereferences (256-byte aligned) and one that is only 8-byte aligned


def _head(**over):
    """Arguments of os2d_head_forward_ex2 for a valid call on fake buffers, with overrides by name."""
    names = ("fm qp w1 b1 w2 b2 w3 b3 A B C H W P inverse stride rec_field loc cls corners workspace workspace_bytes stream precision qs "
             "stage_events chunk_classes status wspec twQ twP wspec2").split()
    a = dict.fromkeys(names, _OK)
    a.update(A=1, B=2, C=16, H=11, W=13, P=6, inverse=0, stride=16, rec_field=16, workspace_bytes=1 << 40, stream=None, precision=0,
             stage_events=None, chunk_classes=None, status=None)
    assert set(over) <= set(names)
    a.update(over)
    return tuple(a[n] for n in names)


def _refusals():
    size = ctypes.byref(ctypes.c_size_t())
    i3 = [ctypes.byref(ctypes.c_int()) for _ in range(3)]
    bad_kind = (ctypes.c_int * 1)(5)
    op_args = (ctypes.c_float * 2)(1.0, 1.0)
    K, N = _OK, None
    pack = (K, K, N, N, N, N, 1e-5)                       # w, b, no BatchNorm, eps
    det = (2, 11, 13, 16, 16, 100.0, 100.0)               # B, H, W, stride, rec_field, img_w, img_h
    out4 = (K, K, K, K, N)                                # out_boxes, out_scores, out_index, out_count, stream
    return [
        # head_call.hip: os2d_head_forward_ex2 in the order of its checks
        ("os2d_head_forward_ex2", _head(fm=N), -1, "os2d_head_forward: null pointer"),
        ("os2d_head_forward_ex2", _head(corners=N, precision=99), -1, "os2d_head_forward: null pointer"),                       # 2x
        ("os2d_head_forward_ex2", _head(workspace=N, A=0), -1, "os2d_head_forward: null pointer"),                              # 2x
        ("os2d_head_forward_ex2", _head(precision=4, wspec=N), -1, "os2d_head_forward: the frequency-domain modes need the weight spectra and the transform tables (fft / fft32: twQ, twP; fftx3: the matrices of os2d_dft_matrices_build as twQ)"),
        ("os2d_head_forward_ex2", _head(precision=4, twQ=N), -1, "os2d_head_forward: the frequency-domain modes need the weight spectra and the transform tables (fft / fft32: twQ, twP; fftx3: the matrices of os2d_dft_matrices_build as twQ)"),
        ("os2d_head_forward_ex2", _head(precision=3, twP=N), -1, "os2d_head_forward: the frequency-domain modes need the weight spectra and the transform tables (fft / fft32: twQ, twP; fftx3: the matrices of os2d_dft_matrices_build as twQ)"),
        ("os2d_head_forward_ex2", _head(precision=5, twP=N, P=5), -1, "os2d_head_forward: the frequency-domain modes need the weight spectra and the transform tables (fft / fft32: twQ, twP; fftx3: the matrices of os2d_dft_matrices_build as twQ)"),                       # 2x
        ("os2d_head_forward_ex2", _head(precision=4, wspec=N, H=0), -1, "os2d_head_forward: the frequency-domain modes need the weight spectra and the transform tables (fft / fft32: twQ, twP; fftx3: the matrices of os2d_dft_matrices_build as twQ)"),                     # 2x: tables before the plan
        ("os2d_head_forward_ex2", _head(precision=99), -1, "os2d_head_forward: unknown precision 99"),
        ("os2d_head_forward_ex2", _head(precision=-1, B=0), -1, "os2d_head_forward: unknown precision -1"),                             # 2x
        ("os2d_head_forward_ex2", _head(W=210), -1, "feature map width 210 > 209: the direct 7x7 kernels keep 3 halo rows of their input in LDS - wider maps need a frequency-domain precision (fftx3 / fft / fft32), which tiles any width up to 3600"),
        ("os2d_head_forward_ex2", _head(W=210, precision=1, qs=N), -1, "feature map width 210 > 209: the direct 7x7 kernels keep 3 halo rows of their input in LDS - wider maps need a frequency-domain precision (fftx3 / fft / fft32), which tiles any width up to 3600"),                      # 2x
        ("os2d_head_forward_ex2", _head(W=210, P=5), -1, "feature map width 210 > 209: the direct 7x7 kernels keep 3 halo rows of their input in LDS - wider maps need a frequency-domain precision (fftx3 / fft / fft32), which tiles any width up to 3600"),                                    # 2x
        ("os2d_head_forward_ex2", _head(precision=4, twP=N, H=0), -3, "os2d_head_forward: no transform plan for a 0x13 map"),                       # 2x: the plan before the shape
        ("os2d_head_forward_ex2", _head(precision=4, H=3000), -3, "os2d_head_forward: no transform plan for a 3000x13 map"),
        ("os2d_head_forward_ex2", _head(precision=3, W=3601), -1, "feature map width 3601 > 3600: beyond what the transform planner of the 7x7 layer tiles (images wider than 57600 px at stride 16 are not supported)"),
        ("os2d_head_forward_ex2", _head(precision=1, qs=N), -1, "os2d_head_forward: precision f16x3 / f16x2 needs the split class operand (os2d_class_split)"),
        ("os2d_head_forward_ex2", _head(precision=2, qs=N, stride=0), -1, "os2d_head_forward: precision f16x3 / f16x2 needs the split class operand (os2d_class_split)"),                   # 2x
        ("os2d_head_forward_ex2", _head(precision=3, qs=N, C=0), -1, "os2d_head_forward: precision f16x3 / f16x2 needs the split class operand (os2d_class_split)"),                        # 2x
        ("os2d_head_forward_ex2", _head(P=5), -1, "bad head shape A=1 B=2 C=16 H=11 W=13 P=5 (need A,B,C,H,W>=1, P in {6,4})"),
        ("os2d_head_forward_ex2", _head(C=0, workspace=_ODD), -1, "bad head shape A=1 B=2 C=0 H=11 W=13 P=6 (need A,B,C,H,W>=1, P in {6,4})"),                           # 2x
        ("os2d_head_forward_ex2", _head(precision=4, W=3601), -1, "feature map width 3601 > 3600: beyond what the transform planner of the 7x7 layer tiles (images wider than 57600 px at stride 16 are not supported)"),
        ("os2d_head_forward_ex2", _head(precision=4, H=2785), -3, "os2d_head_forward: no transform plan for a 2785x13 map"),
        ("os2d_head_forward_ex2", _head(H=2785), -1, "feature map height 2785 > 2784: beyond what the transform planner of the 7x7 layer tiles (images taller than 44544 px at stride 16 are not supported)"),
        ("os2d_head_forward_ex2", _head(precision=5, H=3000, stride=0), -1, "feature map height 3000 > 2784: beyond what the transform planner of the 7x7 layer tiles (images taller than 44544 px at stride 16 are not supported)"),                 # 2x
        ("os2d_head_forward_ex2", _head(stride=0), -1, "os2d_head_forward: bad stride/rec_field 0/16"),
        ("os2d_head_forward_ex2", _head(rec_field=0, workspace=_ODD), -1, "os2d_head_forward: bad stride/rec_field 16/0"),                   # 2x
        ("os2d_head_forward_ex2", _head(workspace=_ODD), -1, "os2d_head_forward: workspace must be 256-byte aligned"),
        ("os2d_head_forward_ex2", _head(workspace=_ODD, workspace_bytes=0), -1, "os2d_head_forward: workspace must be 256-byte aligned"),             # 2x
        ("os2d_head_forward_ex2", _head(workspace_bytes=1000), -2, "os2d_head_forward: workspace too small (1000 B, need >= 694528 B for one class)"),
        ("os2d_head_forward_ex2", _head(workspace_bytes=1000, precision=4), -2, "os2d_head_forward: workspace too small (1000 B, need >= 2887936 B for one class)"),
        ("os2d_head_forward_ex", _head(w3=N)[:-1], -1, "os2d_head_forward: null pointer"),
        ("os2d_head_forward_ex", _head(precision=1, qs=N)[:-1], -1, "os2d_head_forward: precision f16x3 / f16x2 needs the split class operand (os2d_class_split)"),
        ("os2d_head_forward", _head(b3=N)[:23], -1, "os2d_head_forward: null pointer"),
        ("os2d_head_forward", _head(W=210)[:23], -1, "feature map width 210 > 209: the direct 7x7 kernels keep 3 halo rows of their input in LDS - wider maps need a frequency-domain precision (fftx3 / fft / fft32), which tiles any width up to 3600"),
        ("os2d_head_forward", _head(workspace_bytes=8)[:23], -2, "os2d_head_forward: workspace too small (8 B, need >= 694528 B for one class)"),
        ("os2d_head_workspace_bytes", (1, 2, 16, 11, 13, 6, N), -1, "os2d_head_workspace_bytes: null output"),
        ("os2d_head_workspace_bytes", (0, 2, 16, 11, 13, 6, N), -1, "os2d_head_workspace_bytes: null output"),                         # 2x
        ("os2d_head_workspace_bytes", (1, 2, 16, 11, 13, 5, size), -1, "bad head shape A=1 B=2 C=16 H=11 W=13 P=5 (need A,B,C,H,W>=1, P in {6,4})"),
        ("os2d_head_workspace_bytes_ex", (1, 2, 16, 11, 13, 6, 4, N), -1, "os2d_head_workspace_bytes_ex: null output"),
        ("os2d_head_workspace_bytes_ex", (1, 2, 16, 0, 13, 6, 4, size), -1, "bad head shape A=1 B=2 C=16 H=0 W=13 P=6 (need A,B,C,H,W>=1, P in {6,4})"),
        ("os2d_head_workspace_bytes_ex", (1, 2, 16, 11, 3601, 6, 99, size), -1, "feature map width 3601 > 3600: beyond what the transform planner of the 7x7 layer tiles (images wider than 57600 px at stride 16 are not supported)"),             # 2x: an unknown precision is no refusal here
        ("os2d_head_workspace_bytes_ex", (1, 2, 16, 2785, 3601, 6, 1, size), -1, "feature map width 3601 > 3600: beyond what the transform planner of the 7x7 layer tiles (images wider than 57600 px at stride 16 are not supported)"),            # 2x
        ("os2d_head_workspace_bytes_ex", (1, 2, 16, 2785, 13, 6, 3, size), -1, "feature map height 2785 > 2784: beyond what the transform planner of the 7x7 layer tiles (images taller than 44544 px at stride 16 are not supported)"),
        ("os2d_debug_set_dump", (N, 0, K, 16), None, "os2d_debug_set_dump: this library was built without -DOS2D_DIAG_DUMP (diagnostic builds only)"),
        # abi.hip
        ("os2d_pack_conv", (0, 6) + pack + (K, K, N), -1, "os2d_pack_conv: bad layer 0 / P 6"),
        ("os2d_pack_conv", (3, 5) + pack + (K, K, N), -1, "os2d_pack_conv: bad layer 3 / P 5"),
        ("os2d_pack_conv", (4, 6, N, K) + pack[2:] + (K, K, N), -1, "os2d_pack_conv: bad layer 4 / P 6"),                         # 2x
        ("os2d_pack_conv", (1, 6) + pack + (N, K, N), -1, "os2d_pack_conv: null pointer"),
        ("os2d_pack_conv", (1, 6, N, K, K, N, N, N, 1e-5, K, K, N), -1, "os2d_pack_conv: null pointer"),                     # 2x
        ("os2d_pack_conv", (2, 6, K, K, K, K, K, N, 1e-5, K, K, N), -1, "os2d_pack_conv: BatchNorm needs all four of weight/bias/running_mean/running_var"),
        ("os2d_pack_conv_f16x3", (4, 6) + pack + (K, K, K, K, K, N), -1, "os2d_pack_conv_f16x3: bad arguments (layer 4, P 6)"),
        ("os2d_pack_conv_f16x3", (3, 5) + pack + (K, K, N, K, K, N), -1, "os2d_pack_conv_f16x3: bad arguments (layer 3, P 5)"),
        ("os2d_pack_conv_f16x3", (1, 6) + pack + (K, K, N, K, K, N), -1, "os2d_pack_conv_f16x3: bad arguments (layer 1, P 6)"),
        ("os2d_pack_conv_f16x3", (2, 6, K, K, K, N, N, N, 1e-5, K, K, K, K, K, N), -1, "os2d_pack_conv_f16x3: bad arguments (layer 2, P 6)"),
        ("os2d_class_prepare", (K, 0, 3, 3, 1, K, K, N), -1, "os2d_class_prepare: bad arguments (C=0 h=3 w=3)"),
        ("os2d_class_prepare", (K, 16, 3, 3, 1, N, K, N), -1, "os2d_class_prepare: bad arguments (C=16 h=3 w=3)"),
        ("os2d_class_prepare_batch", (K, K, 65536, 16, 1, K, K, K, N), -1, "os2d_class_prepare_batch: bad arguments (B=65536 C=16; at most 65535 classes per call)"),
        ("os2d_class_prepare_batch", (K, N, 2, 16, 1, K, K, K, N), -1, "os2d_class_prepare_batch: bad arguments (B=2 C=16; at most 65535 classes per call)"),
        ("os2d_fm_sumsq", (K, N, 1, 16, 11, 13, N), -1, "os2d_fm_sumsq: bad arguments"),
        ("os2d_fm_sumsq", (K, K, 1, 16, 0, 13, N), -1, "os2d_fm_sumsq: bad arguments"),
        ("os2d_corr", (K, K, N, K, K, 1, 2, 16, 11, 13, N), -1, "os2d_corr: null pointer"),
        ("os2d_corr", (K, K, K, K, K, 1, 0, 16, 11, 13, N), -1, "bad head shape A=1 B=0 C=16 H=11 W=13 P=6 (need A,B,C,H,W>=1, P in {6,4})"),
        ("os2d_corr", (K, K, K, K, N, 1, 2, 16, 11, 3601, N), -1, "os2d_corr: null pointer"),                           # 2x
        ("os2d_corr", (K, K, K, K, K, 1, 2, 16, 2785, 13, N), -1, "feature map height 2785 > 2784: beyond what the transform planner of the 7x7 layer tiles (images taller than 44544 px at stride 16 are not supported)"),
        ("os2d_corr_f16x3", (K, K, K, K, 1, 2, 16, 11, 13, N, 1 << 40, N), -1, "os2d_corr_f16x3: null pointer"),
        ("os2d_corr_f16x3", (K, N, K, K, 0, 2, 16, 11, 13, K, 1 << 40, N), -1, "os2d_corr_f16x3: null pointer"),              # 2x
        ("os2d_corr_f16x3", (K, K, K, K, 1, 2, 16, 11, 3601, K, 0, N), -1, "feature map width 3601 > 3600: beyond what the transform planner of the 7x7 layer tiles (images wider than 57600 px at stride 16 are not supported)"),                  # 2x
        ("os2d_corr_f16x3", (K, K, K, K, 1, 2, 16, 11, 13, K, 100, N), -2, "os2d_corr_f16x3: workspace too small or not 256-byte aligned"),
        ("os2d_corr_f16x3", (K, K, K, K, 1, 2, 16, 11, 13, _ODD, 1 << 40, N), -2, "os2d_corr_f16x3: workspace too small or not 256-byte aligned"),
        ("os2d_corr_f16x3_packed", (K, K, K, N, 1, 2, 16, 11, 13, 1, K, 1 << 40, N), -1, "os2d_corr_f16x3_packed: null pointer"),
        ("os2d_corr_f16x3_packed", (K, K, K, K, 1, 2, 0, 11, 13, 2, K, 1 << 40, N), -1, "bad head shape A=1 B=2 C=0 H=11 W=13 P=6 (need A,B,C,H,W>=1, P in {6,4})"),     # 2x
        ("os2d_corr_f16x3_packed", (K, K, K, K, 1, 2, 16, 11, 13, 2, K, 1 << 40, N), -1, "os2d_corr_f16x3_packed: form 2 (0 padded | 1 packed | -1 the head's choice; + 4: no half tiles at the tail)"),
        ("os2d_corr_f16x3_packed", (K, K, K, K, 1, 2, 16, 11, 13, 8, K, 0, N), -1, "os2d_corr_f16x3_packed: form 8 (0 padded | 1 packed | -1 the head's choice; + 4: no half tiles at the tail)"),          # 2x
        ("os2d_corr_f16x3_packed", (K, K, K, K, 1, 2, 16, 11, 13, -2, K, 1 << 40, N), -1, "os2d_corr_f16x3_packed: form -2 (0 padded | 1 packed | -1 the head's choice; + 4: no half tiles at the tail)"),
        ("os2d_corr_f16x3_packed", (K, K, K, K, 1, 2, 16, 11, 13, 5, K, 100, N), -2, "os2d_corr_f16x3_packed: workspace too small or not 256-byte aligned"),
        ("os2d_corr_f16x3_packed", (K, K, K, K, 1, 2, 16, 11, 13, -1, _ODD, 1 << 40, N), -2, "os2d_corr_f16x3_packed: workspace too small or not 256-byte aligned"),
        ("os2d_corr_normalize", (K, K, 0, 11, 13, N), -1, "os2d_corr_normalize: bad arguments"),
        ("os2d_corr_normalize_f16x3", (K, N, 2, 11, 13, N), -1, "os2d_corr_normalize_f16x3: bad arguments"),
        ("os2d_transform_conv", (3, K, K, K, K, 2, 5, 11, 13, N), -1, "os2d_transform_conv: bad arguments (layer=3 NB=2 P=5)"),
        ("os2d_transform_conv", (1, K, K, K, K, 2, 6, 11, 0, N), -1, "os2d_transform_conv: bad arguments (layer=1 NB=2 P=6)"),
        ("os2d_transform_conv", (5, K, K, K, K, 2, 6, 11, 13, N), -1, "os2d_launch_conv: bad layer 5"),                       # the launcher's own refusal
        ("os2d_transform_conv_f16x3", (0, K, K, K, K, 2, 6, 11, 13, 3, N, N), -1, "os2d_transform_conv_f16x3: bad arguments (layer=0 NB=2 P=6 terms=3)"),
        ("os2d_transform_conv_f16x3", (2, K, K, K, K, 2, 6, 11, 13, 2, N, N), -1, "os2d_transform_conv_f16x3: bad arguments (layer=2 NB=2 P=6 terms=2)"),
        ("os2d_transform_conv_f16x3", (3, K, K, K, K, 2, 5, 11, 13, 3, N, N), -1, "os2d_transform_conv_f16x3: bad arguments (layer=3 NB=2 P=5 terms=3)"),
        ("os2d_transform_conv_f16x3", (1, K, K, K, K, 2, 6, 11, 210, 4, N, N), -1, "os2d_transform_conv_f16x3: bad arguments (layer=1 NB=2 P=6 terms=4)"),          # 2x
        ("os2d_transform_conv_f16x3", (1, K, K, K, K, 2, 6, 11, 210, 2, N, N), -1, "os2d_transform_conv_f16x3: feature map width 210 > 209"),
        ("os2d_transform_conv_f16x3", (2, K, K, K, K, 2, 6, 11, 3601, 3, N, N), -1, "os2d_transform_conv_f16x3: feature map width 3601 > 3600"),
        ("os2d_sample_decode", (K, K, 2, 11, 13, 5, 0, 16, 16, K, K, K, N), -1, "os2d_sample_decode: bad arguments"),
        ("os2d_decode_boxes", (N, 2, 11, 13, 16, 16, 100.0, 100.0, K, N), -1, "os2d_decode_boxes: bad arguments"),
        ("os2d_detect_level", (K, K, 2, 11, 13, 0, 16, 100.0, 100.0, 1.0, 1.0, 0.5, 0.5) + out4, -1, "os2d_detect_level: bad arguments"),
        ("os2d_detect_level_ops", (K, N) + det + (0, N, N, 0.5, 0.5) + out4, -1, "os2d_detect_level_ops: bad arguments"),
        ("os2d_detect_level_ops", (K, K) + det + (-1, N, N, 0.5, 0.5) + out4, -1, "os2d_detect_level_ops: bad transform chain (at most 6 ops of kind 1..4)"),
        ("os2d_detect_level_ops", (K, K) + det + (1, bad_kind, op_args, 0.5, 0.5) + out4, -1, "os2d_detect_level_ops: bad transform chain (at most 6 ops of kind 1..4)"),
        ("os2d_detect_level_ops", (K, K, 0, 11, 13, 16, 16, 100.0, 100.0, 99, N, N, 0.5, 0.5) + out4, -1, "os2d_detect_level_ops: bad arguments"),      # 2x
        ("os2d_nms_workspace_bytes", (2, 8, N), -1, "os2d_nms_workspace_bytes: bad arguments"),
        ("os2d_nms_workspace_bytes", (0, 8, size), -1, "os2d_nms_workspace_bytes: bad arguments"),
        ("os2d_nms", (K, K, 2, 0, 0.5, K, K, K, 1 << 20, N), -1, "os2d_nms: bad arguments"),
        ("os2d_nms", (_ODD, K, 2, 8, 0.5, K, K, K, 1 << 20, N), -1, "os2d_nms: boxes and workspace must be 16-byte aligned"),
        ("os2d_nms", (K, K, 2, 8, 0.5, K, K, _ODD, 0, N), -1, "os2d_nms: boxes and workspace must be 16-byte aligned"),                               # 2x
        ("os2d_nms", (K, K, 2, 8, 0.5, K, K, K, 255, N), -2, "os2d_nms: workspace too small"),
        ("os2d_class_split", (K, K, 0, 16, N), -1, "os2d_class_split: bad arguments"),
        ("os2d_fft_sizes", (11, 13, i3[0], N, i3[2]), -1, "os2d_fft_sizes: null output"),
        ("os2d_fft_sizes", (100000, 100000, i3[0], i3[1], i3[2]), -3, "os2d_fft_sizes: no transform plan for a 100000x100000 map"),
        ("os2d_fft_sizes", (100000, 100000, N, i3[1], i3[2]), -1, "os2d_fft_sizes: null output"),                           # 2x
        ("os2d_fft_tiles", (11, 13, i3[0], i3[1], i3[2], N), -1, "os2d_fft_tiles: null output"),
        ("os2d_fft_tiles", (0, 0, i3[0], i3[1], i3[2], i3[0]), -3, "os2d_fft_tiles: no transform plan for a 0x0 map"),
        ("os2d_fft_forward", (K, K, K, K, N, 2, 225, 11, 13, N), -1, "os2d_fft_forward: bad arguments"),
        ("os2d_fft_inverse_ex", (K, K, K, K, K, 2, 64, 11, 13, N, 0, N), -1, "os2d_fft_inverse: bad arguments (Cout must be 128: the 7x7 layer)"),
        ("os2d_fft_inverse_ex", (K, K, K, K, K, 2, 128, 11, 13, N, 7, N), -1, "os2d_fft_inverse: bad arguments (Cout must be 128: the 7x7 layer)"),
        ("os2d_fft_inverse", (K, K, K, K, K, 0, 128, 11, 13, N, N), -1, "os2d_fft_inverse: bad arguments (Cout must be 128: the 7x7 layer)"),
        ("os2d_spectral_gemm", (K, K, K, 2, 225, 128, 12, N), -1, "os2d_spectral_gemm: bad arguments (NB=2 C=225 Cout=128 nbins=12; nbins must be a multiple of 8)"),
        ("os2d_spectral_gemm", (K, K, _ODD, 2, 225, 128, 16, N), -1, "os2d_spectral_gemm: buffers must be 16-byte aligned"),
        ("os2d_spectral_gemm", (K, _ODD, K, 2, 225, 129, 16, N), -1, "os2d_spectral_gemm: bad arguments (NB=2 C=225 Cout=129 nbins=16; nbins must be a multiple of 8)"),                        # 2x
        ("os2d_spectral_gemm_f16", (K, K, K, 2, 225, 128, 16, 0.0, N), -1, "os2d_spectral_gemm_f16: bad arguments (NB=2 C=225 Cout=128 nbins=16; nbins must be a multiple of 8)"),
        ("os2d_spectral_gemm_f16", (_ODD, K, K, 2, 225, 128, 16, 8.0, N), -1, "os2d_spectral_gemm_f16: buffers must be 16-byte aligned"),
        ("os2d_spectral_gemm_f16_quads", (K, K, K, 2, 225, 128, 4, 8.0, N), -1, "os2d_spectral_gemm_f16_quads: bad arguments (NB=2 C=225 Cout=128 nbins=4)"),
        ("os2d_spectral_gemm_f16_quads", (K, _ODD, K, 2, 225, 128, 16, 8.0, N), -1, "os2d_spectral_gemm_f16_quads: buffers must be 16-byte aligned"),
        ("os2d_spectral_weights_build", (K, K, K, 225, 128, 16, 20, 176, 1, K, N, N), -1, "os2d_spectral_weights_build: bad arguments (C=225 Cout=128 nbins=176)"),
        ("os2d_spectral_weights_build", (K, K, K, 225, 128, 16, 20, 176, 0, _ODD, N, N), -1, "os2d_spectral_weights_build: out must be 16-byte, workspace 8-byte aligned"),
        ("os2d_spectral_weights_build", (K, K, K, 225, 129, 16, 20, 176, 0, _ODD, N, N), -1, "os2d_spectral_weights_build: bad arguments (C=225 Cout=129 nbins=176)"),         # 2x
        ("os2d_spectral_weights_build_dft", (K, K, K, 225, 128, 18, 20, 176, K, K, N), -1, "os2d_spectral_weights_build_dft: bad arguments (C=225 Cout=128 P=18 nbins=176)"),
        ("os2d_spectral_weights_build_dft", (K, K, K, 225, 128, 16, 20, 176, K, N, N), -1, "os2d_spectral_weights_build_dft: bad arguments (C=225 Cout=128 P=16 nbins=176)"),
        ("os2d_spectral_weights_build_dft", (K, K, K, 225, 128, 16, 20, 176, K, 0x10004, N), -1, "os2d_spectral_weights_build_dft: out must be 16-byte, workspace 8-byte aligned"),
        ("os2d_dft_sizes", (11, 13, N, i3[1], i3[2], N), -1, "os2d_dft_sizes: null output"),
        ("os2d_dft_sizes", (100000, 100000, i3[0], i3[1], i3[2], N), -3, "os2d_dft_sizes: no transform plan for a 100000x100000 map"),
        ("os2d_dft_matrices_build", (K, N, 16, 20, K, N), -1, "os2d_dft_matrices_build: bad arguments (out must be 16-byte aligned)"),
        ("os2d_dft_matrices_build", (K, K, 16, 20, _ODD, N), -1, "os2d_dft_matrices_build: bad arguments (out must be 16-byte aligned)"),
        ("os2d_dft_forward", (K, N, K, K, 2, 0, 11, 13, N), -1, "os2d_dft_forward: bad arguments"),
        ("os2d_dft_inverse", (K, K, K, K, 2, 32, 11, 13, N, N), -1, "os2d_dft_inverse: bad arguments (Cout must be 128 or 64: the 7x7 layer / the 5x5 layer 128 -> 64)"),
        ("os2d_dft_inverse_planes", (K, K, K, N, 2, 64, 11, 13, N, N), -1, "os2d_dft_inverse_planes: bad arguments (Cout must be 128 or 64)"),
        ("os2d_alignment_grids", (K, 2, 11, 13, 6, 0, N, N, N), -1, "os2d_alignment_grids: bad arguments"),
        ("os2d_alignment_grids", (K, 2, 11, 13, 5, 0, K, N, N), -1, "os2d_alignment_grids: bad arguments"),
    ]


def test_refusals_keep_their_code_text_and_order(lib_path):
    from os2d_amd import _lib
    lib = _lib.load()
    table = _refusals()
    assert sum(1 for row in table if row[0].startswith("os2d_head_")) >= 30 and len(table) >= 120
    for fn, args, rc, text in table:
        lib.os2d_head_workspace_bytes(1, 1, 1, 1, 1, 6, None)          # another text: the row's call must set its own
        got = getattr(lib, fn)(*args)
        assert (got, lib.os2d_last_error().decode()) == (rc, text), (fn, args)
